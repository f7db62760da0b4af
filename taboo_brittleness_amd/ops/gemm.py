"""The projections of the op layer: one executor for the in-tree MFMA GEMM launches.

:func:`..runtime.gemm_dispatch.plan` turns a shape (or a forced choice) into a short tuple of launches -- the
four-wave kernel (``csrc/gemm4.hip``), the narrow-tile ring GEMM (``csrc/gemm_ring.hip``), split-K ``gemm4`` or
hipBLASLt, each over a row range -- and :func:`run_plan` issues the in-tree ones for the plain, GeGLU and QKV + RoPE +
KV-scatter epilogues, from one A operand or from two (``[x | a2]``, the LoRA-augmented projections).  Everything else
here is a thin caller with its CPU reference branch.  The package's ``__init__`` re-exports the public names.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from ..runtime import gemm_dispatch as _GD
from . import BF16, _k, _out, add_rmsnorm2, rope_qkv_cache
from . import reference as ref

_WS: dict = {}
_WS_KEEP: list = []


def _workspace(tag: str, n: int, device) -> torch.Tensor:
    """fp32 workspace of >= ``n`` floats: one grow-only (doubling) buffer per (tag, device, stream) instead of a
    caching-allocator call per GEMM, so the decode graphs hold a fixed address.  ``"splitk"``: split-K partials
    (``--gemm auto`` only; the default ``tb`` mode never splits K); ``"lens"``: the fused lens GEMM's partials, consumed
    by the merge kernel on the same stream before the next lens GEMM can overwrite them.  Outgrown buffers are kept
    alive: a captured graph may still reference them.  Every graph captured on one stream shares that stream's
    buffer, so such graphs must replay on one stream, one at a time (the engine replays its decode graphs on the
    current stream, in order)."""
    key = (tag, device.index, torch.cuda.current_stream(device).stream_id)
    b = _WS.get(key)
    if b is None or b.numel() < n:
        b = torch.empty(max(n, 2 * b.numel() if b is not None else n), dtype=torch.float32, device=device)
        _WS[key] = b
        _WS_KEEP.append(b)
    return b[:n]


def _splitk_part(x, w, tile_rows: int):
    """``x @ w^T`` split over K into fp32 partials for a consumer that sums them in split order (``add_rmsnorm2_part``,
    ``rope_qkv_cache_part``): no reduction kernel and no bf16 round trip.  Returns ``(partials, splits used)``."""
    K = x.shape[-1]
    M, N = x.numel() // K, w.shape[0]
    ks = int(_k().gemm4_splitk_ks(M, N, K, tile_rows))
    ws = _workspace("splitk", ks * M * N, x.device)
    return ws, int(_k().gemm4_splitk_part(x, w, ws, tile_rows, ks))


def run_plan(launches, x, w, out, epi: int, a2=None, bias=None, thr=None, rope=None) -> None:
    """Issue the in-tree launches of a plan: ``out = epilogue([x | a2] @ w^T)`` with ``epi`` 0 bf16, 1 fp32,
    2 JumpReLU(acc + ``bias``, ``thr``) fp32, 3 GeGLU of interleaved gate|up rows, or 4 QKV + RoPE + KV scatter
    (``out`` is ``q_out`` and ``rope = (pos, slot_of_row, rope_cs, kc, vc, Hq, Hkv)``).  ``a2`` is the optional
    second A source (its columns follow ``x``'s in ``w``'s K; no concatenated copy).  A launch over part of the rows
    takes that slice of every per-row tensor; all in-tree tiles give the same bits, so a split plan equals any single
    launch.  Split-K here means partials plus the ordered reduction (epi 0 / 3, one source)."""
    k = _k()
    M = x.numel() // x.shape[-1]
    pos, slot, cs, kc, vc, Hq, Hkv = rope if rope is not None else (None,) * 7
    for L in launches:
        xa, aa, oa, pa, sa = x, a2, out, pos, slot
        if L.r1 - L.r0 != M:             # a row split: the same rows of every per-row tensor
            xa, aa, oa, pa, sa = (None if t is None else t.reshape(M, -1)[L.r0:L.r1] for t in (x, a2, out, pos, slot))
        if L.family == "g4" and rope is None:
            k.gemm4(xa, w, oa, bias, thr, epi, L.tile, aa)
        elif L.family == "g4":
            k.gemm4_qkv_rope(xa, w, pa, sa, cs, oa, kc, vc, Hq, Hkv, L.tile, aa)
        elif L.family == "ring" and rope is None:
            k.gemm_ring(xa, w, oa, epi, *L.tile, aa)
        elif L.family == "ring":
            k.gemm_ring_qkv_rope(xa, w, pa, sa, cs, oa, kc, vc, Hq, Hkv, *L.tile, aa)
        elif L.family == "splitk" and a2 is None and rope is None:
            N, K = w.shape
            ks = int(k.gemm4_splitk_ks(M, N, K, L.tile))
            k.gemm4_splitk(x, w, out, _workspace("splitk", ks * M * N, x.device), epi, L.tile, ks)
        else:
            raise ValueError(f"no in-tree GEMM launch for {L!r} (epilogue {epi}, {'two' if a2 is not None else 'one'} "
                             "A source)")


def _ring_ok(M: int, N: int, K: int):
    return lambda epi, bm, bn, var: _k().gemm_ring_ok(M, N, K, epi, bm, bn, var)


def tb_gemm(x, w, out, bias, thr, epi: int, choice, a2=None) -> None:
    """One in-tree MFMA GEMM with a forced ``runtime.gemm_dispatch`` choice: ``"g256"`` / ``"g128"`` the four-wave
    kernel (csrc/gemm4.hip), ``"gs"`` its rounds-model tile height(s); ``"k256"`` / ``"k128"`` the four-wave kernel
    split over K (thin grids; fp32 partials + ordered reduction, epi 0 / 3 only, not bit-identical to the unsplit
    kernels); ``"r<bm>x<bn>[b|c]"`` the narrow-tile ring GEMM (csrc/gemm_ring.hip, decode / mid M, epi 0 / 3,
    bit-identical to the four-wave kernel).  ``a2``: the optional second A source (see :func:`gemm_l2a`)."""
    run_plan(_GD.plan(x.numel() // x.shape[-1], *w.shape, choice=choice), x, w, out, int(epi), a2, bias, thr)


def gemm_l2a(x: torch.Tensor, a2: torch.Tensor, w: torch.Tensor, out: torch.Tensor, epi: int, choice) -> torch.Tensor:
    """``out = [x | a2] @ w^T`` (epi 0) or its GeGLU (epi 3, interleaved gate|up rows) on the in-tree GEMMs with two A
    sources and a forced choice (``"g256"`` / ``"g128"`` / ``"gs"`` / ``"r<bm>x<bn>b"``: the 144 KB ring is the only
    one built with two sources)."""
    tb_gemm(x, w, out, None, None, epi, choice, a2=a2)
    return out


def linear(x: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None, choice=None) -> torch.Tensor:
    """y = x @ w^T.  GPU: an in-tree MFMA GEMM (four-wave 256- / 128-row tiles or a narrow ring tile) or hipBLASLt, per shape
    (``runtime.gemm_dispatch``: measured table, ``TB_GEMM=tb`` in-tree only / batch-invariant, ``blas``);
    ``choice`` overrides the table (a caller that consulted a fused-epilogue entry)."""
    if x.is_cuda and x.dtype == BF16 and w.dtype == BF16:
        K = x.shape[-1]
        M, N = x.numel() // K, w.shape[0]
        if M > 0 and x.is_contiguous() and w.is_contiguous() and (out is None or out.is_contiguous()) and \
                _k().gemm4_ok(M, N, K):
            p = _GD.plan(M, N, K, 0, choice=choice)
            if p[0].family != "blas":
                out = _out(out, x.shape[:-1] + (N,), BF16, x.device)
                run_plan(p, x, w, out, 0)
                return out
    if out is not None:
        return torch.matmul(x, w.t(), out=out)
    return F.linear(x, w)


def linear_add_rmsnorm2(a, w, h, w_post, w_next, eps, out=None, o_ws=None):
    """``h += post_norm(a @ w^T)`` (in place); returns the next pre-norm of ``h`` -- a block's o_proj / down
    projection and its residual norm (table key epilogue 5 when measured, else the plain projection's).  When the
    dispatch runs the projection split over K (``"k256"`` / ``"k128"``, thin grids), its fp32 partials go straight
    into ``add_rmsnorm2_part``, which sums them in split order and rounds to bf16 exactly as the split-K reduction
    would: no reduction kernel, no bf16 ``o`` round trip.  Otherwise ``linear`` into ``o_ws`` then ``add_rmsnorm2``."""
    c = None
    if a.is_cuda and a.dtype == BF16 and w.dtype == BF16 and a.is_contiguous() and w.is_contiguous():
        K = a.shape[-1]
        M, N = a.numel() // K, w.shape[0]
        if M > 0 and _k().gemm4_ok(M, N, K):
            c = _GD.resolve(M, N, K, 5)
            if c.kind == "k":
                ws, ks = _splitk_part(a, w, c.tile)
                out = _out(out, h.shape, h.dtype, h.device)
                _k().add_rmsnorm2_part(h, ws, ks, w_post, w_next, out, float(eps))
                return out
    return add_rmsnorm2(h, linear(a, w, out=o_ws, choice=c), w_post, w_next, eps, out=out)


_ROPE_CS: dict = {}


def rope_cs(cos_t: torch.Tensor, sin_t: torch.Tensor) -> torch.Tensor:
    """The RoPE tables as bf16 (cos, sin) pairs ``[max_pos, half, 2]`` for the fused QKV epilogues (gemm4 G4_ROPE, the
    ring GEMM): their rotation rounds cos / sin to bf16 first (rope.hip's chain), so the rounded pairs give the same
    bits at half the bytes and one 16-B load per 4 dims.  Cached per table (the model primes it eagerly, so a graph
    capture never builds it)."""
    key = (cos_t.data_ptr(), sin_t.data_ptr(), tuple(cos_t.shape), cos_t.device)
    t = _ROPE_CS.get(key)
    if t is None:
        t = torch.stack((cos_t, sin_t), -1).to(BF16).contiguous()
        _ROPE_CS[key] = t
    return t


def qkv_rope_cache(x, wqkv, pos, slot_of_row, cos_t, sin_t, kc, vc, Hq, Hkv, HD, q_out=None, qkv_ws=None):
    """``rope_qkv_cache(linear(x, wqkv))`` (head_dim 256 on the GPU; table key epilogue 4, measured against
    hipBLASLt + ``rope_qkv_cache``, where it covers the row count, else the plain projection's; ``TB_GEMM=tb`` always
    fuses: one K order for every row): the fused gemm4 G4_ROPE / ring epilogue (bit-identical to the unfused pair), the
    split-K partials summed inside the RoPE / KV-scatter pass (thin decode grids), or the projection into ``qkv_ws``
    then ``rope_qkv_cache``."""
    M = pos.numel()
    N, K = wqkv.shape
    if x.is_cuda and HD == 256 and M > 0 and _k().gemm4_ok(M, N, K):
        p = _GD.plan(M, N, K, 4, ring_ok=_ring_ok(M, N, K))
        if p[0].family != "blas":
            q_out = _out(q_out, (M, Hq, HD), x.dtype, x.device)
            if p[0].family == "splitk":
                ws, ks = _splitk_part(x, wqkv, p[0].tile)
                _k().rope_qkv_cache_part(ws, ks, pos, slot_of_row, cos_t, sin_t, q_out, kc, vc, int(Hq), int(Hkv),
                                         int(HD))
            else:
                run_plan(p, x, wqkv, q_out, 4, rope=(pos, slot_of_row, rope_cs(cos_t, sin_t), kc, vc, int(Hq), int(Hkv)))
            return q_out
    qkv = linear(x, wqkv, out=qkv_ws)
    return rope_qkv_cache(qkv, pos, slot_of_row, cos_t, sin_t, kc, vc, Hq, Hkv, HD, q_out=q_out)


# ------------------------------------------------------------ two-source projections (models/lora.py LoRABank.fused)
def _cat_ref(x, a2):
    return torch.cat([x.reshape(-1, x.shape[-1]), a2.reshape(-1, a2.shape[-1]).to(x.dtype)], -1)


def linear_lora(x, a2, w, out=None, epi: int = 0):
    """``[x | a2] @ w^T`` (the LoRA-augmented projection; ``epi`` 5 picks the o / down table entry): the dispatch
    table's choice for the base shape on the in-tree GEMMs with two A sources, never split-K / hipBLASLt (one K
    order)."""
    N, K = w.shape
    M = x.numel() // x.shape[-1]
    if x.is_cuda and _k().gemm4_ok(M, N, K):
        out = _out(out, x.shape[:-1] + (N,), BF16, x.device)
        run_plan(_GD.plan(M, N, K, epi, True, _ring_ok(M, N, K)), x, w, out, 0, a2=a2)
        return out
    y = (_cat_ref(x, a2).float() @ w.float().t()).to(BF16).view(x.shape[:-1] + (N,))
    if out is not None:
        out.copy_(y)
        return out
    return y


def linear_lora_add_rmsnorm2(a, a2, w, h, w_post, w_next, eps, out=None, o_ws=None):
    """:func:`linear_add_rmsnorm2` of the LoRA-augmented o / down projection (never split over K)."""
    return add_rmsnorm2(h, linear_lora(a, a2, w, out=o_ws, epi=5), w_post, w_next, eps, out=out)


def gate_up_geglu_lora(x, a2, w_il, out=None):
    """:func:`gate_up_geglu` of ``[x | a2]`` (the bank's gate|up deltas folded into the GeGLU GEMM's K)."""
    F2, K = w_il.shape
    M = x.numel() // x.shape[-1]
    if x.is_cuda:
        out = _out(out, x.shape[:-1] + (F2 // 2,), BF16, x.device)
        run_plan(_GD.plan(M, F2, K, 3, True, _ring_ok(M, F2, K)), x, w_il, out, 3, a2=a2)
        return out
    return gate_up_geglu(_cat_ref(x, a2).view(x.shape[:-1] + (K,)), w_il, out)


def qkv_rope_cache_lora(x, a2, wqkv, pos, slot_of_row, cos_t, sin_t, kc, vc, Hq, Hkv, HD, q_out=None):
    """:func:`qkv_rope_cache` of ``[x | a2]``: the fused QKV + RoPE + KV-scatter epilogue with the bank's q / k / v
    deltas in the same GEMM (gemm4 G4_ROPE or ring RG_ROPE, two A sources)."""
    M = pos.numel()
    N, K = wqkv.shape
    if not x.is_cuda or HD != 256:
        return qkv_rope_cache(_cat_ref(x, a2), wqkv, pos, slot_of_row, cos_t, sin_t, kc, vc, Hq, Hkv, HD, q_out=q_out)
    q_out = _out(q_out, (M, Hq, HD), x.dtype, x.device)
    run_plan(_GD.plan(M, N, K, 4, True, _ring_ok(M, N, K)), x, wqkv, q_out, 4, a2=a2,
             rope=(pos, slot_of_row, rope_cs(cos_t, sin_t), kc, vc, int(Hq), int(Hkv)))
    return q_out


# ------------------------------------------------------------ SAE encode, gate|up + GeGLU
def gemm_nt(A, W, epi=0, bias=None, thr=None, out=None):
    """C = A @ W^T on an MFMA kernel; epi 0 = bf16, 1 = fp32, 2 = JumpReLU(acc + bias, thr) fp32.
    Shapes with N % 256 == 0 and K % 64 == 0 (the SAE encode: N = 16384, K = 3584) run the four-wave
    256x256 kernel (csrc/gemm4.hip); others the 128x128 ``gemm_nt`` kernel (csrc/sae.hip)."""
    M = A.numel() // A.shape[-1]
    N = W.shape[0]
    if A.is_cuda:
        out = _out(out, (M, N), BF16 if epi == 0 else torch.float32, A.device)
        if _k().gemm4_ok(M, N, A.shape[-1]) and A.is_contiguous():
            tb_gemm(A, W, out, bias, thr, int(epi), _GD.fill_choice(max(M, 4096), N))
        else:
            _k().gemm_nt(A, W, out, bias, thr, int(epi))
        return out
    y = ref.gemm_nt(A, W, epi, bias, thr)
    if out is not None:
        out.copy_(y.view_as(out))
        return out
    return y


def geglu_interleave_index(F: int, device=None) -> torch.Tensor:
    """Row order of a gate|up weight ``[2F, K]`` for the fused GeGLU epilogues (epi 3):
    every 256-row tile holds features ``f0 .. f0+127`` as two 128-row wave-group slices
    ``[gate 64 | up 64]``, so a lane's gate and up accumulators of the same feature land in the same
    lane (csrc/gemm4.hip G4_GEGLU, csrc/gemm_ring.hip RG_GEGLU).  Needs F % 128 == 0."""
    assert F % 128 == 0, "fused GeGLU needs ffn % 128 == 0"
    p = torch.arange(2 * F)
    tile, q = p // 256, p % 256
    g, half, rest = q // 128, (q // 64) % 2, q % 64
    return (half * F + tile * 128 + g * 64 + rest).to(device)


def fused_geglu_wins(x: torch.Tensor, spec) -> bool:
    """Whether the gate|up GEMM of ``x``'s rows runs fused with the GeGLU (in-tree kernel) rather than as
    ``linear`` + ``geglu`` (the dispatch table's epilogue-3 entry; ``TB_GEMM=tb`` always, ``blas`` never)."""
    M = x.numel() // x.shape[-1]
    return _GD.choose(M, 2 * spec.ffn, x.shape[-1], 3) != "blas"


def gate_up_geglu(x: torch.Tensor, w_gu_interleaved: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``geglu(x @ w_gu^T)`` in one in-tree MFMA GEMM (gemm4 G4_GEGLU or ring RG_GEGLU) whose epilogue applies GeGLU to the fp32 accumulators
    (rounded to bf16 first, so the result equals the unfused bf16 graph up to the GEMM's summation order);
    ``w_gu_interleaved = w_gu[geglu_interleave_index(F)]``."""
    K = x.shape[-1]
    M = x.numel() // K
    F = w_gu_interleaved.shape[0] // 2
    if x.is_cuda:
        out = _out(out, x.shape[:-1] + (F,), BF16, x.device)
        run_plan(_GD.plan(M, 2 * F, K, 3), x, w_gu_interleaved, out, 3)
        return out
    inv = torch.argsort(geglu_interleave_index(F))
    y = ref.geglu((x.reshape(M, -1).float() @ w_gu_interleaved[inv].float().T).to(BF16)).view(x.shape[:-1] + (F,))
    if out is not None:
        out.copy_(y)
        return out
    return y
