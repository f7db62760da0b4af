"""Device-dispatching op layer.

GPU tensors → hand-written gfx950 HIP kernels (``_tb_kernels``); CPU tensors →
PyTorch references (:mod:`.reference`).  The projections (``linear``, its fused QKV + RoPE, gate|up + GeGLU and
residual-norm forms, their two-source LoRA twins, ``gemm_nt``) live in :mod:`.gemm` and are re-exported here: the
in-tree MFMA GEMMs (the four-wave kernel ``csrc/gemm4.hip`` and the narrow-tile ring GEMM ``csrc/gemm_ring.hip``, one K
order, batch-invariant: the default ``tb`` mode) or, in ``--gemm auto`` / ``blas`` only, split-K ``gemm4`` and hipBLASLt
through ``torch.matmul``, as :func:`..runtime.gemm_dispatch.plan` chooses per shape.  Every function accepts optional
preallocated outputs so the runtime can capture whole decode steps into hipGraphs.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from ..runtime import gemm_dispatch as _GD
from . import reference as ref
from ._ext import available as ext_available  # noqa: F401
from ._ext import kernels as _k

BF16 = torch.bfloat16


def _out(out: Optional[torch.Tensor], shape, dtype, device) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    return out


_CAP_TABLES = {}


def _softcap_table(cap: float, device) -> None:
    """Register the exact bf16 softcap table for ``cap`` on ``device`` (built once with the reference
    op, so the GPU lookup reproduces it bit for bit); used by every emulated-softcap vocab kernel."""
    key = (float(cap), device.index if device.index is not None else torch.cuda.current_device())
    if key in _CAP_TABLES or not (cap > 0):
        return
    bits = torch.arange(32768, dtype=torch.int32).to(torch.int16)
    x = bits.view(BF16)
    tab_cpu = ref.softcap_bf16(x, float(cap)).to(BF16).contiguous()
    tab = tab_cpu.to(device)
    _k().register_softcap_table(tab, float(cap))
    _CAP_TABLES[key] = tab        # keep alive: kernels (and captured graphs) hold its pointer
    split = softcap_compact_split(tab_cpu, float(cap))
    if split is not None:
        lo, hi, sat = split
        tc = tab_cpu[lo:hi].contiguous().to(device)
        if _k().register_softcap_compact(tc, float(cap), lo, hi, sat):
            _CAP_TABLES[key + ("compact",)] = tc


def softcap_compact_split(tab: torch.Tensor, cap: float):
    """``(lo, hi, sat)`` of the compact exact softcap (csrc/lens.hip CapC) for the 32768-entry reference table
    ``tab`` of the non-negative bf16 inputs, or None: every bit pattern below ``lo`` must equal
    ``rbf(rbf(x * (1/cap)) * cap)`` (fp32 multiply by the fp32 reciprocal, as the kernel does) and every finite
    pattern from ``hi`` on (and +inf) the saturated value — checked exhaustively here, so the kernel reproduces the
    table bit for bit."""
    t = tab.float()
    xs = torch.arange(32768, dtype=torch.int32).to(torch.int16).view(BF16).float()
    rc = torch.tensor(1.0 / cap, dtype=torch.float32)
    arith = ((xs * rc).to(BF16).float() * torch.tensor(cap, dtype=torch.float32)).to(BF16).float()
    ok = arith == t
    fin = 0x7F80                                   # +inf; patterns above are NaNs
    bad = (~ok[:fin]).nonzero()
    lo = int(bad[0]) if bad.numel() else fin
    sat = float(t[fin])
    diff = (t[: fin + 1] != sat).nonzero()
    hi = int(diff[-1]) + 1 if diff.numel() else 0
    hi = max(hi, lo)
    if hi - lo > 2048 or not torch.isnan(t[fin + 1:]).all():
        return None
    return lo, hi, sat


def softcap_values(v: torch.Tensor, cap: float) -> torch.Tensor:
    """fp32 values of the exact bf16 final softcap of bf16 logits ``v`` (any shape): the registered table on the
    GPU (bit-identical to the vocab kernels), the reference op on the CPU."""
    if not (cap > 0):
        return v.float()
    if v.is_cuda:
        _softcap_table(cap, v.device)
        y = torch.empty(v.shape, dtype=torch.float32, device=v.device)
        if _k().softcap_compact(v.contiguous(), y, float(cap)):     # compact exact form (csrc/lens.hip)
            return y
        tab = _CAP_TABLES[(float(cap), v.device.index if v.device.index is not None else torch.cuda.current_device())]
        b = v.contiguous().view(torch.int16).to(torch.int32)
        mag = tab.view(torch.int16).to(torch.int32)[b & 0x7FFF]
        bits = ((mag & 0x7FFF) | (b & 0x8000)) << 16
        return bits.view(torch.float32)
    return ref.softcap_bf16(v, float(cap)).float()


def rmsnorm(x, w, eps, out=None):
    if x.is_cuda:
        out = _out(out, x.shape, x.dtype, x.device)
        _k().rmsnorm(x, w, out, float(eps))
        return out
    y = ref.rmsnorm(x, w, eps)
    if out is not None:
        out.copy_(y)
        return out
    return y


def add_rmsnorm2(h, o, w_post, w_next, eps, out=None):
    """h += post_norm(o) (in place); returns next pre-norm of h."""
    if h.is_cuda:
        out = _out(out, h.shape, h.dtype, h.device)
        _k().add_rmsnorm2(h, o, w_post, w_next, out, float(eps))
        return out
    y = ref.add_rmsnorm2(h, o, w_post, w_next, eps)
    if out is not None:
        out.copy_(y)
        return out
    return y


def embed_rmsnorm(ids, E, w, scale, eps, h_out=None, x_out=None):
    if E.is_cuda:
        M, D = ids.numel(), E.shape[1]
        h_out = _out(h_out, (M, D), E.dtype, E.device)
        x_out = _out(x_out, (M, D), E.dtype, E.device)
        _k().embed_rmsnorm(ids, E, w, h_out, x_out, float(scale), float(eps))
        return h_out, x_out
    h, x = ref.embed_rmsnorm(ids, E, w, scale, eps)
    if h_out is not None:
        h_out.copy_(h.view_as(h_out))
        x_out.copy_(x.view_as(x_out))
        return h_out, x_out
    return h, x


def rope_qkv_cache(qkv, pos, slot_of_row, cos_t, sin_t, kc, vc, Hq, Hkv, HD, q_out=None):
    if qkv.is_cuda:
        q_out = _out(q_out, (pos.numel(), Hq, HD), qkv.dtype, qkv.device)
        _k().rope_qkv_cache(qkv, pos, slot_of_row, cos_t, sin_t, q_out, kc, vc, int(Hq), int(Hkv), int(HD))
        return q_out
    q = ref.rope_qkv_cache(qkv, pos, slot_of_row, cos_t, sin_t, kc, vc, Hq, Hkv, HD)
    if q_out is not None:
        q_out.copy_(q.view_as(q_out))
        return q_out
    return q


# the projections (ops/gemm.py builds on the helpers above, so it is imported here and not at the top)
from .gemm import (_workspace, fused_geglu_wins, gate_up_geglu, gate_up_geglu_lora,  # noqa: E402,F401
                   geglu_interleave_index, gemm_l2a, gemm_nt, linear, linear_add_rmsnorm2, linear_lora,
                   linear_lora_add_rmsnorm2, qkv_rope_cache, qkv_rope_cache_lora, rope_cs, run_plan, tb_gemm)


def row_combine(ptr: torch.Tensor, coef: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """``out[b] = sum_t coef[b, t] * row(ptr[b, t])``: fp32 rows of ``out``'s width at device addresses ``ptr`` (int64
    ``[B, T]``), the terms of a row summed in order (csrc/elementwise.hip; GPU only -- the caller's CPU path keeps
    its dense matmul)."""
    _k().row_combine(ptr, coef, out)
    return out


# ------------------------------------------------------------ multi-adapter LoRA (models/lora.py LoRABank.fused)
# earlier directions whose table rows the basis kernel loads together (1 / 2 / 4; the same bits; tools/basis_bench.py)
RANDOM_BASIS_QU = 1


def random_basis(seeds: torch.Tensor, ranks: torch.Tensor, rows: torch.Tensor, table: torch.Tensor,
                 qu: Optional[int] = None) -> torch.Tensor:
    """Random orthonormal bases into an fp32 ``[R, D]`` table: basis ``i`` (``ranks[i]`` directions, seed
    ``seeds[i]``) fills rows ``rows[i] .. rows[i] + ranks[i] - 1`` (csrc/basis.hip, one workgroup per basis; the
    numpy reference of the same algorithm on CPU tables)."""
    if table.is_cuda:
        _k().random_basis(seeds, ranks, rows, table, int(qu or RANDOM_BASIS_QU))
        return table
    D = table.shape[-1]
    for s, r, o in zip(seeds.tolist(), ranks.tolist(), rows.tolist()):
        table[o:o + r] = torch.from_numpy(ref.random_basis(D, r, s))
    return table


_EMPTY_F32: dict = {}

def lora_t_plan(M: int, K: int, nt: int):
    """(split, bm, bn) of the LoRA T launch (measured per projection and row count, tools/lora_t_bench.py ->
    profiles/r6/lorachunk2/lora_t.jsonl; every form gives the same bits).  One column tile over all ``nt`` used
    columns (x read once).  Unsplit, a tile's time is its K chain's latency, so the row tile is the smallest that
    keeps the grid within one round of 256 workgroups; the K chunks are split over workgroups (fp32 chunk sums +
    the ordered fold kernel) while even 16-row tiles leave the chip under one round, and for the long K = 14336
    chain up to 4096 rows."""
    bn = nt if nt in (32, 64, 96) else 32
    cols = nt // bn
    split = -(-M // 16) * cols < 256 or (K >= 8192 and M <= 4096)
    if split:
        bm = 32 if M <= 1024 else (64 if M <= 2048 else 128)
        if K >= 8192 and M > 256:
            bm = 64 if M <= 512 else 128
        if M <= 512:
            bn, cols = 32, nt // 32
    else:
        cand = (16, 32, 64, 128) if bn == 64 else (16, 32, 64)
        bm = next((b for b in cand if -(-M // b) * cols <= 256), cand[-1])
    if bn == 96 and bm > 64:
        bm = 64
    return split, bm, bn


def lora_t(x: torch.Tensor, a_all: torch.Tensor, adapter: torch.Tensor, nsr: int, nr: int, r: int,
           out: Optional[torch.Tensor] = None, split: Optional[bool] = None, bm: Optional[int] = None,
           bn: Optional[int] = None) -> torch.Tensor:
    """The bank's masked down-projection ``T [M, KP]``: column ``c`` = ``x . a_all[c]`` rounded to bf16 where it belongs
    to the row's adapter (``c < nsr`` and ``(c % nr) // r == adapter[row]``), else 0 (``adapter < 0``: all 0).  GPU:
    the ring GEMM's RG_LMASK epilogue (csrc/gemm_ring.hip), batch-invariant, over the first ``nsr`` columns rounded
    up to 32 only (the rest of ``a_all`` is zero padding): columns past those are NOT written, so a caller's ``out``
    must hold zeros there (``out=None`` allocates zeros; models/gemma2.py keeps one zeroed buffer per projection).
    K runs in fixed 512-deep chunks summed in order, so the K chain can be split over workgroups at decode row counts
    (``split``; default: :func:`lora_t_plan`, as are the tile ``bm`` x ``bn``) with the same bits as the unsplit
    launch.
    CPU: the fp32 reference."""
    K = x.shape[-1]
    M, N = x.numel() // K, a_all.shape[0]
    if x.is_cuda:
        out = out if out is not None else torch.zeros(M, N, dtype=BF16, device=x.device)
        nt = min(N, -(-int(nsr) // 32) * 32)
        if nt == 0:
            return out
        psplit, pbm, pbn = lora_t_plan(M, K, nt)
        if split is None:
            split = psplit
        elif split != psplit:
            pbm = 32 if split else 16
        bm = bm or pbm
        bn = bn or pbn
        k = _k()
        # (split: the chunk sums from the caching allocator -- graph-private memory inside a capture)
        if split:
            part = torch.empty(k.lora_t_chunks(K), M, nt, dtype=torch.float32, device=x.device)
        else:
            part = _EMPTY_F32.get(x.device)
            if part is None:
                part = _EMPTY_F32[x.device] = torch.empty(0, dtype=torch.float32, device=x.device)
        k.lora_t(x.reshape(M, K), a_all[:nt], out, adapter, int(nsr), int(nr), int(r), bm, bn, part)
        return out
    out = _out(out, (M, N), BF16, x.device)
    out.copy_(ref.lora_t(x.reshape(M, K), a_all, adapter, nsr, nr, r))
    return out


def decode_pre(step_idx, tf_tgt, tf_step, nb: int) -> None:
    """Greedy decode step, before the head: ``tf_step[r] = tf_tgt[r, min(step_idx[r], W - 1)]`` (``r < nb``)."""
    if tf_tgt.is_cuda:
        _k().decode_pre(step_idx, tf_tgt, tf_step, int(nb))
        return
    ref.decode_pre(step_idx, tf_tgt, tf_step, nb)


def decode_post(nxt, nll, tf_nll, done, step_idx, out_tok, out_nll, out_tf_nll, stop, tok, pos, nb: int,
                pad: int) -> None:
    """Greedy decode step, after the head, rows ``< nb``: the token (``pad`` once done) and its NLLs into output
    column ``min(step_idx, W - 1)``, ``done |= token in stop``, then next token, position + 1, column + 1 -- one
    kernel instead of ~12 PyTorch ones per captured step."""
    if nxt.is_cuda:
        _k().decode_post(nxt, nll, tf_nll, done, step_idx, out_tok, out_nll, out_tf_nll, stop, tok, pos, int(nb),
                         int(pad))
        return
    ref.decode_post(nxt, nll, tf_nll, done, step_idx, out_tok, out_nll, out_tf_nll, stop, tok, pos, nb, pad)


def share_lo_gather(rep, U, tok, pos, slot, s_tok, s_pos, s_slot, kp_slot, kp_len_lo, l_slot, l_len_lo, nb: int,
                    S: int) -> None:
    """Prefix-trie decode, blocks ``0..l``: lo row ``i < nb`` takes token, slot (and shared-prefix slot / length)
    of its group representative ``rep[i]``, and its position when ``i < U`` (else ``S``: parked)."""
    if tok.is_cuda:
        _k().share_lo_gather(rep, U, tok, pos, slot, s_tok, s_pos, s_slot, kp_slot, kp_len_lo, l_slot, l_len_lo,
                             int(nb), int(S))
        return
    ref.share_lo_gather(rep, U, tok, pos, slot, s_tok, s_pos, s_slot, kp_slot, kp_len_lo, l_slot, l_len_lo, nb, S)


def capture_rows(store, h, pos, slot, B: int, T: int) -> None:
    """``store[slot[b], p] = h[b * T + t]`` for ``p = pos[b, t]`` in ``[0, S1 - 1)``, else into the slot's scratch
    row ``S1 - 1`` (``store [slots, S1, D]`` bf16; one kernel, graph-capturable)."""
    if h.is_cuda:
        _k().capture_rows(store, h, pos.reshape(-1), slot.reshape(-1), int(T))
        return
    ref.capture_rows(store, h, pos, slot, B, T)


def row_gather(src, idx, out) -> None:
    """``out[i] = src[idx[i]]`` (bf16 rows of the last dimension; int32 / int64 indices)."""
    if src.is_cuda:
        _k().row_gather(src, idx, out)
        return
    torch.index_select(src.reshape(-1, src.shape[-1]), 0, idx.long(), out=out[: idx.numel()])


def share_group(gid, tok, rep, grp, src, U, nb: int, act: int, first: bool, vocab: int) -> bool:
    """Prefix-trie regrouping of rows ``< nb`` by (group ``gid``, token ``tok``) -- rows ``>= act`` form one parked
    group -- in one kernel (csrc/decode_step.hip): dense ``gid`` / ``grp``, each group's first row in ``rep``, the
    K/V fan-out source ``src`` (-1 for representatives and parked rows), the group count in ``U``.  Returns False
    (nothing done) off the GPU or past the kernel's row limit; the caller then runs the PyTorch version."""
    if not tok.is_cuda or nb > _share_group_max():
        return False
    _k().share_group(gid, tok.reshape(-1), rep, grp, src, U, int(nb), int(act), bool(first), int(vocab))
    return True


_SG_MAX = []


def _share_group_max() -> int:
    if not _SG_MAX:
        _SG_MAX.append(int(_k().share_group_max_rows()))
    return _SG_MAX[0]


def kv_fanout(kc, vc, src_row, slot, pos, nlayers: int) -> None:
    """Prefix-trie decode: copy the K/V of layers ``< nlayers`` that row ``src_row[r]`` wrote at its position
    into row ``r``'s own slot at ``r``'s position (``kc/vc [L, slots, Hkv, S, HD]``; ``src_row < 0`` or
    ``== r``: nothing).  A source row must not itself be a copy target (representatives only), so the
    rows are independent."""
    if kc.is_cuda:
        _k().kv_fanout(kc, vc, src_row, slot, pos, int(nlayers))
        return
    ref.kv_fanout(kc, vc, src_row, slot, pos, nlayers)


def attention(q, kc, vc, pos, slot, B, T, scale, softcap, window, out=None, prefix=None):
    """``prefix = (pk, pv, pslot, plen)`` (decode, T == 1): row ``b`` reads keys ``[0, plen[b])`` from slot
    ``pslot[b]`` of the shared prefix cache ``pk/pv [P, Hkv, S, HD]`` instead of its own slot."""
    if q.is_cuda:
        out = _out(out, (B * T, q.numel() // (B * T)), q.dtype, q.device)
        if prefix is not None:
            assert T == 1, "shared-prefix attention is decode-only"
            pk, pv, ps, pl = prefix
            _k().attention_prefix(q, kc, vc, out, pos, slot, int(B), float(scale), float(softcap), int(window),
                                  pk, pv, ps, pl)
            return out
        _k().attention(q, kc, vc, out, pos, slot, int(B), int(T), float(scale), float(softcap), int(window))
        return out
    o = ref.attention(q, kc, vc, pos, slot, B, T, scale, softcap, window,
                      prefix=prefix)
    if out is not None:
        out.copy_(o.view_as(out))
        return out
    return o


def attention_varlen(q, kc, vc, pos, slot_rows, blk, scale, softcap, window, out=None, prefix_kv=None):
    """Attention over packed rows ``q [M, Hq, HD]``: row ``i`` reads cache slot ``slot_rows[i]`` up to
    ``pos[i]``.  ``blk [nblk, 3] = (first row, rows, slot)`` groups consecutive rows of one sequence
    (<= 16 / GQA-ratio rows each) for the MFMA kernel; the CPU path only needs ``slot_rows``.
    ``prefix_kv = (pk, pv)`` with ``blk [nblk, 5]`` (+ prefix slot, prefix length): a block's keys below
    its prefix length come from that slot of the shared prefix cache ``pk/pv [P, Hkv, S, HD]``.

    Exactness: over a cache of at most 512 positions (``S <= 512``) a packed row is bit-identical to the same query
    run as a decode row (``attention`` with ``T == 1``).  Over a longer cache the rows run the prefill kernel's online
    softmax, which agrees with the decode to bf16 rounding only, not bit for bit."""
    M = pos.numel()
    if q.is_cuda:
        out = _out(out, (M, q.numel() // M), q.dtype, q.device)
        if prefix_kv is not None:
            _k().attention_varlen_prefix(q, kc, vc, out, pos, blk, float(scale), float(softcap), int(window),
                                         prefix_kv[0], prefix_kv[1])
            return out
        _k().attention_varlen(q, kc, vc, out, pos, blk, float(scale), float(softcap), int(window))
        return out
    pre = None
    if prefix_kv is not None:
        ps = torch.zeros(M, dtype=torch.long)
        pl = torch.zeros(M, dtype=torch.long)
        for r0, n, _, s_, l_ in blk.cpu().long().tolist():
            ps[r0:r0 + n] = s_
            pl[r0:r0 + n] = l_
        pre = (prefix_kv[0], prefix_kv[1], ps, pl)
    o = ref.attention(q, kc, vc, pos, slot_rows, M, 1, scale, softcap, window, prefix=pre)
    if out is not None:
        out.copy_(o.view_as(out))
        return out
    return o


def geglu(gu, out=None):
    if gu.is_cuda:
        out = _out(out, gu.shape[:-1] + (gu.shape[-1] // 2,), gu.dtype, gu.device)
        _k().geglu(gu, out)
        return out
    y = ref.geglu(gu)
    if out is not None:
        out.copy_(y)
        return out
    return y


def argmax_rows(logits, cap=0.0, out=None):
    if logits.is_cuda:
        _softcap_table(cap, logits.device)
        out = _out(out, logits.shape[:-1], torch.int32, logits.device)
        _k().argmax_rows(logits, out, float(cap))
        return out
    y = ref.argmax_rows(logits, cap)
    if out is not None:
        out.copy_(y.view_as(out))
        return out
    return y


def row_lse(logits, cap=0.0, emulate_bf16=False, out=None):
    if logits.is_cuda:
        if emulate_bf16:
            _softcap_table(cap, logits.device)
        out = _out(out, logits.shape[:-1], torch.float32, logits.device)
        _k().row_lse(logits, out, float(cap), bool(emulate_bf16))
        return out
    y = ref.row_lse(logits, cap, emulate_bf16)
    if out is not None:
        out.copy_(y.view_as(out))
        return out
    return y


def _rows_of(logits, lse, rowmap):
    """CPU path of a ``rowmap``: materialise the logical rows."""
    V = logits.shape[-1]
    r = rowmap.view(-1).long()
    return logits.reshape(-1, V).index_select(0, r), lse.reshape(-1).index_select(0, r)


def gather_probs(logits, lse, ids, round_bf16=False, out=None, rowmap=None):
    """``p[r, k] = softmax(logits[row r])[ids[r, k]]``; ``rowmap [R]``: logical row ``r`` is logits row
    ``rowmap[r]`` (deduplicated rows)."""
    if logits.is_cuda:
        out = _out(out, ids.shape, torch.float32, logits.device)
        _k().gather_probs(logits, lse, ids, out, bool(round_bf16), rowmap)
        return out
    if rowmap is not None:
        logits, lse = _rows_of(logits, lse, rowmap)
    y = ref.gather_probs(logits, lse, ids, round_bf16).view(ids.shape)
    if out is not None:
        out.copy_(y)
        return out
    return y


def lens_colsum(logits, lse, mask, excl, B, T, acc=None, accumulate=False, round_bf16=False, offs=None, cum=None,
                rowmap=None):
    """Per-sequence sum over rows of ``softmax(logits)`` with 2 excluded ids per row.

    Dense layout: rows ``[B*T]`` with ``mask``; packed: ``offs [B+1]`` row offsets (``mask`` None, ``T``
    unused).  ``cum [B, T+1, V]`` (dense only) also receives the running sum after every row.
    ``rowmap [R]`` (packed only): logical row ``r`` (its exclusions, its place in ``offs``) reads logits row
    ``rowmap[r]`` — identical rows evaluated once."""
    V = logits.shape[-1]
    if logits.is_cuda:
        if acc is None:
            acc = torch.zeros(B, V, dtype=torch.float32, device=logits.device)
            accumulate = False
        _k().lens_colsum(logits, lse, mask, excl, acc, int(B), int(T), bool(accumulate), bool(round_bf16),
                         offs, cum, rowmap)
        return acc
    if rowmap is not None:
        logits, lse = _rows_of(logits, lse, rowmap)
    res = ref.lens_colsum(logits, lse, mask, excl, B, T, None, round_bf16, offs=offs, with_cum=cum is not None)
    s, c = res if isinstance(res, tuple) else (res, None)
    if acc is None:
        acc = s
    elif accumulate:
        if c is not None:
            c.add_(acc.view(B, 1, V))
        acc.add_(s)
    else:
        acc.copy_(s)
    if cum is not None:
        cum.copy_(c)
    return acc


def topk_rows(x, k) -> Tuple[torch.Tensor, torch.Tensor]:
    if x.is_cuda and k <= 64:
        R = x.numel() // x.shape[-1]
        vals = torch.empty(R, k, dtype=torch.float32, device=x.device)
        idx = torch.empty(R, k, dtype=torch.int32, device=x.device)
        _k().topk_rows(x.float().contiguous(), vals, idx, int(k))
        return vals, idx
    return ref.topk_rows(x.float(), k)


def xent_rows(logits, tgt, cap=0.0, emulate_bf16=True, out=None):
    if logits.is_cuda:
        if emulate_bf16:
            _softcap_table(cap, logits.device)
        out = _out(out, tgt.shape, torch.float32, logits.device)
        _k().xent_rows(logits, tgt, out, float(cap), bool(emulate_bf16))
        return out
    y = ref.xent_rows(logits, tgt, cap, emulate_bf16).view(tgt.shape)
    if out is not None:
        out.copy_(y)
        return out
    return y


# fused GEMM head (gemm4 G4_HEAD): opt-in; the in-tree logits GEMM + decode_head measured faster (round 2: 0.4-1.7 %,
# profiles/r2/head_ab/; round 5 in tb mode: 0.94-0.99x, profiles/r5/head_bench_tb.log); TB_FUSED_HEAD=1 / --fused-head
FUSED_HEAD = os.environ.get("TB_FUSED_HEAD", "0") == "1"


def head_part_numel(rows: int, vocab: int) -> int:
    """fp32 elements of the fused head's partial workspace for ``rows`` rows (16 B per 128 vocab columns)."""
    return rows * (vocab // 128) * 4


def vocab_head(x, w, cap, tgt=None, nxt=None, nll_self=None, nll_tgt=None, part=None, tgt_logit=None,
               fused: Optional[bool] = None):
    """``decode_head(x @ w^T, ...)`` from the final-normed rows ``x``: greedy token (bf16-softcap argmax), its
    NLL and the optional teacher target's NLL.  GPU with ``fused`` (default ``TB_FUSED_HEAD``): one
    four-wave MFMA GEMM (csrc/gemm4.hip G4_HEAD) whose epilogue applies the exact bf16 softcap table and reduces each row's 128-column
    slices to {max, sum exp, first argmax} (+ the target logit), then a merge kernel — the [rows, V] logits
    never reach HBM (``part``: optional fp32 workspace of ``head_part_numel`` elements, e.g. an idle logits
    buffer).  Otherwise the unembedding GEMM + ``decode_head``.  Returns ``(nxt, nll_self, nll_tgt)``."""
    K = x.shape[-1]
    R = x.numel() // K
    V = w.shape[0]
    fused = FUSED_HEAD if fused is None else fused
    if x.is_cuda and fused and _k().gemm4_ok(R, V, K) and x.is_contiguous():
        dev = x.device
        _softcap_table(cap, dev)
        nxt = _out(nxt, (R,), torch.int32, dev)
        nll_self = _out(nll_self, (R,), torch.float32, dev)
        need = head_part_numel(R, V)
        part = torch.empty(need, dtype=torch.float32, device=dev) if part is None else part.view(-1)[:need]
        if tgt is not None:
            nll_tgt = _out(nll_tgt, (R,), torch.float32, dev)
            tgt_logit = _out(tgt_logit, (R,), torch.float32, dev)
            _k().head_fused(x, w, part, float(cap), tgt, tgt_logit, nxt, nll_self, nll_tgt)
        else:
            _k().head_fused(x, w, part, float(cap), None, None, nxt, nll_self, None)
        return nxt, nll_self, nll_tgt
    return decode_head(linear(x, w), cap, tgt, nxt, nll_self, nll_tgt)


FUSED_LENS = os.environ.get("TB_FUSED_LENS", "1") == "1"   # gemm4 G4_LENS (round 4); 0: GEMM dispatch + row_lse
def lens_unembed(xn, w, fused: Optional[bool] = None, out=None, lse_out=None):
    """Logit-lens unembedding of final-normed rows: ``(logits = xn @ w^T (bf16), lse = logsumexp(logits))``, no
    softcap.  GPU with ``fused`` (default ``TB_FUSED_LENS``, off under ``TB_GEMM=blas``): one four-wave MFMA GEMM
    (csrc/gemm4.hip G4_LENS) that stores the bf16 logits and reduces each row's 128-column slices to {max, sum exp}
    in its epilogue, then the partial merge (tb_head_merge) -- no separate ``row_lse`` pass over the logits.
    Otherwise ``linear`` (the GEMM dispatch: hipBLASLt under ``blas``) + ``row_lse``."""
    K = xn.shape[-1]
    R = xn.numel() // K
    V = w.shape[0]
    fused = (FUSED_LENS and _GD.mode() != "blas") if fused is None else fused
    if xn.is_cuda and fused and _k().gemm4_ok(R, V, K) and xn.is_contiguous():
        logits = _out(out, xn.shape[:-1] + (V,), BF16, xn.device)
        part = _workspace("lens", head_part_numel(R, V), xn.device)
        lse = _out(lse_out, xn.shape[:-1], torch.float32, xn.device)
        _k().lens_gemm(xn, w, logits, part, lse)
        return logits, lse
    logits = linear(xn, w, out=out)
    return logits, row_lse(logits)


def decode_head(logits, cap, tgt=None, nxt=None, nll_self=None, nll_tgt=None):
    """One pass over decode logits: greedy token (bf16-softcap argmax), its NLL, and the NLL of an
    optional teacher target per row (``tgt < 0`` -> 0).  Returns ``(nxt, nll_self, nll_tgt)``."""
    R = logits.numel() // logits.shape[-1]
    dev = logits.device
    nxt = _out(nxt, (R,), torch.int32, dev)
    nll_self = _out(nll_self, (R,), torch.float32, dev)
    if tgt is not None:
        nll_tgt = _out(nll_tgt, (R,), torch.float32, dev)
    if logits.is_cuda:
        _softcap_table(cap, logits.device)
        _k().decode_head(logits, tgt, nxt, nll_self, nll_tgt if tgt is not None else None, float(cap))
        return nxt, nll_self, nll_tgt
    nxt.copy_(ref.argmax_rows(logits, cap).view(R))
    nll_self.copy_(ref.xent_rows(logits, nxt, cap, True).view(R))
    if tgt is not None:
        nll_tgt.copy_(ref.xent_rows(logits, tgt, cap, True).view(R))
    return nxt, nll_self, nll_tgt


HEAD_TRACK_MAX = 8      # tracked columns of decode_head_track (csrc/lens.hip DH_TRACK_MAX)


def decode_head_track(logits, cap, track, n_rank, tgt=None, nxt=None, nll_self=None, nll_tgt=None, logp=None,
                      rank=None, col=None):
    """:func:`decode_head` plus the output-side readout of the tracked vocab ids ``track [R, T]`` (int32,
    ``1 <= T <= 8``, ``-1`` = empty column) in the same pass over the logits: ``logp[r, k]`` = the model's
    next-token log-probability of ``track[r, k]`` (capped logit - the row's log-sum-exp; 0 for an empty column) and,
    for the first ``n_rank`` columns, ``rank[r, k]`` = the number of vocab entries with a strictly greater capped
    logit (-1 for an empty or unranked column).  ``logp`` / ``rank`` are ``[R, T]``; with ``col [R]`` (int64) they
    are ``[R, W, T]`` buffers and row ``r`` writes column ``min(col[r], W - 1)`` only.  The GPU path is one HIP kernel
    (csrc/lens.hip decode_head_track_kernel) and exists for the default head kernel only (``0 < cap <= 40``,
    ``TB_DECODE_HEAD`` unset or ``f``); anything else raises.  Returns ``(nxt, nll_self, nll_tgt, logp, rank)``."""
    V = logits.shape[-1]
    R = logits.numel() // V
    dev = logits.device
    if track.dim() != 2 or track.shape[0] != R:
        raise ValueError(f"decode_head_track: track must be [R={R}, T], got {tuple(track.shape)}")
    T = track.shape[1]
    if not 1 <= T <= HEAD_TRACK_MAX:
        raise ValueError(f"decode_head_track: 1 <= T <= {HEAD_TRACK_MAX} tracked columns, got {T}")
    if not 0 <= int(n_rank) <= T:
        raise ValueError(f"decode_head_track: n_rank must lie in [0, {T}], got {n_rank}")
    if logits.is_cuda and not cap > 0:
        raise ValueError(f"decode_head_track needs a final softcap on the GPU (0 < cap <= 40), got {cap}")
    nxt = _out(nxt, (R,), torch.int32, dev)
    nll_self = _out(nll_self, (R,), torch.float32, dev)
    if tgt is not None:
        nll_tgt = _out(nll_tgt, (R,), torch.float32, dev)
    if col is None:
        logp = _out(logp, (R, T), torch.float32, dev)
        rank = _out(rank, (R, T), torch.int32, dev)
    elif logp is None or rank is None or logp.dim() != 3 or logp.shape != rank.shape or logp.shape[2] != T:
        raise ValueError("decode_head_track: col needs logp / rank buffers of shape [R, W, T]")
    if logits.is_cuda:
        _softcap_table(cap, dev)
        _k().decode_head_track(logits, tgt, nxt, nll_self, nll_tgt if tgt is not None else None, track, int(n_rank),
                               logp, rank, col, float(cap))
        return nxt, nll_self, nll_tgt, logp, rank
    decode_head(logits, cap, tgt, nxt, nll_self, nll_tgt)
    lp, rk = ref.head_track(logits, cap, track, int(n_rank))
    if col is None:
        logp.copy_(lp)
        rank.copy_(rk)
    else:
        ar = torch.arange(R, device=dev)
        c = col.reshape(-1).long().clamp(0, logp.shape[1] - 1)
        logp[ar, c] = lp
        rank[ar, c] = rk
    return nxt, nll_self, nll_tgt, logp, rank


def head_shift(logits, base, rowmap, cap, kl=None, kl_rev=None):
    """Output shift of edited logits rows against their baseline rows: for row ``r`` of ``logits [R, V]`` (bf16) and
    ``b = rowmap[r]`` (``[R]`` int32) into ``base [Rb, V]`` (bf16), ``kl[r] = KL(base || edit)`` and ``kl_rev[r] =
    KL(edit || base)`` between the next-token distributions of the two rows' capped logits (the bf16 final-softcap
    chain, the values :func:`decode_head` sees), fp32 and not clamped at zero.  ``rowmap[r]`` outside ``[0, Rb)``
    gives 0, 0; rows of identical bits give exactly 0, 0; a row's result does not depend on the other rows of the
    call.  The GPU path is one HIP kernel (csrc/lens.hip head_shift_kernel) and exists for the default head kernel
    only (``0 < cap <= 40``, ``TB_DECODE_HEAD`` unset or ``f``); anything else raises.  Returns ``(kl, kl_rev)``."""
    if logits.dim() != 2 or base.dim() != 2 or base.shape[1] != logits.shape[1]:
        raise ValueError(f"head_shift: logits [R, V] and base [Rb, V] must share V, got {tuple(logits.shape)} and "
                         f"{tuple(base.shape)}")
    R, V = logits.shape
    if V < 1:
        raise ValueError("head_shift: empty rows")
    if logits.dtype != BF16 or base.dtype != BF16:
        raise ValueError(f"head_shift: logits and base must be bf16, got {logits.dtype} and {base.dtype}")
    if rowmap.dtype != torch.int32 or rowmap.dim() != 1 or rowmap.shape[0] != R:
        raise ValueError(f"head_shift: rowmap must be [R={R}] int32, got {tuple(rowmap.shape)} {rowmap.dtype}")
    dev = logits.device
    if base.device != dev or rowmap.device != dev:
        raise ValueError("head_shift: logits, base and rowmap must be on one device")
    if logits.is_cuda and not 0 < cap <= 40:
        raise ValueError(f"head_shift needs a final softcap 0 < cap <= 40 on the GPU, got {cap}")
    for name, o in (("kl", kl), ("kl_rev", kl_rev)):
        if o is not None and (o.shape != (R,) or o.dtype != torch.float32 or o.device != dev):
            raise ValueError(f"head_shift: {name} must be [R={R}] float32 on the logits' device")
    kl = _out(kl, (R,), torch.float32, dev)
    kl_rev = _out(kl_rev, (R,), torch.float32, dev)
    if logits.is_cuda:
        _softcap_table(cap, dev)
        _k().head_shift(logits.contiguous(), base.contiguous(), rowmap, kl, kl_rev, float(cap))
        return kl, kl_rev
    a, b = ref.head_shift(logits, base, rowmap, cap)
    kl.copy_(a)
    kl_rev.copy_(b)
    return kl, kl_rev


HEAD_MOVERS_KMAX = 8    # list entries of head_movers (csrc/lens.hip HM_KMAX); its tracked ids: HEAD_TRACK_MAX


def head_movers(logits, base, rowmap, rows, cap, k, ids=None, tv=None, up_id=None, up_dp=None, dn_id=None, dn_dp=None,
                dp_track=None):
    """Output movers of edited logits rows: where the probability went.  For selected row ``i`` with ``r = rows[i]``
    (``[Rs]`` int32, into ``logits [R, V]`` bf16) and ``b = rowmap[r]`` (``[R]`` int32, the map :func:`head_shift`
    takes, into ``base [Rb, V]`` bf16), ``d = Q - P`` is the difference of the two next-token distributions of the
    rows' capped logits.  Returns ``(tv, up_id, up_dp, dn_id, dn_dp, dp_track)``: ``tv [Rs] = 1/2 sum |d|`` (the total
    variation), ``up_id / up_dp [Rs, k]`` the ``k`` columns with the largest ``d > 0`` (``d`` descending, id
    ascending), ``dn_id / dn_dp [Rs, k]`` the ``k`` with the smallest ``d < 0`` (``d`` ascending, id ascending; the
    negative value), unfilled slots ``-1`` / ``+0.0``, and ``dp_track [Rs, T] = d`` at ``ids [Rs, T]`` (int32, ``T <=
    8``; an id outside ``[0, V)`` gives 0; ``[Rs, 0]`` without ``ids``).  ``rows[i]`` outside ``[0, R)`` or
    ``rowmap[r]`` outside ``[0, Rb)`` gives 0, empty lists and zeros; so do rows of identical bits, exactly; a row's
    result does not depend on the other rows of the call, and a tracked id that is also listed carries the list's
    float.  ``1 <= k <= 8``.  The GPU path is one HIP kernel (csrc/lens.hip head_movers_kernel) and exists for the
    default head kernel only (``0 < cap <= 40``, ``TB_DECODE_HEAD`` unset or ``f``); anything else raises."""
    if logits.dim() != 2 or base.dim() != 2 or base.shape[1] != logits.shape[1]:
        raise ValueError(f"head_movers: logits [R, V] and base [Rb, V] must share V, got {tuple(logits.shape)} and "
                         f"{tuple(base.shape)}")
    R, V = logits.shape
    if V < 1:
        raise ValueError("head_movers: empty rows")
    if logits.dtype != BF16 or base.dtype != BF16:
        raise ValueError(f"head_movers: logits and base must be bf16, got {logits.dtype} and {base.dtype}")
    if rowmap.dtype != torch.int32 or rowmap.dim() != 1 or rowmap.shape[0] != R:
        raise ValueError(f"head_movers: rowmap must be [R={R}] int32, got {tuple(rowmap.shape)} {rowmap.dtype}")
    if rows.dtype != torch.int32 or rows.dim() != 1:
        raise ValueError(f"head_movers: rows must be [Rs] int32, got {tuple(rows.shape)} {rows.dtype}")
    Rs = rows.shape[0]
    k = int(k)
    if not 1 <= k <= HEAD_MOVERS_KMAX:
        raise ValueError(f"head_movers: 1 <= k <= {HEAD_MOVERS_KMAX} list entries, got {k}")
    T = 0
    if ids is not None:
        if ids.dtype != torch.int32 or ids.dim() != 2 or ids.shape[0] != Rs:
            raise ValueError(f"head_movers: ids must be [Rs={Rs}, T] int32, got {tuple(ids.shape)} {ids.dtype}")
        T = ids.shape[1]
        if T > HEAD_TRACK_MAX:
            raise ValueError(f"head_movers: T <= {HEAD_TRACK_MAX} tracked ids, got {T}")
    dev = logits.device
    if base.device != dev or rowmap.device != dev or rows.device != dev or (ids is not None and ids.device != dev):
        raise ValueError("head_movers: logits, base, rowmap, rows and ids must be on one device")
    if logits.is_cuda and not 0 < cap <= 40:
        raise ValueError(f"head_movers needs a final softcap 0 < cap <= 40 on the GPU, got {cap}")
    spec = (("tv", tv, (Rs,), torch.float32), ("up_id", up_id, (Rs, k), torch.int32),
            ("up_dp", up_dp, (Rs, k), torch.float32), ("dn_id", dn_id, (Rs, k), torch.int32),
            ("dn_dp", dn_dp, (Rs, k), torch.float32), ("dp_track", dp_track, (Rs, T), torch.float32))
    outs = []
    for name, o, shape, dt in spec:
        if o is not None and (tuple(o.shape) != shape or o.dtype != dt or o.device != dev or not o.is_contiguous()):
            raise ValueError(f"head_movers: {name} must be a contiguous {list(shape)} {dt} tensor on the logits' "
                             f"device")
        outs.append(o if o is not None else torch.empty(shape, dtype=dt, device=dev))
    if logits.is_cuda:
        _softcap_table(cap, dev)
        _k().head_movers(logits.contiguous(), base.contiguous(), rowmap, rows.contiguous(),
                         None if ids is None else ids.contiguous(), k, *outs, float(cap))
        return tuple(outs)
    for o, v in zip(outs, ref.head_movers(logits, base, rowmap, rows, cap, k, ids)):
        o.copy_(v)
    return tuple(outs)


def slot_copy(dst: torch.Tensor, src: torch.Tensor, dst_slots, src_slots, layers: Optional[range] = None,
              src_layers: Optional[range] = None) -> None:
    """``dst[l, dst_slots[i]] = src[l', src_slots[i]]`` for the layer ranges ``layers`` (of dst) and ``src_layers``
    (of src, default the same) of two ``[L, slots, ...]`` bf16 tensors (KV caches): one pass on the GPU
    (``csrc/elementwise.hip`` slot_copy), no temporary.  Slot lists are host sequences (checked here)."""
    ds, ss = [int(v) for v in dst_slots], [int(v) for v in src_slots]
    assert len(ds) == len(ss)
    if not ds:
        return
    layers = range(dst.shape[0]) if layers is None else layers
    src_layers = layers if src_layers is None else src_layers
    assert len(layers) == len(src_layers) and layers.step == 1 and src_layers.step == 1
    if not len(layers):
        return
    assert 0 <= min(ds) and max(ds) < dst.shape[1] and 0 <= min(ss) and max(ss) < src.shape[1], "slot out of range"
    if dst.is_cuda and dst.dtype == BF16 and src.dtype == BF16 and dst.is_contiguous() and src.is_contiguous():
        dt = torch.tensor(ds, dtype=torch.int32).pin_memory().to(dst.device, non_blocking=True)
        st = torch.tensor(ss, dtype=torch.int32).pin_memory().to(dst.device, non_blocking=True)
        _k().slot_copy(dst, src, dt, st, int(layers.start), int(src_layers.start), len(layers))
        return
    d = torch.tensor(ds, device=dst.device)
    s_ = torch.tensor(ss, device=dst.device)
    dst[layers.start:layers.stop].index_copy_(1, d, src[src_layers.start:src_layers.stop].index_select(1, s_))


# ------------------------------------------------------------------ vocab-parallel merges (csrc/vp.hip)
def decode_head_stats(logits, tgt, off: int, cap: float, out=None):
    """Vocab-parallel head, this rank's columns ``logits [R, V_local]`` (vocab ids ``off ..``): per row
    ``{log-sum-exp, best capped logit, its global id, teacher target's capped logit or -inf}`` as ``[R, 4]`` fp32 from
    one HIP pass (csrc/lens.hip decode_head_f_kernel, stats mode) -- the input of :func:`vp_head_merge` after the
    group's all-gather.  None off the GPU or for a cap without a registered table (callers use the PyTorch path)."""
    if not logits.is_cuda or not (cap > 0):
        return None
    _softcap_table(cap, logits.device)
    R = logits.numel() // logits.shape[-1]
    out = _out(out, (R, 4), torch.float32, logits.device)
    if not _k().decode_head_stats(logits, tgt, int(off), out, float(cap)):
        return None
    return out


def vp_head_merge(st, tgt, V: int, nxt=None, nll_self=None, nll_tgt=None):
    """Merge the per-rank head stats ``st [tp, R, 4]`` = {log-sum-exp, best capped logit, its global index,
    target logit (-inf off the rank's slice)} in rank order: greedy token, its NLL and the teacher target's NLL
    (0 for targets outside ``[0, V)``), identical to :func:`decode_head` on the full row."""
    tp, R = st.shape[0], st.shape[1]
    dev = st.device
    nxt = _out(nxt, (R,), torch.int32, dev)
    nll_self = _out(nll_self, (R,), torch.float32, dev)
    if tgt is not None:
        nll_tgt = _out(nll_tgt, (R,), torch.float32, dev)
    if st.is_cuda:
        _k().vp_head_merge(st.contiguous(), tgt, int(V), nxt, nll_self, nll_tgt if tgt is not None else None)
        return nxt, nll_self, nll_tgt
    a, b, c = ref.vp_head_merge(st, tgt, V)
    nxt.copy_(a)
    nll_self.copy_(b)
    if tgt is not None:
        nll_tgt.copy_(c)
    return nxt, nll_self, nll_tgt


def vp_lse_merge(lse_parts: torch.Tensor, out=None) -> torch.Tensor:
    """``[tp, R]`` per-rank log-sum-exps of disjoint vocab slices -> ``[R]`` log-sum-exp of the whole row."""
    R = lse_parts.shape[1]
    out = _out(out, (R,), torch.float32, lse_parts.device)
    if lse_parts.is_cuda:
        _k().vp_lse_merge(lse_parts.float().contiguous(), out)
        return out
    out.copy_(ref.vp_lse_merge(lse_parts))
    return out


def vp_topk_merge(vals: torch.Tensor, ids: torch.Tensor):
    """Per-rank top-k candidates ``[tp, n, k]`` (values, GLOBAL ids) -> the global top-k ``[n, k]``, descending,
    ties to the lower id (the order of :func:`topk_rows` on the full row)."""
    tp, n, k = vals.shape
    if vals.is_cuda and k <= 64:
        ov = torch.empty(n, k, dtype=torch.float32, device=vals.device)
        oi = torch.empty(n, k, dtype=torch.int32, device=vals.device)
        _k().vp_topk_merge(vals.float().contiguous(), ids.to(torch.int32).contiguous(), ov, oi)
        return ov, oi
    return ref.vp_topk_merge(vals, ids)


reference_geglu = ref.geglu


def lowrank_edit(h, apply, idx, cnt, E, Dm, bias=None, thr=None, pre_bias=None, alpha=1.0, w_next=None, eps=1e-6,
                 x_next=None, coef_out=None):
    """Per flagged row: h -= sum_j f(<h - pre_bias, E_j> + bias_j) * alpha * Dm_j; refresh x_next = norm(h)."""
    if h.is_cuda:
        _k().lowrank_edit(h, x_next, apply, idx, cnt, E, Dm, bias, thr, pre_bias, float(alpha), w_next, float(eps),
                          coef_out)
        return h
    ref.lowrank_edit(h, apply, idx, cnt, E, Dm, bias, thr, pre_bias, alpha, w_next, eps, x_next, coef_out)
    return h


def latent_affine_edit(h, apply, idx, cnt, val, E, Dm, bias=None, thr=None, pre_bias=None, alpha=1.0, w_next=None,
                       eps=1e-6, x_next=None, coef_out=None):
    """Latent clamping / steering, in place: per flagged row ``h <- bf16(h + sum_j delta_j Dm[idx_j])`` with
    ``delta_j = val[row, j] - alpha * a_j`` and ``a_j = f(<h - pre_bias, E[idx_j]> + bias)`` as in
    :func:`lowrank_edit` (``val [rows, mmax]`` fp32, aligned with ``idx``), then ``x_next = RMSNorm(h, w_next)``.
    ``alpha = 1`` holds latent ``j`` at ``val_j`` whether or not it fires, ``alpha = 0`` adds ``val_j`` of it.  The
    terms are added in slot order in fp32, so a row's bits do not depend on its batch; a row whose deltas are all
    zero keeps ``h`` and ``x_next`` bit for bit; ``val == 0`` gives :func:`lowrank_edit`'s bits (the same device
    code, csrc/sae.hip).  ``coef_out`` receives ``a_j``."""
    if h.is_cuda:
        _k().latent_affine_edit(h, x_next, apply, idx, cnt, val, E, Dm, bias, thr, pre_bias, float(alpha), w_next,
                                float(eps), coef_out)
        return h
    ref.latent_affine_edit(h, apply, idx, cnt, val, E, Dm, bias, thr, pre_bias, alpha, w_next, eps, x_next, coef_out)
    return h


def matched_noise_edit(h, apply, idx, cnt, E, Dm, seeds, pos, val=None, bias=None, thr=None, pre_bias=None, alpha=1.0,
                       w_next=None, eps=1e-6, x_next=None, coef_out=None, norm_out=None):
    """The norm-matched random-direction control of :func:`lowrank_edit` (``val`` None) and
    :func:`latent_affine_edit` (``val [rows, mmax]`` fp32), in place: a flagged row that the targeted edit would move
    by ``delta = sum_j c_j Dm[idx_j]`` (their coefficients, the same device code) moves by ``n = |delta|_2`` along
    ``z / |z|_2`` instead, ``z_d = rb_gauss(seeds[row], pos[row], d)`` (``seeds [rows]`` int64, ``pos [rows]`` int32):
    ``h <- bf16(h + n z / |z|)``, then ``x_next = RMSNorm(h, w_next)``.  A row whose coefficients are all zero (or
    whose ``delta`` is) keeps ``h`` and ``x_next`` bit for bit.  A row's bits depend on its own inputs only.
    ``coef_out`` receives ``a_j``, ``norm_out [rows]`` fp32 receives ``n`` (0 on every untouched row)."""
    if h.is_cuda:
        _k().matched_noise_edit(h, x_next, apply, idx, cnt, E, Dm, seeds, pos, val, bias, thr, pre_bias, float(alpha),
                                w_next, float(eps), coef_out, norm_out)
        return h
    ref.matched_noise_edit(h, apply, idx, cnt, E, Dm, seeds, pos, val, bias, thr, pre_bias, alpha, w_next, eps, x_next,
                           coef_out, norm_out)
    return h


def interchange_edit(h, apply, idx, cnt, E, Dm, donor, src, bias=None, thr=None, pre_bias=None, alpha=1.0, w_next=None,
                     eps=1e-6, x_next=None, coef_out=None, dcoef_out=None):
    """Interchange (donor-swap) intervention, in place: per flagged row with donor row ``d = donor[src[row]]``
    (``donor [R, D]`` like ``h``, ``src [rows]`` int32), ``h <- bf16(h - sum_j c_j Dm[idx_j])`` with ``c_j =
    fl32(alpha * a_j(h)) - fl32(alpha * a_j(d))`` and ``a_j`` as in :func:`lowrank_edit`, then ``x_next = RMSNorm(h,
    w_next)``: the selected latents (SAE tables) or subspace coordinates (``E = Dm = U``: ``h + alpha U^T U (d - h)``)
    take the donor's values and everything else stays.  A row whose ``src`` is outside ``[0, R)`` and a row whose
    ``c_j`` are all zero (its own donor, say) keep ``h`` and ``x_next`` bit for bit; a donor on which every selected
    ``a_j`` is zero gives :func:`lowrank_edit`'s bits, and any donor gives :func:`latent_affine_edit`'s with ``val =
    alpha * a(d)`` (the same device code, csrc/sae.hip).  The terms are added in slot order in fp32, so a row's bits
    do not depend on its batch.  ``coef_out`` receives ``a_j(h)``, ``dcoef_out`` ``a_j(d)``."""
    if h.is_cuda:
        _k().interchange_edit(h, x_next, apply, idx, cnt, E, Dm, donor, src, bias, thr, pre_bias, float(alpha), w_next,
                              float(eps), coef_out, dcoef_out)
        return h
    ref.interchange_edit(h, apply, idx, cnt, E, Dm, donor, src, bias, thr, pre_bias, alpha, w_next, eps, x_next,
                         coef_out, dcoef_out)
    return h


def sae_splice_edit(h, apply, acts, idx, cnt, Wdec, b_dec=None, alpha=1.0, w_next=None, eps=1e-6, x_next=None,
                    src_row=None):
    """Reconstruct-mode SAE ablation, in place: per flagged row ``h <- bf16(b_dec + sum_{a_j != 0, ascending j}
    s_j a_j Wdec[j])`` with ``a = acts[src_row[row]]`` (``src_row`` None: ``acts[row]``), ``s_j = 1 - alpha`` for
    ``j`` in ``idx[row, :cnt[row]]`` and 1 elsewhere (fp32 accumulation in that order, so a row's bits do not
    depend on its batch), then ``x_next = RMSNorm(h, w_next)``.  ``cnt == 0`` is the pure splice; unflagged rows
    (and rows whose ``src_row`` is outside ``acts``) keep ``h`` and ``x_next`` bit for bit."""
    if h.is_cuda:
        _k().sae_splice_edit(h, x_next, apply, src_row, acts, idx, cnt, Wdec, b_dec, float(alpha), w_next, float(eps))
        return h
    ref.sae_splice_edit(h, apply, acts, idx, cnt, Wdec, b_dec, alpha, w_next, eps, x_next, src_row)
    return h


def flag_compact(flags, cap: int, rows=None, inv=None):
    """``rows [cap]`` int32: the indices of the set entries of ``flags [n]`` (uint8), ascending, unused entries -1;
    ``inv [n]`` int32 (optional output): each row's place in the list, -1 if unflagged.  Static shapes and no host
    sync, so a hook inside a captured graph can encode only its flagged rows; ``cap`` must bound the flag count
    (flags past it are dropped, ``inv`` -1).  Returns ``rows``."""
    rows = _out(rows, (int(cap),), torch.int32, flags.device)
    if flags.is_cuda:
        _k().flag_compact(flags, rows, inv)
        return rows
    ref.flag_compact(flags, rows, inv)
    return rows


def sae_decode_sparse(acts, Wdec, b_dec=None, out_bf16=None, out_f32=None):
    if acts.is_cuda:
        M = acts.numel() // Wdec.shape[0]
        if out_bf16 is None and out_f32 is None:
            out_f32 = torch.empty(M, Wdec.shape[1], dtype=torch.float32, device=acts.device)
        _k().sae_decode_sparse(acts, Wdec, b_dec, out_bf16, out_f32)
        return out_f32 if out_f32 is not None else out_bf16
    y = ref.sae_decode_sparse(acts, Wdec, b_dec)
    if out_f32 is not None:
        out_f32.copy_(y)
        return out_f32
    if out_bf16 is not None:
        out_bf16.copy_(y.to(BF16))
        return out_bf16
    return y


def latent_score(acts, p, spike, seg):
    """Returns (score, spike_mean, corr), each [G, L]."""
    if acts.is_cuda:
        G = seg.numel() - 1
        L = acts.shape[-1]
        out = torch.empty(G, L, dtype=torch.float32, device=acts.device)
        sm = torch.empty_like(out)
        cr = torch.empty_like(out)
        _k().latent_score(acts, p, spike, seg, out, sm, cr)
        return out, sm, cr
    return ref.latent_score(acts, p, spike, seg)


def latent_effect(acts, X, V, Wdec, seg, alpha, eps, cap, mode, want_eff=False):
    """Causal latent scores at the spike rows (csrc/latent_effect.hip).  ``acts [R, L]`` fp32, ``X [R, D]`` bf16
    residuals, ``V [1 | R, D]`` fp32, ``Wdec [L, D]`` fp32 or bf16, ``seg [G + 1]`` int32 (ascending, 0 .. R).
    Per row and latent with ``a > 0`` and ``c = alpha a``: mode 0 the exact change of the softcapped readout
    ``f((x . v) / rms(x))`` when ``x`` becomes ``x - c W_dec[j]``; mode 1 ``c (v . W_dec[j])``; 0.0 where ``a <= 0``.
    Returns ``score [G, L]`` (segment means) or ``(score, eff [R, L])`` with ``want_eff``, fp32."""
    if acts.is_cuda:
        R, L = acts.shape
        score = torch.empty(seg.numel() - 1, L, dtype=torch.float32, device=acts.device)
        eff = torch.empty(R, L, dtype=torch.float32, device=acts.device) if want_eff else None
        _k().latent_effect(acts, X, V, Wdec, seg, score, eff, float(alpha), float(eps), float(cap), int(mode))
        return (score, eff) if want_eff else score
    score, eff = ref.latent_effect(acts, X, V, Wdec, seg, alpha, eps, cap, int(mode))
    return (score.float(), eff.float()) if want_eff else score.float()


LENS_TRACK_MAX = 8      # tracked columns of lens_track (csrc/lens_track.hip: one kernel instance per T)


def lens_track(h, V, vrow, eps, cap, out=None):
    """Tracked-token lens logits of residual rows (csrc/lens_track.hip): ``out[r, t] = f((h_r . V[vrow[r], t]) /
    sqrt(|h_r|^2 / D + eps))`` for ``h [M, D]`` bf16, a table ``V [U, T, D]`` fp32 of lens directions
    (``interp/gradient.py::lens_direction``), a row map ``vrow [M]`` int32 and ``f`` the softcap ``cap tanh(. / cap)``
    (``cap <= 0``: identity).  A row with ``vrow[r]`` outside ``[0, U)`` gets 0.0 in all ``T`` columns and reads no
    table row; an all-zero table row gives exactly 0.0.  A row's bits depend on that row and its table block alone
    (not on ``M``, its place in the call or the other rows' ``vrow``).  ``D % 8 == 0``, ``D <= 4096``,
    ``1 <= T <= 8``; anything else raises ``ValueError``.  Returns ``out [M, T]`` fp32."""
    if h.dim() != 2 or V.dim() != 3 or V.shape[2] != h.shape[1]:
        raise ValueError(f"lens_track: h [M, D] and V [U, T, D] must share D, got {tuple(h.shape)} and {tuple(V.shape)}")
    M, D = h.shape
    U, T = V.shape[0], V.shape[1]
    if D % 8 != 0 or not 8 <= D <= 4096:
        raise ValueError(f"lens_track: D must be a multiple of 8 and at most 4096, not {D}")
    if not 1 <= T <= LENS_TRACK_MAX:
        raise ValueError(f"lens_track: 1 <= T <= {LENS_TRACK_MAX} tracked columns, not {T}")
    if h.dtype != BF16 or V.dtype != torch.float32:
        raise ValueError(f"lens_track: h must be bf16 and V float32, got {h.dtype} and {V.dtype}")
    if vrow.dtype != torch.int32 or vrow.dim() != 1 or vrow.shape[0] != M:
        raise ValueError(f"lens_track: vrow must be [M={M}] int32, got {tuple(vrow.shape)} {vrow.dtype}")
    dev = h.device
    if V.device != dev or vrow.device != dev:
        raise ValueError("lens_track: h, V and vrow must be on one device")
    if out is not None and (out.shape != (M, T) or out.dtype != torch.float32 or out.device != dev
                            or not out.is_contiguous()):
        raise ValueError(f"lens_track: out must be a contiguous [M={M}, T={T}] float32 on h's device")
    out = _out(out, (M, T), torch.float32, dev)
    if M == 0:
        return out
    if h.is_cuda:
        _k().lens_track(h.contiguous(), V.contiguous(), vrow.contiguous(), out, float(eps), float(cap))
        return out
    out.copy_(ref.lens_track(h, V, vrow, eps, cap))
    return out


SEG_DOTS_MAX_T, SEG_DOTS_MAX_S, SEG_DOTS_MAX_K = 4, 64, 4096     # csrc/comp_trace.hip


def seg_dots_check(K, S, T, Dn=None, what="seg_dots"):
    """Raise ``ValueError`` unless ``(K, S, T, Dn)`` is inside the kernel's range (csrc/comp_trace.hip)."""
    if not 1 <= T <= SEG_DOTS_MAX_T:
        raise ValueError(f"{what}: 1 <= T <= {SEG_DOTS_MAX_T} table columns, not {T}")
    if not 1 <= S <= SEG_DOTS_MAX_S:
        raise ValueError(f"{what}: 1 <= S <= {SEG_DOTS_MAX_S} segments, not {S}")
    if K % 8 != 0 or not 8 <= K <= SEG_DOTS_MAX_K or K % S != 0 or (K // S) % 8 != 0:
        raise ValueError(f"{what}: K and K / S must be multiples of 8 and K at most {SEG_DOTS_MAX_K}, not K = {K}, "
                         f"S = {S}")
    if Dn is not None and (Dn % 8 != 0 or not 8 <= Dn <= SEG_DOTS_MAX_K):
        raise ValueError(f"{what}: Dn must be a multiple of 8 and at most {SEG_DOTS_MAX_K}, not {Dn}")


def seg_dots(X, W, rows, blk, S, R, eps, out=None, rms=None):
    """Segment-wise dot products of selected rows over the rows' RMS (csrc/comp_trace.hip): ``out[i, t, s] =
    (sum_{k in segment s} X[rows[i], k] W[blk[i], t, k]) / rho_i`` with ``rho_i = sqrt(|R[rows[i]]|^2 / Dn + eps)``
    (``R = None``: 1) and ``rms[i] = rho_i``, for ``X [M, K]`` bf16, a table ``W [U, T, K]`` fp32, ``rows [Ms]`` and
    ``blk [Ms]`` int32, ``R [M, Dn]`` bf16; segment ``s`` is columns ``[s K / S, (s + 1) K / S)``.  A selected row
    with ``rows[i]`` outside ``[0, M)`` or ``blk[i]`` outside ``[0, U)`` gets +0.0 in every column and ``rms[i] =
    0.0`` and reads nothing; an all-zero table segment gives exactly +0.0.  A row's bits depend on that row, its table
    block and ``(K, S, T, Dn)`` alone.  ``1 <= T <= 4``, ``1 <= S <= 64``, ``K % 8 == 0``, ``(K / S) % 8 == 0``,
    ``K, Dn <= 4096``, ``Dn % 8 == 0``; anything else raises ``ValueError``.  Returns ``(out [Ms, T, S], rms [Ms])``
    fp32."""
    if X.dim() != 2 or W.dim() != 3 or W.shape[2] != X.shape[1]:
        raise ValueError(f"seg_dots: X [M, K] and W [U, T, K] must share K, got {tuple(X.shape)} and {tuple(W.shape)}")
    M, K = X.shape
    T = W.shape[1]
    S = int(S)
    if R is not None and (R.dim() != 2 or R.shape[0] != M):
        raise ValueError(f"seg_dots: R must be [M={M}, Dn], got {tuple(R.shape)}")
    seg_dots_check(K, S, T, None if R is None else R.shape[1])
    if X.dtype != BF16 or W.dtype != torch.float32 or (R is not None and R.dtype != BF16):
        raise ValueError(f"seg_dots: X and R must be bf16 and W float32, got {X.dtype}, "
                         f"{None if R is None else R.dtype} and {W.dtype}")
    if rows.dtype != torch.int32 or blk.dtype != torch.int32 or rows.dim() != 1 or blk.shape != rows.shape:
        raise ValueError(f"seg_dots: rows and blk must be [Ms] int32, got {tuple(rows.shape)} {rows.dtype} and "
                         f"{tuple(blk.shape)} {blk.dtype}")
    Ms = rows.shape[0]
    dev = X.device
    if any(t is not None and t.device != dev for t in (W, rows, blk, R)):
        raise ValueError("seg_dots: X, W, rows, blk and R must be on one device")
    for t, shape, name in ((out, (Ms, T, S), "out"), (rms, (Ms,), "rms")):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != dev
                              or not t.is_contiguous()):
            raise ValueError(f"seg_dots: {name} must be a contiguous {list(shape)} float32 on X's device")
    out = _out(out, (Ms, T, S), torch.float32, dev)
    rms = _out(rms, (Ms,), torch.float32, dev)
    if Ms == 0:
        return out, rms
    if X.is_cuda:
        _k().seg_dots(X.contiguous(), W.contiguous(), rows.contiguous(), blk.contiguous(), S,
                      None if R is None else R.contiguous(), out, rms, float(eps))
        return out, rms
    o, r = ref.seg_dots(X, W, rows, blk, S, R, eps)
    out.copy_(o)
    rms.copy_(r)
    return out, rms
