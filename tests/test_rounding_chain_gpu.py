"""The rounding chains of the small kernels, to the bf16 step (criteria and inputs: tests/rounding_cases.py, checked
against themselves in tests/test_rounding_chain_cpu.py): the RMSNorm family of csrc/norm.hip at every launch shape
against ops/reference.py, its width and weight guards, ``ops.geglu`` at every gate bit pattern, the fused GeGLU
epilogues of csrc/gemm4.hip and csrc/gemm_ring.hip against the unfused chain they claim to equal, and the RoPE /
KV-scatter kernels of csrc/rope.hip against ops/reference.py at three head geometries."""
import math

import pytest
import torch

import rounding_cases as rc
from taboo_brittleness_amd import ops
from taboo_brittleness_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _nan(shape, gpu):
    return torch.full(shape, float("nan"), dtype=BF, device=gpu)


# ---- A. norm family ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", rc.NORM_ROWS)
@pytest.mark.parametrize("D", rc.NORM_WIDTHS)
def test_norm_family_to_the_ulp(gpu, D, M):
    """rmsnorm, add_rmsnorm2 (h and x) and embed_rmsnorm (x) within one bf16 step of ops/reference.py with at most
    ``norm_budget`` elements unequal, at both ends of the one-slot and the four-slot launch.  add_rmsnorm2's h is the
    exact rounded sum of the old h and a post-norm within one step of the reference's (``check_residual``: where the
    sum cancels, one step of the post-norm is several of h); its x is compared with the reference norm of the GPU's
    own h, so a difference in h is not counted twice.  embed_rmsnorm's h is bit-equal (sqrt(3584) rounds to 59.75 in
    bf16; ids -5, V and V + 7 are clamped).  Seen on an MI355X: never more than one step, at most 17 of 1 212 416
    elements unequal (budget 1212) at D = 32768 and 3 of 303 104 below; h up to 8 steps from the reference's h
    (D = 8200), every one of them the exact sum for a post-norm one step off."""
    c = rc.norm_case(D, M)
    x, w, wn = c["x"].to(gpu), c["w"].to(gpu), c["wn"].to(gpu)
    y = ops.rmsnorm(x, w, rc.EPS, out=_nan((M, D), gpu))
    rc.check_norm(y.cpu(), c["y"], f"rmsnorm D {D} M {M}")
    h = c["h0"].to(gpu)
    xn = ops.add_rmsnorm2(h, x, w, wn, rc.EPS, out=_nan((M, D), gpu))
    h = h.cpu()
    rc.check_residual(h, c["h0"], c["y"], f"add_rmsnorm2 h D {D} M {M}")
    rc.check_norm(xn.cpu(), ref.rmsnorm(h, c["wn"], rc.EPS), f"add_rmsnorm2 x D {D} M {M}")
    e = rc.embed_case(D, M)
    he, xe = ops.embed_rmsnorm(e["ids"].to(gpu), e["E"].to(gpu), e["w"].to(gpu), math.sqrt(D), rc.EPS,
                               h_out=_nan((M, D), gpu), x_out=_nan((M, D), gpu))
    assert torch.equal(he.cpu(), e["h"])
    rc.check_norm(xe.cpu(), e["x"], f"embed_rmsnorm x D {D} M {M}")


@pytest.mark.parametrize("ks", [1, 4, 5])
def test_add_rmsnorm2_part_wide(gpu, ks):
    """add_rmsnorm2_part on the four-slot path (D = 8200) with random fp32 partials: h and x bit-equal to
    add_rmsnorm2 given o = bf16(partials added in split order from 0), computed on the CPU.  ks = 5 takes the
    four-at-a-time loop and the tail of sum_splits8."""
    D, M = 8200, 5
    g = torch.Generator().manual_seed(ks)
    part = torch.randn(ks, M, D, generator=g) * 2
    o = rc.sum_splits(part).to(gpu)
    h0 = torch.randn(M, D, generator=g).to(BF).to(gpu)
    wp = (torch.randn(D, generator=g) * 0.1).to(BF).to(gpu)
    wn = (torch.randn(D, generator=g) * 0.1).to(BF).to(gpu)
    k = ops._k()
    h1, x1 = h0.clone(), _nan((M, D), gpu)
    k.add_rmsnorm2(h1, o, wp, wn, x1, rc.EPS)
    h2, x2 = h0.clone(), _nan((M, D), gpu)
    k.add_rmsnorm2_part(h2, part.to(gpu), ks, wp, wn, x2, rc.EPS)
    assert not torch.equal(h1, h0)
    assert torch.equal(h1, h2) and torch.equal(x1, x2)
    assert not bool(torch.isnan(x2.float()).any())


# ---- B. guards --------------------------------------------------------------------------------------------------
def _norm_calls(gpu, D, M=2, short=None):
    """The four entries on sentinel-filled ``[M, D]`` tensors: ``(name, call, tensors that must keep the sentinel)``.
    ``short``: the name of one weight argument to pass as a ``D - 8`` view of a D-long buffer (so that even an
    unguarded kernel reads allocated memory only)."""
    k = ops._k()

    def t():
        return torch.full((M, D), 7.0, dtype=BF, device=gpu)

    def wt(name):
        buf = torch.zeros(D, dtype=BF, device=gpu)
        return buf[: D - 8] if name == short else buf

    x, y, h, o, xo = t(), t(), t(), t(), t()
    part = torch.ones(1, M, D, device=gpu)
    E = torch.zeros(4, D, dtype=BF, device=gpu)
    ids = torch.zeros(M, dtype=torch.int32, device=gpu)
    return [("rmsnorm", lambda: k.rmsnorm(x, wt("w"), y, rc.EPS), (y,)),
            ("add_rmsnorm2", lambda: k.add_rmsnorm2(h, o, wt("w_post"), wt("w_next"), xo, rc.EPS), (h, xo)),
            ("add_rmsnorm2_part", lambda: k.add_rmsnorm2_part(h, part, 1, wt("w_post"), wt("w_next"), xo, rc.EPS),
             (h, xo)),
            ("embed_rmsnorm", lambda: k.embed_rmsnorm(ids, E, wt("w"), h, xo, 1.0, rc.EPS), (h, xo))]


def test_norm_rejects_rows_past_the_widest_launch(gpu):
    """D = 32776 would need more than 1024 lanes of four 16-B slots: every entry of the family raises, names the
    limit, and leaves its outputs untouched (an unguarded launch is rejected by the runtime without a report)."""
    for name, call, outs in _norm_calls(gpu, rc.NORM_MAX_D + 8):
        with pytest.raises(RuntimeError, match=str(rc.NORM_MAX_D)):
            call()
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in outs), name


@pytest.mark.parametrize("short", ["w", "w_post", "w_next"])
def test_norm_rejects_short_weights(gpu, short):
    """A weight vector that is not D long is refused by every entry that takes it; the outputs keep their sentinel."""
    n = 0
    for name, call, outs in _norm_calls(gpu, 512, short=short):
        if (short == "w") != (name in ("rmsnorm", "embed_rmsnorm")):
            continue
        with pytest.raises(RuntimeError):
            call()
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in outs), name
        n += 1
    assert n == 2


def test_norm_accepts_the_widest_launch_unchanged(gpu):
    """The guarded entries still run at the limit itself (D = 32768) and with full-length weights."""
    for name, call, outs in _norm_calls(gpu, rc.NORM_MAX_D):
        call()
        torch.cuda.synchronize()
        assert not any(bool((o == 7.0).all()) for o in outs), name


# ---- C. GeGLU, exhaustive in the gate ---------------------------------------------------------------------------
def test_geglu_every_gate(gpu):
    """ops.geglu at all 65536 gate bit patterns against seven constant up values and a random one: inside the window
    of the stable-form GELU at every finite gate, ops/reference.py's NaN / inf pattern at the others.  Seen on an
    MI355X: all 310 832 outputs whose GELU and product are at least 2^-100 equal the correctly rounded fp64 result,
    so none of the window's second values was needed."""
    c = rc.geglu_case()
    out = ops.geglu(c["gu"].to(gpu), out=_nan((8, 65536), gpu))
    rc.check_geglu(out.cpu(), "ops.geglu")


# ---- D. fused GeGLU == the unfused chain ------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", rc.FUSED_SHAPES)
def test_fused_geglu_equals_unfused_chain(gpu, M, N, K):
    """gemm4 epilogue 3 (both tile heights), every ring tile and variant, and split-K epilogue 3 (three tile heights,
    heuristic and explicit split count) equal ``ops.geglu`` of the same GEMM's bf16 output bit for bit: a rounding
    missing on the gate or the up accumulator of an epilogue would show."""
    A, W = (t.to(gpu) for t in rc.fused_operands(M, N, K))
    F = N // 2
    Wi = W[ops.geglu_interleave_index(F, gpu)].contiguous()
    k = ops._k()
    c0 = _nan((M, N), gpu)
    k.gemm4(A, W, c0, None, None, 0, 256)
    want = ops.geglu(c0, out=_nan((M, F), gpu))
    gates = c0[:, :F].float()
    assert bool(((gates > -10) & (gates < -3)).any()) and float(gates.min()) < -20 and float(gates.max()) > 20
    for t in (256, 128):
        got = _nan((M, F), gpu)
        k.gemm4(A, Wi, got, None, None, 3, t)
        assert torch.equal(got, want), f"gemm4 tile {t}"
    n = 0
    for bm, bn in k.gemm_ring_tiles(3):
        for var in (0, 1, 2):
            if not k.gemm_ring_ok(M, N, K, 3, bm, bn, var):
                continue
            got = _nan((M, F), gpu)
            k.gemm_ring(A, Wi, got, 3, bm, bn, var)
            assert torch.equal(got, want), f"ring tile {bm}x{bn} variant {var}"
            n += 1
    assert n >= 1
    for t in (64, 128, 256):
        for ks in (int(k.gemm4_splitk_ks(M, N, K, t)), 4):
            ws = torch.full((ks * M * N,), float("nan"), device=gpu)
            s0 = _nan((M, N), gpu)
            k.gemm4_splitk(A, W, s0, ws, 0, t, ks)
            got = _nan((M, F), gpu)
            k.gemm4_splitk(A, Wi, got, ws, 3, t, ks)
            assert torch.equal(got, ops.geglu(s0)), f"split-K tile {t} ks {ks}"
            assert not bool(torch.isnan(got.float()).any())


# ---- E. RoPE and the cache scatter ------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv,HD", rc.ROPE_GEOMS)
def test_rope_and_cache_bit_equal(gpu, Hq, Hkv, HD):
    """rope_qkv_cache == ops/reference.py bit for bit (q, K cache, V cache) at head sizes 256, 128 and 16, with
    positions at both ends of the cache, past it, on and past the table's last row (clamped to it) and a padding
    row; caches and q pre-filled with random values, so an unwritten or over-written cell shows."""
    c = rc.rope_case(Hq, Hkv, HD)
    kc, vc, q = c["kc0"].to(gpu), c["vc0"].to(gpu), c["q0"].to(gpu)
    ops.rope_qkv_cache(c["qkv"].to(gpu), c["pos"].to(gpu), c["slot"].to(gpu), c["cos"].to(gpu), c["sin"].to(gpu), kc,
                       vc, Hq, Hkv, HD, q_out=q)
    assert torch.equal(q.cpu(), c["q"])
    assert torch.equal(kc.cpu(), c["kc"]) and torch.equal(vc.cpu(), c["vc"])
    assert not torch.equal(c["kc"], c["kc0"])


@pytest.mark.parametrize("ks", [1, 5])
def test_rope_part_bit_equal(gpu, ks):
    """rope_qkv_cache_part at the Gemma-2-2B head geometry (8 / 4 heads of 128) with random fp32 partials == the
    reference (and rope_qkv_cache on the GPU) on the bf16 of their ordered sum, same positions and pre-fill."""
    Hq, Hkv, HD = 8, 4, 128
    c = rc.rope_case(Hq, Hkv, HD)
    M, N = c["qkv"].shape
    g = torch.Generator().manual_seed(ks)
    part = torch.randn(ks, M, N, generator=g)
    qkv = rc.sum_splits(part)
    kcr, vcr = c["kc0"].clone(), c["vc0"].clone()
    qr = ref.rope_qkv_cache(qkv, c["pos"], c["slot"], c["cos"], c["sin"], kcr, vcr, Hq, Hkv, HD)
    pos, slot, cos_t, sin_t = (c[n].to(gpu) for n in ("pos", "slot", "cos", "sin"))
    k = ops._k()
    outs = []
    for fused in (False, True):
        kc, vc, q = c["kc0"].to(gpu), c["vc0"].to(gpu), c["q0"].to(gpu)
        if fused:
            k.rope_qkv_cache_part(part.to(gpu), ks, pos, slot, cos_t, sin_t, q, kc, vc, Hq, Hkv, HD)
        else:
            k.rope_qkv_cache(qkv.to(gpu), pos, slot, cos_t, sin_t, q, kc, vc, Hq, Hkv, HD)
        outs.append((q.cpu(), kc.cpu(), vc.cpu()))
    for a, b, r in zip(outs[0], outs[1], (qr, kcr, vcr)):
        assert torch.equal(a, b) and torch.equal(b, r)
