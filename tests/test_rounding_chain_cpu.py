"""The criteria of tests/test_rounding_chain_gpu.py, checked against themselves on the CPU (tests/rounding_cases.py):
the GELU window is tight and contains an fp32 emulation of the kernel's fast form, PyTorch's fp32 tanh form leaves it
exactly where ``1 + tanh`` cancels, and the norm budget separates legitimate fp32 differences from a misplaced bf16
rounding.  The last test turns every assertion of the GPU module against a deliberately wrong stand-in."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rounding_cases as rc
from taboo_brittleness_amd.ops import reference as ref

BF = torch.bfloat16


def test_bf16_ulps_and_rounding():
    """``bf16_ulps`` counts steps across zero, the sign, the binade and infinity; ``rn_bf16`` is PyTorch's own
    round-to-nearest-even on float32 inputs and rounds a float64 once (a value a cast through float32 would first
    round onto a tie, and then to the even side, stays on its own side)."""
    a = torch.tensor([0.0, -0.0, 1.0, 1.0, -1.0, 2.0 ** -133, float("inf"), float("nan"), float("nan")]).to(BF)
    b = torch.tensor([-0.0, 0.0, 1.0078125, 0.99609375, 1.0, -2.0 ** -133, 3.3895e38, float("nan"), 1.0]).to(BF)
    assert rc.bf16_ulps(a, b).tolist() == [0, 0, 1, 1, 2 * 0x3F80, 2, 1, 0, 1 << 16]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(200000, generator=g) * torch.exp(torch.randn(200000, generator=g) * 30)
    x = torch.cat([x, rc.all_bf16().float(), torch.tensor([3.39e38, -3.4e38, 1e-45, 4.6e-41])])
    got, want = rc.rn_bf16(x.double()), x.to(BF)
    assert torch.equal(torch.isnan(got.float()), torch.isnan(want.float()))
    assert int(rc.bf16_ulps(got, want).max()) == 0
    above = torch.tensor([1.00390625 + 2.0 ** -40, 1.01171875 - 2.0 ** -40], dtype=torch.float64)   # next to a tie
    assert rc.rn_bf16(above).float().tolist() == [1.0078125, 1.0078125]
    assert above.float().to(BF).float().tolist() == [1.0, 1.015625]                                   # rounded twice


def test_gelu_window_is_tight_and_pins_the_tanh_form():
    """Over all 65536 gate bit patterns: the window is one bf16 value for all but 2 % of the finite gates whose GELU
    is at least 2^-112 (measured: 265 of 45211, 0.59 %, never more than three values); PyTorch's fp32 ``0.5 x (1 +
    tanh(y))`` rounded to bf16 lies inside it at every finite gate outside [-10.5, -2.9] and leaves it at 147 gates
    inside (between -9.875 and -4.03125, by up to 13345 bf16 steps but at most 1.5e-7 in absolute value: ``1 +
    tanh(y)`` cancels there, the stable form the kernels use does not).  That is the one deliberate departure of
    csrc/common.h gelu_tanh_fast from the graph it mirrors; a change of either side moves the count."""
    g = rc.all_bf16()
    gf = g.float()
    fin = torch.isfinite(gf)
    lo, hi = rc.gelu_window(g)
    width = rc.bf16_ulps(lo, hi)
    assert bool((lo.float() <= hi.float())[fin].all())
    big = fin & (rc.gelu64(g.double()).abs() >= 2.0 ** -112)
    assert int(big.sum()) > 40000
    wide = int((width[big] != 0).sum())
    print(f"window wider than one value: {wide} of {int(big.sum())}, widest {int(width[big].max()) + 1} values")
    assert wide <= 0.02 * int(big.sum())
    assert int(width[big].max()) <= 2
    tanh = F.gelu(gf, approximate="tanh").to(BF)
    out = fin & ~rc.in_window(tanh, lo, hi)
    tail = (gf >= -10.5) & (gf <= -2.9)
    n = int((out & tail).sum())
    print(f"fp32 tanh form outside the window at {n} gates of [-10.5, -2.9]")
    assert int((out & ~tail).sum()) == 0
    assert 100 <= n <= 200
    assert n == 147, "the pinned count moved: PyTorch's tanh form or the window changed"
    assert float((tanh.double() - rc.gelu64(g.double())).abs()[out].max()) < 2e-7


def _fast_f32(x: np.ndarray, fma: bool) -> np.ndarray:
    """csrc/common.h gelu_tanh_fast in numpy float32, operation by operation: ``y = k0 (x + ((k1 x) x) x)``,
    ``__expf(a) = exp2(a log2 e)``, a reciprocal, a multiply; every intermediate rounded to float32 (the elementary
    functions correctly rounded, which the hardware's are to about an ulp).  ``fma``: with the compiler's
    contraction of ``x + c * x`` into one fused multiply-add."""
    f = np.float32
    k0, k1, l2e = f(0.7978845608028654), f(0.044715), f(1.4426950408889634)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        c = (k1 * x) * x
        inner = (c.astype(np.float64) * x + x).astype(f) if fma else x + c * x
        y = k0 * inner
        a = (f(-2.0) * y) * l2e
        e = np.exp2(a.astype(np.float64)).astype(f)
        r = (1.0 / (f(1.0) + e).astype(np.float64)).astype(f)
        return x * r


@pytest.mark.parametrize("fma", [False, True])
def test_fast_form_emulation_stays_inside_window(fma):
    """An fp32 emulation of gelu_tanh_fast, rounded to bf16, lies inside the window at every finite gate; so does
    the same emulation with its reciprocal flushed to zero where it is subnormal (v_rcp_f32's behaviour)."""
    g = rc.all_bf16()
    fin = torch.isfinite(g.float())
    lo, hi = rc.gelu_window(g)
    y = _fast_f32(g.float().numpy(), fma)
    got = torch.from_numpy(y).to(BF)
    assert bool(rc.in_window(got, lo, hi)[fin].all())
    flushed = torch.from_numpy(np.where(np.abs(y) < 2.0 ** -120, np.float32(0), y)).to(BF)
    assert bool(rc.in_window(flushed, lo, hi)[fin].all())
    # and the window is a real constraint: one bf16 step off the emulation is outside it almost everywhere
    big = fin & (got.float().abs() >= 2.0 ** -112)
    up = (got.view(torch.int16) + 1).view(BF)
    assert float((~rc.in_window(up, lo, hi))[big].float().mean()) > 0.97


def _rmsnorm_perturbed(x, w, eps, scale):
    """ops/reference.py rmsnorm with the mean of squares taken in float64 and the reciprocal root scaled."""
    xf = x.float()
    r = torch.rsqrt((xf.double().pow(2).mean(-1, keepdim=True)).float() + eps) * scale
    return (xf * r * (1.0 + w.float())).to(x.dtype)


def _add_rmsnorm2_unrounded(h, o, w_post, eps):
    """The residual of ops/reference.py add_rmsnorm2 with the rounding of the post-norm skipped: bf16(h + norm(o))
    instead of bf16(h + bf16(norm(o)))."""
    of = o.float()
    r = torch.rsqrt(of.pow(2).mean(-1, keepdim=True) + eps)
    return (h.float() + of * r * (1.0 + w_post.float())).to(h.dtype)


def test_norm_budget_separates_the_two_populations():
    """At the widths and row kinds of the GPU test (M = 37): a reference whose sum is taken in float64 and whose
    reciprocal root is 2 fp32 ulp off (1 +- 2.4e-7) differs from ops/reference.py by one bf16 step at most, in no
    more than a tenth of the budget at every width (measured: 0 to 63 elements per width, at most 0.82 of that tenth; 100
    of 2 056 016 elements over all widths at +, 92 at -: 0.005 %, a twentieth of the budget of 2056); the residual
    without the rounding of the post-norm exceeds 50 budgets over all widths and at every width of 512 and up
    (measured: 273x to 285x, 27 % of the elements).  At D = 8 the budget is its floor of 2 for 296 elements, so 50
    budgets would be a third of them: there the stand-in must move a tenth of the elements (measured: 72, 24 %)."""
    M = 37
    tot = {1.0 + 2.4e-7: 0, 1.0 - 2.4e-7: 0, "unrounded": 0}
    numel = 0
    for D in rc.NORM_WIDTHS:
        c = rc.norm_case(D, M)
        budget = rc.norm_budget(M * D)
        numel += M * D
        for s in (1.0 + 2.4e-7, 1.0 - 2.4e-7):
            worst, n = rc.norm_mismatch(_rmsnorm_perturbed(c["x"], c["w"], rc.EPS, s), c["y"])
            print(f"D {D}: r * {s!r}: {n} of {M * D} one step off (budget {budget})")
            assert worst <= 1
            assert 10 * n <= budget
            tot[s] += n
        worst, n = rc.norm_mismatch(_add_rmsnorm2_unrounded(c["h0"], c["x"], c["w"], rc.EPS), c["h1"])
        print(f"D {D}: post-norm left unrounded: {n} of {M * D} off, {n / budget:.0f} budgets")
        assert n > 50 * budget if D >= 512 else 10 * n > M * D
        tot["unrounded"] += n
    print(tot, numel)
    assert 10 * max(tot[1.0 + 2.4e-7], tot[1.0 - 2.4e-7]) <= rc.norm_budget(numel)
    assert tot["unrounded"] > 50 * rc.norm_budget(numel)


def _geglu_fast(gate: torch.Tensor, up: torch.Tensor, fma: bool = False) -> torch.Tensor:
    """The kernels' GeGLU chain on fp32 gate / up values that are already what the GELU sees:
    ``bf16(bf16(gelu_tanh_fast(gate)) * up)``."""
    act = torch.from_numpy(_fast_f32(gate.contiguous().numpy(), fma))
    return (ref.rbf(act) * up).to(BF)


def test_gpu_assertions_trip_on_wrong_stand_ins():
    """Every assertion of tests/test_rounding_chain_gpu.py, turned on the CPU against a result that is subtly wrong
    (the GPU cannot produce one without editing a kernel), next to a faithful one that passes:

    * norms (``check_norm``, ``check_residual``): the residual with the post-norm left unrounded, and a norm that
      rounds ``1 + w`` to bf16 first, both break the budget at every width; the reference with a float64 mean and a
      reciprocal root 2 ulp off passes both, although its residual is up to 16 steps from the reference's;
    * GeGLU window (``check_geglu``): PyTorch's fp32 tanh form (ops/reference.py geglu) leaves the window, the fp32
      emulation of the fast form passes, NaN / inf pattern included;
    * fused == unfused (``torch.equal``): the chain with the gate accumulator left unrounded before the GELU, or the
      up accumulator before the product, differs from the chain on the bf16 GEMM output at both shapes;
    * RoPE (``torch.equal``): cos / sin left in fp32 differs from ops/reference.py."""
    far = 0
    for D in rc.NORM_WIDTHS:
        c = rc.norm_case(D, 37)
        for s in (1.0 + 2.4e-7, 1.0 - 2.4e-7):
            n = _rmsnorm_perturbed(c["x"], c["w"], rc.EPS, s)
            rc.check_norm(n, c["y"], f"perturbed D {D}")
            worst, _ = rc.check_residual((c["h0"].float() + n.float()).to(BF), c["h0"], c["y"], f"perturbed h D {D}")
            far = max(far, worst)
        with pytest.raises(AssertionError, match="budget|not bf16"):
            rc.check_residual(_add_rmsnorm2_unrounded(c["h0"], c["x"], c["w"], rc.EPS), c["h0"], c["y"],
                              f"unrounded D {D}")
        xf = c["x"].float()
        r = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + rc.EPS)
        with pytest.raises(AssertionError, match="budget|steps"):
            rc.check_norm((xf * r * ref.rbf(1.0 + c["w"].float())).to(BF), c["y"], f"rounded weight D {D}")
    assert far > 1        # a legitimate post-norm difference is more than one step of the residual somewhere

    g = rc.geglu_case()
    gate, up = g["gu"][:, :65536].float(), g["gu"][:, 65536:].float()
    with pytest.raises(AssertionError, match="outside the window"):
        rc.check_geglu(g["want"], "fp32 tanh form")
    for fma in (False, True):
        rc.check_geglu(_geglu_fast(gate, up, fma), "fp32 emulation of the fast form")

    for M, N, K in rc.FUSED_SHAPES:
        A, W = rc.fused_operands(M, N, K)
        acc = A.float() @ W.float().t()
        ga, ua = acc[:, : N // 2], acc[:, N // 2:]
        want = _geglu_fast(ref.rbf(ga), ref.rbf(ua))
        assert torch.equal(want, _geglu_fast(ref.rbf(ga).clone(), ref.rbf(ua).clone()))
        assert not torch.equal(_geglu_fast(ga, ref.rbf(ua)), want)           # gate left unrounded
        assert not torch.equal(_geglu_fast(ref.rbf(ga), ua), want)           # up left unrounded

    for Hq, Hkv, HD in rc.ROPE_GEOMS:
        c = rc.rope_case(Hq, Hkv, HD)
        kc, vc = c["kc0"].clone(), c["vc0"].clone()
        x = c["qkv"].view(-1, Hq + 2 * Hkv, HD).float()[:, :Hq]
        p = c["pos"].long().clamp(0, rc.ROPE_TABLE - 1)
        cs, sn = c["cos"][p].unsqueeze(1), c["sin"][p].unsqueeze(1)                # not rounded to bf16
        x1, x2 = x[..., : HD // 2], x[..., HD // 2:]
        q = torch.cat([ref.rbf(ref.rbf(x1 * cs) + ref.rbf(-x2 * sn)), ref.rbf(ref.rbf(x2 * cs) + ref.rbf(x1 * sn))],
                      -1).to(BF)
        q[c["pos"] < 0] = 0
        assert q.shape == c["q"].shape and not torch.equal(q, c["q"])
        assert torch.equal(q[0], c["q"][0])                                  # position 0: cos 1, sin 0 either way
