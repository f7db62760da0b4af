"""Criteria and shared inputs for the rounding-chain tests (tests/test_rounding_chain_cpu.py and
tests/test_rounding_chain_gpu.py).  Everything here runs on the CPU and imports nothing from the GPU side.

Three criteria:

* ``bf16_ulps``: the distance between two bf16 tensors in bf16 steps.
* ``gelu_window``: for a bf16 gate, the closed interval of bf16 values the rounded tanh-GELU may take when it is
  computed in the stable form ``g / (1 + exp(-2y))`` with a few fp32 roundings (csrc/common.h gelu_tanh_fast).
* ``norm_budget``: how many elements of an RMSNorm output may sit one bf16 step away from ops/reference.py.  fp32
  differences that are legitimate (the order of the sum of squares, a reciprocal square root 2 ulp off) move about
  0.005 % of the elements by one step; a misplaced bf16 rounding moves tens of percent.  The budget, 0.1 %, sits
  between the two (tests/test_rounding_chain_cpu.py measures both sides).

``check_norm``, ``check_residual`` and ``check_geglu`` are the assertions of the GPU tests; they live here so that the
CPU suite can turn them against deliberately wrong results.

The builders return CPU tensors, seeded per case and cached: the tests share them and must not write to them.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Tuple

import torch

from taboo_brittleness_amd.ops import reference as ref

BF = torch.bfloat16
EPS = 1e-6                                        # Gemma-2's rms_norm_eps

K0, K1 = 0.7978845608028654, 0.044715             # sqrt(2 / pi) and the cubic coefficient of the tanh GELU


def _ordered(x: torch.Tensor) -> torch.Tensor:
    """bf16 -> int32 that is monotone in the value, with -0 and +0 both at 0."""
    b = x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = b & 0x7FFF
    return torch.where(b >= 0x8000, -mag, mag)


def bf16_ulps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance in bf16 steps between two bf16 tensors (int32).  +0 and -0 are equal; a NaN / NaN pair is 0 apart,
    a NaN against anything else ``2 ** 16``.  An infinity is one step past the largest finite value."""
    assert a.dtype == BF and b.dtype == BF and a.shape == b.shape
    d = (_ordered(a) - _ordered(b)).abs()
    na, nb = torch.isnan(a), torch.isnan(b)
    d = torch.where(na | nb, torch.full_like(d, 1 << 16), d)
    return torch.where(na & nb, torch.zeros_like(d), d)


def rn_bf16(x: torch.Tensor) -> torch.Tensor:
    """float64 -> bf16, one round-to-nearest-even (a cast through float32 would round twice)."""
    assert x.dtype == torch.float64
    _m, e = torch.frexp(x)                                    # |x| = m 2^e, m in [0.5, 1)
    e = e.clamp(min=-125)                                     # below 2^-126 the step stays 2^-133
    step = torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 8).double())    # the bf16 step at x, exact
    q = torch.round(x / step) * step                          # torch.round: half to even; both scalings exact
    q = torch.where(q.abs() >= 2.0 ** 128, torch.copysign(torch.full_like(q, math.inf), x), q)
    q = torch.where(torch.isfinite(x), q, x)
    return q.to(torch.float32).to(BF)                         # q is a bf16 value: both casts are exact


def _gelu_y(g: torch.Tensor) -> torch.Tensor:
    return K0 * (g + K1 * g * g * g)


def gelu64(g: torch.Tensor) -> torch.Tensor:
    """tanh-form GELU in float64, in the stable form ``g / (1 + exp(-2y))`` (no ``1 + tanh`` cancellation)."""
    assert g.dtype == torch.float64
    return g / (1.0 + torch.exp(-2.0 * _gelu_y(g)))


# |2y| past which the exponent's error no longer reaches the result: for g > 0, exp(-2y) < 2^-184 vanishes against
# the 1 in fp32 and in fp64 alike (the result is g itself); for g < 0, |t| < |g| exp(-128) < 2^-120 for every g with
# |2y| >= 128 (|g| >= 12, and |g| exp(-|2y|) falls with |g|), which the absolute term of the window covers.
_Y2_SAT = 128.0


def gelu_eps(g: torch.Tensor) -> torch.Tensor:
    """Relative error bound of the fp32 fast form at gate ``g`` (float64): ``2^-20 (4 + |2y|)``, |2y| saturating at
    128.  Derived, not measured: the result's relative error is that of ``exp(-2y)`` times ``e / (1 + e) <= 1``; the
    exponent ``-2y`` is an fp32 value built with four roundings (and one more inside ``__expf``'s scaling by log2 e),
    so its absolute error is a few 2^-24 |2y| -- bounded here by 2^-20 |2y| -- and ``v_exp_f32``, the add, ``v_rcp_f32``
    and the final multiply add about an fp32 ulp each, bounded by 4 * 2^-20.  The largest value is 1.26e-4, 3 % of a
    bf16 step."""
    return 2.0 ** -20 * (4.0 + (2.0 * _gelu_y(g)).abs().clamp(max=_Y2_SAT))


def gelu_window(g: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(lo, hi)`` bf16: the closed interval of values ``bf16(gelu(g))`` may take for bf16 gates ``g``:
    ``[RN(min(t (1 - e), t (1 + e)) - 2^-120), RN(max(..) + 2^-120)]`` with ``t = gelu64(g)``, ``e = gelu_eps(g)``.
    The 2^-120 covers ``v_rcp_f32`` returning 0 where the true reciprocal is subnormal (gates near -10).  Only
    meaningful at finite gates."""
    assert g.dtype == BF
    gd = g.double()
    t, e = gelu64(gd), gelu_eps(gd)
    a, b = t * (1.0 - e), t * (1.0 + e)
    return rn_bf16(torch.minimum(a, b) - 2.0 ** -120), rn_bf16(torch.maximum(a, b) + 2.0 ** -120)


def in_window(y: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    """Elementwise ``lo <= y <= hi`` on bf16 values (NaN is outside)."""
    yf = y.float()
    return (yf >= lo.float()) & (yf <= hi.float())


def all_bf16() -> torch.Tensor:
    """All 65536 bf16 bit patterns, in bit order."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)


def norm_budget(numel: int) -> int:
    """How many elements of a norm output of ``numel`` elements may sit one bf16 step off the reference."""
    return max(2, numel // 1000)


def norm_mismatch(got: torch.Tensor, want: torch.Tensor) -> Tuple[int, int]:
    """``(largest distance in bf16 steps, number of unequal elements)``."""
    d = bf16_ulps(got, want)
    return int(d.max()), int((d != 0).sum())


def check_norm(got: torch.Tensor, want: torch.Tensor, what: str) -> Tuple[int, int]:
    """The norm criterion: every element within one bf16 step of ``want``, at most ``norm_budget`` of them unequal.
    Prints and returns ``(largest distance, number unequal)``."""
    worst, n = norm_mismatch(got, want)
    budget = norm_budget(want.numel())
    print(f"{what}: {n} of {want.numel()} elements off (budget {budget}), largest distance {worst} step(s)")
    assert worst <= 1, f"{what}: an element is {worst} bf16 steps from the reference"
    assert n <= budget, f"{what}: {n} of {want.numel()} elements one step off, the budget is {budget}"
    return worst, n


def bf16_step(x: torch.Tensor, k: int) -> torch.Tensor:
    """The bf16 value ``k`` steps above (below for ``k < 0``) each finite element of ``x``."""
    i = _ordered(x) + k
    bits = torch.where(i < 0, 0x8000 | -i, i)
    return ((bits + 0x8000) % 0x10000 - 0x8000).to(torch.int16).view(BF)      # the same 16 bits as an int16


def check_residual(h: torch.Tensor, h0: torch.Tensor, n: torch.Tensor, what: str) -> Tuple[int, int]:
    """The norm criterion carried through the residual add ``h = bf16(h0 + n')``, ``n'`` the kernel's bf16 post-norm
    and ``n`` the reference's: every element of ``h`` is ``bf16(h0 + n')`` for an ``n'`` within one bf16 step of
    ``n``, and at most ``norm_budget`` elements differ from ``bf16(h0 + n)``.  The add and its rounding are exact
    given ``n'``, so this asks of the post-norm what :func:`check_norm` asks, and of the add bit-equality.  (The
    distance between ``h`` and the reference's ``h`` itself is no criterion: where ``h0 + n`` cancels, one step of
    ``n`` is many steps of the sum -- the reference with nothing changed but a float64 mean is 8 steps off at
    D = 8200.)  Prints and returns ``(largest distance of h from the reference's h, number of unequal elements)``."""
    hf = h0.float()
    cands = [(hf + bf16_step(n, k).float()).to(BF) for k in (0, 1, -1)]
    d0 = bf16_ulps(h, cands[0])
    ok = (d0 == 0) | (bf16_ulps(h, cands[1]) == 0) | (bf16_ulps(h, cands[2]) == 0)
    worst, cnt = int(d0.max()), int((d0 != 0).sum())
    budget = norm_budget(h.numel())
    print(f"{what}: {cnt} of {h.numel()} elements off (budget {budget}), largest distance {worst} step(s), "
          f"{int((~ok).sum())} not explained by one step of the post-norm")
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements are not bf16(h + n') for any n' one step from n"
    assert cnt <= budget, f"{what}: {cnt} of {h.numel()} elements off, the budget is {budget}"
    return worst, cnt


# ---- norm family ------------------------------------------------------------------------------------------------
# 8: the smallest launch; 2304 / 3584: Gemma-2-2B / 9B; 8192: the last width with one 16-B slot per lane (1024
# lanes); 8200 and 32768: the two ends of the four-slot path
NORM_WIDTHS = (8, 512, 2304, 3584, 8192, 8200, 32768)
NORM_ROWS = (1, 37)
NORM_MAX_D = 32768


def norm_rows(M: int, D: int, g: torch.Generator) -> torch.Tensor:
    """``randn * 3`` rows; with enough rows also a massive-activation row (one element at 3000), an all-zero row, a
    row scaled by 1e-4 (eps dominates the mean square) and a row scaled by 1e4."""
    x = torch.randn(M, D, generator=g) * 3
    if M >= 12:
        x[3, (5 * D) // 8] = 3000.0
        x[5] = 0.0
        x[7] *= 1e-4
        x[11] *= 1e4
    return x.to(BF)


@functools.lru_cache(maxsize=None)
def norm_case(D: int, M: int) -> Dict[str, torch.Tensor]:
    """Inputs of one (D, M) case and their ops/reference.py results: ``x`` rows and weights ``w`` / ``wn``
    (``randn * 0.1``), residual ``h0``; ``y = rmsnorm(x, w)``, ``h1`` = the residual after ``add_rmsnorm2(h0, x, w,
    wn)``."""
    g = torch.Generator().manual_seed(1000 * D + M)
    x = norm_rows(M, D, g)
    w = (torch.randn(D, generator=g) * 0.1).to(BF)
    wn = (torch.randn(D, generator=g) * 0.1).to(BF)
    h0 = torch.randn(M, D, generator=g).to(BF)
    h1 = h0.clone()
    ref.add_rmsnorm2(h1, x, w, wn, EPS)
    return {"x": x, "w": w, "wn": wn, "h0": h0, "y": ref.rmsnorm(x, w, EPS), "h1": h1}


@functools.lru_cache(maxsize=None)
def embed_case(D: int, M: int) -> Dict[str, torch.Tensor]:
    """An embedding table of :func:`norm_rows` scaled to embedding size, ids that include -5, V and V + 7 (clamped to
    the table) and every special row, and ops/reference.py's ``h`` / ``x`` at ``scale = sqrt(D)``."""
    g = torch.Generator().manual_seed(2000 * D + M)
    V = 23
    E = (norm_rows(V, D, g).float() * 0.02).to(BF)
    ids = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    for i, v in enumerate((-5, V, V + 7, 3, 5, 7, 11)[:M]):
        ids[i] = v
    w = (torch.randn(D, generator=g) * 0.1).to(BF)
    h, x = ref.embed_rmsnorm(ids, E, w, math.sqrt(D), EPS)
    return {"E": E, "ids": ids, "w": w, "h": h, "x": x}


def sum_splits(part: torch.Tensor) -> torch.Tensor:
    """bf16 of the fp32 split-K partials ``[ks, ...]`` added in split order starting from 0 (csrc/common.h
    sum_splits8, then the consumer's rounding)."""
    acc = torch.zeros_like(part[0])
    for s in range(part.shape[0]):
        acc = acc + part[s]
    return acc.to(BF)


# ---- GeGLU ------------------------------------------------------------------------------------------------------
GEGLU_UPS = (1.0, -1.0, 0.0078125, 3.140625, -96.0, 2.0 ** -60, 2.0 ** 60)


@functools.lru_cache(maxsize=None)
def geglu_case() -> Dict[str, torch.Tensor]:
    """``gu [8, 2 * 65536]``: every row's gate half is all bf16 bit patterns in one fixed shuffled order; the up half
    is a constant of GEGLU_UPS on rows 0..6 and ``randn * 4`` on row 7.  ``lo`` / ``hi [8, 65536]``: the bounds
    ``bf16(window edge * up)`` (a product of two bf16 values is exact in fp32, so the only rounding is the kernel's
    own), sorted so that ``lo <= hi`` whatever the sign of ``up``.  ``mid``: the same product for the correctly
    rounded ``gelu64``.  ``finite``: the gate is finite; ``normal``: and its GELU is at least 2^-100, well clear of
    the window's 2^-120 term.  ``want``: ``ops.reference.geglu(gu)``."""
    g = torch.Generator().manual_seed(65536)
    gate = all_bf16()[torch.randperm(65536, generator=g)]
    up = torch.empty(8, 65536)
    for r, u in enumerate(GEGLU_UPS):
        up[r] = u
    up[7] = torch.randn(65536, generator=g) * 4
    up = up.to(BF)
    gu = torch.cat([gate.expand(8, -1), up], 1).contiguous()
    wl, wh = gelu_window(gate)
    a, b = (wl.float() * up.float()).to(BF), (wh.float() * up.float()).to(BF)
    lo = torch.minimum(a.float(), b.float()).to(BF)
    hi = torch.maximum(a.float(), b.float()).to(BF)
    t = gelu64(gate.double())
    mid = (rn_bf16(t).float() * up.float()).to(BF)
    fin = torch.isfinite(gate.float())
    return {"gu": gu, "lo": lo, "hi": hi, "mid": mid, "finite": fin.expand(8, -1),
            "normal": (fin & (t.abs() >= 2.0 ** -100)).expand(8, -1), "want": ref.geglu(gu)}


def nonfinite_pattern(y: torch.Tensor) -> torch.Tensor:
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    yf = y.float()
    p = torch.zeros(y.shape, dtype=torch.int8)
    p[torch.isnan(yf)] = 1
    p[yf == math.inf] = 2
    p[yf == -math.inf] = 3
    return p


def check_geglu(out: torch.Tensor, what: str = "geglu") -> Tuple[int, int]:
    """The GeGLU criterion on an output ``[8, 65536]`` for :func:`geglu_case`'s input: inside ``[lo, hi]`` at every
    finite gate, the NaN / +-inf pattern of ops/reference.py at the others.  Prints and returns how much of the
    window's slack was used: ``(number of outputs that differ from the correctly rounded fp64 result ``mid``, largest
    such distance in bf16 steps)``, where the GELU and ``mid`` are at least 2^-100 (and ``mid`` is finite)."""
    c = geglu_case()
    fin = c["finite"]
    assert out.shape == c["lo"].shape and out.dtype == BF
    bad = fin & ~in_window(out, c["lo"], c["hi"])
    if bool(bad.any()):
        r, j = [int(v[0]) for v in torch.nonzero(bad, as_tuple=True)]
        gate, up = c["gu"][r, j], c["gu"][r, 65536 + j]
        raise AssertionError(f"{what}: {int(bad.sum())} outputs outside the window, first at gate {float(gate)!r} up "
                             f"{float(up)!r}: {float(out[r, j])!r} not in [{float(c['lo'][r, j])!r}, "
                             f"{float(c['hi'][r, j])!r}]")
    pat, want = nonfinite_pattern(out), nonfinite_pattern(c["want"])
    assert torch.equal(pat[~fin], want[~fin]), f"{what}: NaN / inf pattern at non-finite gates differs"
    sel = c["normal"] & (c["mid"].float().abs() >= 2.0 ** -100) & torch.isfinite(c["mid"].float())
    d = bf16_ulps(out, c["mid"])[sel]
    used = int((d != 0).sum()), int(d.max())
    print(f"{what}: {used[0]} of {int(sel.sum())} outputs (GELU and product of at least 2^-100) differ from the "
          f"correctly rounded fp64 result, by at most {used[1]} step(s)")
    return used


FUSED_SHAPES = ((37, 1024, 640), (300, 1024, 640))            # (M, N = 2F, K)


def fused_operands(M: int, N: int, K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """A ``[M, K]`` and W ``[N, K]`` uniform in (-1, 1) as bf16: gates of standard deviation sqrt(K) / 3 (8.4 at
    K = 640), which fills the [-10, -3] tail, the flush region and both saturated ends."""
    g = torch.Generator().manual_seed(M * 7 + K)
    return (torch.rand(M, K, generator=g) * 2 - 1).to(BF), (torch.rand(N, K, generator=g) * 2 - 1).to(BF)


# ---- RoPE -------------------------------------------------------------------------------------------------------
ROPE_GEOMS = ((4, 2, 256), (8, 4, 128), (1, 1, 16))          # (Hq, Hkv, HD)
ROPE_S, ROPE_TABLE, ROPE_SLOTS = 24, 40, 3
# 0, S - 1 and S (query rotated, cache untouched); 39, 40 and 57 (the table's last row, clamped to it twice, all
# past the cache); -1 (query zeroed, nothing written); one writer per (slot, position)
ROPE_POS = (0, 23, 24, 39, 40, 57, -1, 0, 23, 7, 12, 1)
ROPE_SLOT = (0, 0, 0, 1, 2, 0, 1, 2, 1, 1, 2, 0)


@functools.lru_cache(maxsize=None)
def rope_case(Hq: int, Hkv: int, HD: int) -> Dict[str, torch.Tensor]:
    """qkv rows, positions, slots and tables; random pre-fills ``kc0`` / ``vc0`` / ``q0`` of both caches and of the
    query output; ops/reference.py's results ``q`` (every row is written: rotated, or zeroed at ``pos < 0``) and
    ``kc`` / ``vc`` (the pre-fill wherever no row writes)."""
    g = torch.Generator().manual_seed(Hq * 1000 + HD)
    M = len(ROPE_POS)
    pos = torch.tensor(ROPE_POS, dtype=torch.int32)
    slot = torch.tensor(ROPE_SLOT, dtype=torch.int32)
    ok = (pos >= 0) & (pos < ROPE_S)
    assert len({(int(s), int(p)) for s, p in zip(slot[ok], pos[ok])}) == int(ok.sum())
    qkv = torch.randn(M, (Hq + 2 * Hkv) * HD, generator=g).to(BF)
    cos_t, sin_t = ref.rope_tables(HD, ROPE_TABLE, 10000.0)
    kc0 = torch.randn(ROPE_SLOTS, Hkv, ROPE_S, HD, generator=g).to(BF)
    vc0 = torch.randn(ROPE_SLOTS, Hkv, ROPE_S, HD, generator=g).to(BF)
    q0 = torch.randn(M, Hq, HD, generator=g).to(BF)
    kc, vc = kc0.clone(), vc0.clone()
    q = ref.rope_qkv_cache(qkv, pos, slot, cos_t, sin_t, kc, vc, Hq, Hkv, HD)
    return {"qkv": qkv, "pos": pos, "slot": slot, "cos": cos_t.contiguous(), "sin": sin_t.contiguous(), "kc0": kc0,
            "vc0": vc0, "q0": q0, "q": q, "kc": kc, "vc": vc}
