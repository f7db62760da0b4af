"""Operands, exact references, criteria and case runners for the in-tree MFMA GEMMs -- csrc/gemm4.hip,
csrc/gemm_ring.hip (``lora_t`` included) and ``gemm_nt`` in csrc/sae.hip (tests/test_gemm_exact_cpu.py and
tests/test_gemm_exact_gpu.py).
Everything here runs on the CPU; a runner takes the implementation under test as an object with the callables listed at
:class:`RefImpl` and the device to put the operands on, so the same cases hold the HIP kernels, the float64 reference
(``RefImpl()``) and deliberately wrong stand-ins (``RefImpl(drop_term=True)`` and friends) to the same criteria.

The primary criterion needs no tolerance.  Operands are non-zero integers in ``+-1 .. +-h`` (class ``small``: h = 2,
``wide``: h = 8), optionally with every row of A and of W scaled by a power of two (class ``scaled``, exponents within
+-12; ``shift`` scales all of A by ``2^-shift``).  A product of two bf16 values is exact in fp32; every partial sum of
one output, in any order, is an integer times the output's own power of two and is bounded by ``S = sum |a_k| |w_k| <
2^24`` times it, so every adder of at least fp32 width -- rounding or truncating, in whatever order the MFMA and the
kernel's K loop, split-K planes or chunk folds take -- gives the exact sum.  The one assumption is that the bf16 MFMA
accumulates at no less than fp32 width.  Expected values come from float64 (int64 in the CPU test of the property):

* fp32 stores and split-K partial planes equal the exact value;
* bf16 stores equal ``rn_bf16(exact)`` -- one rounding from float64 -- as int16 bits;
* JumpReLU is ``where(pre > thr, pre, 0)`` exactly, thresholds sitting on attained values;
* fused epilogues equal the pinned elementwise op (``ops.geglu``, ``ops/reference.py rope_qkv_cache``) of the uploaded
  ``rn_bf16(exact)`` tensor bit for bit; log-sum-exps and NLLs lie within ``readout_cases.lse_bound``.

Every output is a leading slice of a larger allocation whose other rows (for ``lora_t`` also columns) hold a sentinel
bit pattern, compared as integers afterwards; the slice itself is pre-filled with NaN.

Class ``tall`` (:func:`run_width`: positive 64 .. 127 at K = 1024, outputs of 24 significant bits) asks the assumption
itself.  The secondary criterion (:func:`run_uniform`) holds uniform (-1, 1) operands at K <= 320 to ``gamma S``.

The builders return CPU tensors, seeded per case and cached: the tests share them and must not write to them.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from readout_cases import Report, lse_bound
from rounding_cases import rn_bf16
from taboo_brittleness_amd import ops as _ops
from taboo_brittleness_amd.ops import reference as ref

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
NAN = float("nan")

CLASSES = ("small", "wide", "scaled")
HEIGHT = {"small": 2, "wide": 8, "scaled": 8, "tall": 127}   # tall: positive 64 .. 127, see run_width
MAX_EXP = 12
GUARD = 3                                       # guard rows behind every output
SENT16, SENT32 = 0x5A5B, 0x5A5B5C5D             # finite, never a result of these cases

HD = 256                                        # head dim of the fused QKV + RoPE epilogues


class GReport(Report):
    """:class:`readout_cases.Report` plus ``counts``: how much of each kind was checked (summed over the cases)."""

    def __init__(self) -> None:
        super().__init__()
        self.counts: Dict[str, int] = {}

    def count(self, key: str, n: int = 1) -> None:
        self.counts[key] = self.counts.get(key, 0) + int(n)

    def assert_ok(self, what: str) -> None:
        for k in sorted(self.counts):
            print(f"{what}: {k}: {self.counts[k]}")
        super().assert_ok(what)


# ---- operands and exact values -------------------------------------------------------------------------------------
def _ints(g: torch.Generator, shape, h: int) -> torch.Tensor:
    mag = torch.randint(1, h + 1, shape, generator=g)
    return mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1)


@functools.lru_cache(maxsize=None)
def operands(cls: str, M: int, N: int, K: int, shift: int = 0, seed: int = 0) -> SimpleNamespace:
    """``A [M, K]`` and ``W [N, K]`` bf16 of class ``cls`` (A times ``2^-shift``), their integers ``ai`` / ``wi``
    (int64) and row exponents ``ea`` / ``fw``.  Asserts that the bf16 operands hold the intended values exactly and that
    ``S_max = max sum_k |a_k| |w_k| <= K h^2 < 2^24``."""
    h = HEIGHT[cls]
    assert K * h * h < 2 ** 24, "S_max must stay below 2^24"
    g = torch.Generator().manual_seed(((list(HEIGHT).index(cls) * 8191 + M) * 8191 + N) * 8191 + K + 104729 * seed)
    if cls == "tall":
        ai, wi = torch.randint(64, h + 1, (M, K), generator=g), torch.randint(64, h + 1, (N, K), generator=g)
    else:
        ai, wi = _ints(g, (M, K), h), _ints(g, (N, K), h)
    if cls == "scaled":
        ea = torch.randint(-MAX_EXP, MAX_EXP + 1, (M,), generator=g)
        fw = torch.randint(-MAX_EXP, MAX_EXP + 1, (N,), generator=g)
    else:
        ea, fw = torch.zeros(M, dtype=torch.long), torch.zeros(N, dtype=torch.long)
    a64 = torch.ldexp(ai.double(), (ea - shift)[:, None])
    w64 = torch.ldexp(wi.double(), fw[:, None])
    A, W = a64.to(BF), w64.to(BF)
    assert torch.equal(A.double(), a64) and torch.equal(W.double(), w64)
    return SimpleNamespace(A=A, W=W, ai=ai, wi=wi, ea=ea, fw=fw, shift=shift, cls=cls)


def exact(A: torch.Tensor, W: torch.Tensor, dev=None) -> torch.Tensor:
    """``A @ W^T`` in float64 (on ``dev`` where given; the result comes back to the CPU).  For the integer classes
    every partial sum is an integer below 2^24 times the output's power of two, so float64 adds without rounding."""
    if dev is None:
        return A.double() @ W.double().t()
    return (A.to(dev).double() @ W.to(dev).double().t()).cpu()


def s_max(op: SimpleNamespace) -> int:
    """The largest ``sum_k |a_k| |w_k|`` over the outputs, on the integers."""
    return int((op.ai.abs().double() @ op.wi.abs().double().t()).max())


def bf16_ties(E: torch.Tensor) -> torch.Tensor:
    """Where the float64 values sit exactly halfway between two bf16 values."""
    _m, e = torch.frexp(E)
    t = torch.ldexp(E.abs(), 9 - e.clamp(min=-125))               # |E| in half steps
    return (t == torch.floor(t)) & (torch.remainder(t, 2) == 1)


def bf16_lossless(E: torch.Tensor) -> torch.Tensor:
    return rn_bf16(E).double() == E


def pack_trunc(x: torch.Tensor) -> torch.Tensor:
    """float64 (holding fp32 values) -> bf16 by dropping the low 16 bits."""
    b = x.float().contiguous().view(torch.int32) & -65536
    return b.view(F32).to(BF)


def pack_away(x: torch.Tensor) -> torch.Tensor:
    """float64 -> bf16, ties away from zero."""
    r = rn_bf16(x).double()
    tie = bf16_ties(x)
    _m, e = torch.frexp(x)
    step = torch.ldexp(torch.ones_like(x), e.clamp(min=-125) - 8)
    away = torch.where(r.abs() > x.abs(), r, r + torch.copysign(step, x))
    return torch.where(tie, away, r).float().to(BF)


@functools.lru_cache(maxsize=None)
def interleave(F: int) -> torch.Tensor:
    return _ops.geglu_interleave_index(F)


@functools.lru_cache(maxsize=None)
def case(cls: str, M: int, N: int, K: int, shift: int = 0, seed: int = 0) -> SimpleNamespace:
    """One GEMM case and everything expected of it: the operands, ``E`` (float64 exact), ``Ebf`` (``rn_bf16(E)``),
    ``Wi`` (W's rows in GeGLU-interleaved order, where N allows), the JumpReLU ``bias`` / ``thr`` (integers on the
    unscaled classes; ``thr`` is the column's most frequent value of ``pre`` -- on class ``scaled`` its lower median --
    on seven columns of eight and a little below it on the eighth) with ``jump`` the expected result and ``n_eq`` the
    number of ``pre == thr``."""
    op = operands(cls, M, N, K, shift, seed)
    E = exact(op.A, op.W)
    c = SimpleNamespace(**vars(op), M=M, N=N, K=K, E=E, Ebf=rn_bf16(E))
    c.n_ties = int(bf16_ties(E).sum())
    g = torch.Generator().manual_seed(M * 31 + N * 7 + K)
    scale = 2.0 ** -shift
    bias = torch.zeros(N) if cls == "scaled" else torch.randint(-4, 5, (N,), generator=g).float() * scale
    pre = E + bias.double()
    med = pre.median(0).values if cls == "scaled" else pre.mode(0).values      # scaled: hardly any value repeats
    low = med * 0.5 if cls == "scaled" else med - (1.0 + (torch.arange(N) % 5).double()) * scale
    thr = torch.where(torch.arange(N) % 8 != 7, med, low).float()
    assert torch.equal(thr.double().float(), thr) and torch.equal(pre.float().double(), pre)
    c.bias, c.thr = bias, thr
    c.jump = torch.where(pre > thr.double(), pre, torch.zeros_like(pre)).float()
    c.n_eq = int((pre == thr.double()).sum())
    if N % 256 == 0:
        c.Wi = op.W[interleave(N // 2)].contiguous()
    return c


# ---- outputs with guards -------------------------------------------------------------------------------------------
class Out:
    """An output ``[M, N]`` as the leading rows of a ``[M + GUARD, N + gcols]`` allocation: the output NaN, the guard
    rows (and the ``gcols`` guard columns) a sentinel bit pattern."""

    def __init__(self, dev, M: int, N: int, dtype, gcols: int = 0) -> None:
        self.M, self.N = M, N
        if dtype in (BF, F32):
            self.buf = torch.full((M + GUARD, N + gcols), NAN, dtype=dtype, device=dev)
            self.ibuf = self.buf.view(torch.int16 if dtype == BF else torch.int32)
            self.sent = SENT16 if dtype == BF else SENT32
        else:                                        # int32 outputs
            self.buf = torch.full((M + GUARD, N + gcols), -7, dtype=dtype, device=dev)
            self.ibuf, self.sent = self.buf, SENT32
        self.ibuf[M:] = self.sent
        if gcols:
            self.ibuf[:, N:] = self.sent
        self.c = self.buf[:M]                        # what the kernel is handed (contiguous)

    def guard_ok(self) -> bool:
        ok = bool((self.ibuf[self.M:] == self.sent).all())
        return ok and bool((self.ibuf[:, self.N:] == self.sent).all())

    def got(self) -> torch.Tensor:
        return self.buf[:self.M, :self.N]


def _first(bad: torch.Tensor) -> Tuple[int, ...]:
    return tuple(int(v) for v in bad.nonzero()[0])


def check_out(rep: GReport, what: str, out: Out, want: torch.Tensor) -> None:
    """``out`` against ``want`` (on ``out``'s device): bf16 as int16 bits, fp32 and integers by value (a NaN -- an
    unwritten cell -- differs from everything); the guards as integers."""
    got = out.got()
    if got.dtype == BF:
        bad = got.contiguous().view(torch.int16) != want.contiguous().view(torch.int16)
    else:
        bad = ~(got == want)
    n = int(bad.sum())
    rep.use(what.split(":")[0] + " mismatches", n)
    if n:
        i = _first(bad)
        rep.fail(f"{what}: {n} of {bad.numel()} outputs differ, first at {i}: got {float(got[i])!r}, want "
                 f"{float(want[i])!r}")
    if not out.guard_ok():
        rep.fail(f"{what}: a guard cell outside the output was written")


def check_bound(rep: GReport, what: str, got: torch.Tensor, want64: torch.Tensor, bound: torch.Tensor) -> None:
    """``|got - want64| <= bound`` elementwise (CPU float64); NaN fails."""
    frac = (got.detach().cpu().double().reshape(want64.shape) - want64).abs() / bound
    bad = ~(frac <= 1.0)
    if bool(bad.any()):
        i = _first(bad)
        rep.fail(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound, first at {i}: "
                 f"{float(frac[i]):.3g} of it")
    else:
        rep.use(what.split(":")[0], float(frac.max()) if frac.numel() else 0.0)


def _bf(dev, M, N, gcols=0) -> Out:
    return Out(dev, M, N, BF, gcols)


def _f32(dev, M, N) -> Out:
    return Out(dev, M, N, F32)


def geglu_want(Ebf_gu: torch.Tensor, dev) -> torch.Tensor:
    """``ops.geglu`` (pinned by the rounding-chain tests) of the uploaded gate|up tensor."""
    return _ops.geglu(Ebf_gu.to(dev).contiguous())


# ---- gemm4: every epilogue, both tile heights, both K loops -------------------------------------------------------
G4_KS = (64, 128, 192, 256, 320, 3584)          # one K tile; two; the first streamed size, odd; even; odd; the model's
G4_MS = (1, 127, 128, 129, 255, 256, 257, 513)
G4_NS = (256, 512)
G4_LAUNCHES = ((256, 0), (256, 1), (128, 1))    # (tile rows, streamed K loop on)
GEGLU_SHIFT = 3


def g4_cases(K: int) -> List[Tuple[str, int, int]]:
    """``(class, M, N)`` for one K: every M once, N alternating, the class rotating with K and M so that every K
    (up to 320) and every M meets all three classes over the table; K = 3584 takes ``wide`` alone."""
    ik = G4_KS.index(K)
    return [("wide" if K > 320 else CLASSES[(im + ik) % 3], M, G4_NS[(im + ik) % 2]) for im, M in enumerate(G4_MS)]


@functools.lru_cache(maxsize=None)
def gate_case(cls: str, M: int, N: int, K: int) -> SimpleNamespace:
    """The GeGLU case: ``case(.., shift=3)``, so the gates of class ``small`` (sd ``2.5 sqrt(K) / 8``: 2.5 at K = 64)
    fill the [-10, -3] tail, the centre and both saturated ends; ``tail`` / ``gmin`` / ``gmax`` describe the bf16
    gates.  A ``small`` case of 255 rows or more takes the first seed that puts 1000 gates in the tail and reaches
    past -10 and 10 (at K = 64 those are four standard deviations out), and asserts it."""
    for seed in range(16):
        c = case(cls, M, N, K, GEGLU_SHIFT, seed)
        gates = c.Ebf[:, : N // 2].float()
        c.tail = int(((gates >= -10) & (gates <= -3)).sum())
        c.gmin, c.gmax = float(gates.min()), float(gates.max())
        if cls != "small" or M < 255 or (c.tail >= 1000 and c.gmin < -10 and c.gmax > 10):
            return c
    raise AssertionError(f"no seed spreads the gates of {cls} M {M} N {N} K {K}")


def run_gemm4(impl, dev, K: int, cases: Optional[Sequence[Tuple[str, int, int]]] = None,
              launches=G4_LAUNCHES, epis=(0, 1, 2, 3)) -> GReport:
    rep = GReport()
    for cls, M, N in (g4_cases(K) if cases is None else cases):
        c = case(cls, M, N, K)
        A, W = c.A.to(dev), c.W.to(dev)
        want = {0: c.Ebf.to(dev), 1: c.E.float().to(dev), 2: c.jump.to(dev)}
        args = {0: (W, None, None), 1: (W, None, None), 2: (W, c.bias.to(dev), c.thr.to(dev))}
        if 3 in epis:
            gc = gate_case(cls, M, N, K)
            Ag = gc.A.to(dev)
            want[3] = geglu_want(gc.Ebf, dev)
            args[3] = (gc.Wi.to(dev), None, None)
        for tile, pipe in launches:
            old = impl.set_pipe(pipe)
            try:
                for epi in epis:
                    out = (_f32 if epi in (1, 2) else _bf)(dev, M, N // 2 if epi == 3 else N)
                    w, b, th = args[epi]
                    impl.gemm4(Ag if epi == 3 else A, w, out.c, b, th, epi, tile, None)
                    check_out(rep, f"gemm4 epi {epi}: {cls} M {M} N {N} K {K} tile {tile} pipe {pipe}", out, want[epi])
            finally:
                impl.set_pipe(old)
        rep.count("bf16 ties among the checked outputs", c.n_ties * len(launches))
        rep.count("pre == thr among the checked outputs", c.n_eq * len(launches))
        rep.count("launches", len(launches) * len(epis))
    return rep


# ---- RoPE positions ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rope_rows(M: int) -> SimpleNamespace:
    """Positions, slots, tables and cache geometry for ``M`` rows: 7 slots, row ``m`` writes ``(m % 7, m // 7)`` -- one
    writer per cache entry, both cache ends ``0`` and ``S - 1`` hit -- except every 11th row from the sixth, which takes
    in turn ``S`` (past the cache), ``T - 1`` (the table's last row), ``T`` and ``T + 17`` (clamped to it) and ``-1`` (a
    padding row: q zeroed, nothing written)."""
    S = (M - 1) // 7 + 1
    T = S + 16
    pos = (torch.arange(M, dtype=torch.int32) // 7).contiguous()
    slot = (torch.arange(M, dtype=torch.int32) % 7).contiguous()
    odd = (S, T - 1, T, T + 17, -1)
    for j, m in enumerate(range(5, M - 1, 11)):
        pos[m] = odd[j % 5]
    assert int(pos[0]) == 0 and int(pos[M - 1]) == S - 1
    cos_t, sin_t = ref.rope_tables(HD, T, 10000.0)
    return SimpleNamespace(S=S, T=T, pos=pos, slot=slot, cos=cos_t.contiguous(), sin=sin_t.contiguous())


@functools.lru_cache(maxsize=None)
def rope_fill(Hkv: int, S: int) -> Tuple[torch.Tensor, torch.Tensor]:
    g = torch.Generator().manual_seed(Hkv * 100 + S)
    return torch.randn(7, Hkv, S, HD, generator=g).to(BF), torch.randn(7, Hkv, S, HD, generator=g).to(BF)


def rope_want(Ebf: torch.Tensor, M: int, Hq: int, Hkv: int):
    """``(q, kc, vc)`` of ops/reference.py ``rope_qkv_cache`` (pinned by ``test_rope_and_cache_bit_equal``) on the
    bf16 qkv rows ``Ebf``, over random cache pre-fills."""
    rr = rope_rows(M)
    kc0, vc0 = rope_fill(Hkv, rr.S)
    kc, vc = kc0.clone(), vc0.clone()
    q = ref.rope_qkv_cache(Ebf.contiguous(), rr.pos, rr.slot, rr.cos, rr.sin, kc, vc, Hq, Hkv, HD)
    return q.reshape(M, Hq * HD).contiguous(), kc, vc


def run_rope(rep: GReport, what: str, impl, dev, family: str, tile, A, W, M: int, Hq: int, Hkv: int, want, a2=None):
    """One fused QKV + RoPE + KV-scatter launch against ``want = rope_want(..)`` uploaded to ``dev``."""
    rr = rope_rows(M)
    kc0, vc0 = rope_fill(Hkv, rr.S)
    q = _bf(dev, M, Hq * HD)
    kc, vc = kc0.to(dev).clone(), vc0.to(dev).clone()
    impl.qkv_rope(family, tile, A, W, rr.pos.to(dev), rr.slot.to(dev), rr.cos.to(dev), rr.sin.to(dev),
                  q.c.view(M, Hq, HD), kc, vc, Hq, Hkv, a2)
    check_out(rep, f"{what} q", q, want[0])
    for name, got, w in (("K cache", kc, want[1]), ("V cache", vc, want[2])):
        bad = got.view(torch.int16) != w.view(torch.int16)
        if bool(bad.any()):
            rep.fail(f"{what} {name}: {int(bad.sum())} of {bad.numel()} entries differ, first at {_first(bad)}")


# ---- several tiles per workgroup ----------------------------------------------------------------------------------
MANY_M, MANY_N, MANY_KS = 4400, 4096, (192, 256, 320)      # 18 x 16 = 288 tiles of 256 x 256
MANY_HQ, MANY_HKV = 8, 4


def many_tiles(M: int, N: int) -> int:
    return -(-M // 256) * (N // 256)


def lens_want(Ebf: torch.Tensor):
    """``(lse64, bound)`` of bf16 logits: their float64 log-sum-exp and ``lse_bound`` at the span ``max - min``."""
    z = Ebf.double()
    lse = torch.logsumexp(z, -1)
    return lse, lse_bound(lse, z.max(-1).values - z.min(-1).values)


def run_many(impl, dev, K: int, M: int = MANY_M, N: int = MANY_N, Hq: int = MANY_HQ, Hkv: int = MANY_HKV,
             cus: Optional[int] = None) -> GReport:
    """One ``small`` case scaled by 2^-3 with more 256 x 256 tiles than the device has compute units (``cus``), so a
    persistent workgroup takes several: epilogues 0 and 3, the fused RoPE and the lens epilogue of one exact product,
    computed in float64 on ``dev``."""
    rep = GReport()
    if cus is not None:
        assert many_tiles(M, N) > cus, f"{many_tiles(M, N)} tiles do not exceed the {cus} compute units"
    assert N == (Hq + 2 * Hkv) * HD and N % 256 == 0
    op = operands("small", M, N, K, GEGLU_SHIFT)
    A, W = op.A.to(dev), op.W.to(dev)
    E = exact(op.A, op.W, dev)
    Ebf = rn_bf16(E)
    tag = f"M {M} N {N} K {K}"
    want0 = Ebf.to(dev)
    for tile in (256, 128):
        out = _bf(dev, M, N)
        impl.gemm4(A, W, out.c, None, None, 0, tile, None)
        check_out(rep, f"gemm4 epi 0: {tag} tile {tile}", out, want0)
    # GeGLU: the same product with W's rows interleaved
    Wi = op.W[interleave(N // 2)].contiguous().to(dev)
    wantg = geglu_want(Ebf, dev)
    for tile in (256, 128):
        out = _bf(dev, M, N // 2)
        impl.gemm4(A, Wi, out.c, None, None, 3, tile, None)
        check_out(rep, f"gemm4 epi 3: {tag} tile {tile}", out, wantg)
    wr = tuple(t.to(dev) for t in rope_want(Ebf, M, Hq, Hkv))
    for tile in (256, 128):
        run_rope(rep, f"gemm4 rope: {tag} tile {tile}", impl, dev, "g4", tile, A, W, M, Hq, Hkv, wr)
    lg, lse = _bf(dev, M, N), _f32(dev, M, 1)
    impl.lens(A, W, lg.c, lse.c.view(M))
    check_out(rep, f"lens logits: {tag}", lg, want0)
    l64, bound = lens_want(Ebf)
    check_bound(rep, f"lens lse: {tag}", lse.got().reshape(M), l64, bound)
    if not lse.guard_ok():
        rep.fail(f"lens lse: {tag}: a guard cell outside the output was written")
    rep.count("bf16 ties among the checked outputs", int(bf16_ties(E).sum()))
    rep.count("tiles per launch", many_tiles(M, N))
    return rep


# ---- two-source A ---------------------------------------------------------------------------------------------------
L2A_SHAPES = ((128, 256), (128, 640), (512, 640))          # (k0, K)
L2A_M, L2A_N = 130, 1024                                   # N = (2 + 2) * 256: Hq = 2, Hkv = 1


def run_two_source(impl, dev, k0: int, K: int, M: int = L2A_M, N: int = L2A_N) -> GReport:
    """``[x | a2]`` read from two tensors: gemm4 at both tile heights (epilogues 0, 3 and the fused RoPE) and every
    ring tile with variant 1 (epilogues 0, 3 and RoPE), against the exact product of the concatenation."""
    rep = GReport()
    cls = CLASSES[(k0 // 128 + K // 128) % 3]
    c, gc = case(cls, M, N, K), gate_case(cls, M, N, K)
    Hq, Hkv = N // HD - 2, 1
    want0, wantg = c.Ebf.to(dev), geglu_want(gc.Ebf, dev)
    wr = tuple(t.to(dev) for t in rope_want(c.Ebf, M, Hq, Hkv))
    x, a2 = c.A[:, :k0].contiguous().to(dev), c.A[:, k0:].contiguous().to(dev)
    xg, a2g = gc.A[:, :k0].contiguous().to(dev), gc.A[:, k0:].contiguous().to(dev)
    W, Wi = c.W.to(dev), gc.Wi.to(dev)
    tag = f"{cls} M {M} N {N} k0 {k0} K {K}"
    for tile in (256, 128):
        out = _bf(dev, M, N)
        impl.gemm4(x, W, out.c, None, None, 0, tile, a2)
        check_out(rep, f"gemm4 two-source epi 0: {tag} tile {tile}", out, want0)
        out = _bf(dev, M, N // 2)
        impl.gemm4(xg, Wi, out.c, None, None, 3, tile, a2g)
        check_out(rep, f"gemm4 two-source epi 3: {tag} tile {tile}", out, wantg)
        run_rope(rep, f"gemm4 two-source rope: {tag} tile {tile}", impl, dev, "g4", tile, x, W, M, Hq, Hkv, wr, a2)
        rep.count("gemm4 launches", 3)
    for epi in (0, 3, 4):
        for bm, bn in impl.ring_tiles(epi):
            if not impl.ring_ok(M, N, K, epi, bm, bn, 1):
                continue
            what = f"ring two-source epi {epi}: {tag} tile {bm}x{bn} variant 1"
            if epi == 4:
                run_rope(rep, what, impl, dev, "ring", (bm, bn, 1), x, W, M, Hq, Hkv, wr, a2)
            else:
                out = _bf(dev, M, N // 2 if epi == 3 else N)
                impl.gemm_ring(xg if epi else x, Wi if epi else W, out.c, epi, bm, bn, 1, a2g if epi else a2)
                check_out(rep, what, out, wantg if epi else want0)
            rep.count("ring launches")
    return rep


# ---- split-K --------------------------------------------------------------------------------------------------------
SPLIT_MS, SPLIT_TILES, SPLIT_N = (1, 65, 300), (64, 128, 256), 512
# at K = 640 (10 K tiles): one split; 4, 4, 2; 3, 3, 3, 1; 7 rounds to 5 of 2; 1 each; 64 clamps to 10
SPLIT_KS = (1, 3, 4, 7, 10, 64)


def split_count(K: int, ks: int) -> Tuple[int, int]:
    """``(splits used, K tiles per split)`` for a request of ``ks`` splits: ``kc = ceil(NT / min(ks, NT))`` tiles each,
    ``ceil(NT / kc)`` splits, so that none is empty."""
    NT = K // 64
    kc = -(-NT // max(1, min(ks, NT)))
    return -(-NT // kc), kc


@functools.lru_cache(maxsize=None)
def split_prefix(cls: str, M: int, N: int, K: int) -> torch.Tensor:
    """``P [NT + 1, M, N]`` float64: ``P[t]`` the exact product over the first ``t`` 64-deep K tiles."""
    op = operands(cls, M, N, K)
    A, W = op.A.double(), op.W.double()
    P = torch.zeros(K // 64 + 1, M, N, dtype=F64)
    for t in range(K // 64):
        P[t + 1] = P[t] + A[:, 64 * t: 64 * t + 64] @ W[:, 64 * t: 64 * t + 64].t()
    return P


def run_splitk(impl, dev, K: int, splits: Sequence[int], Ms: Sequence[int] = SPLIT_MS,
               tiles: Sequence[int] = SPLIT_TILES, N: int = SPLIT_N) -> GReport:
    """``splits``: requested split counts; 0 asks the launcher's heuristic (``impl.splitk_ks``).  Per (M, tile, ks):
    the split count returned, every fp32 partial plane against the exact sum over its own K range (the plane behind
    the last is the guard), the reduced bf16 and GeGLU outputs against the exact expectation and, bit for bit, against
    the unsplit kernel."""
    rep = GReport()
    for im, M in enumerate(Ms):
        cls = "wide" if K > 640 else CLASSES[im % 3]
        c, gc = case(cls, M, N, K), gate_case(cls, M, N, K)
        P = split_prefix(cls, M, N, K)
        assert torch.equal(P[-1], c.E)
        A, W, Ag, Wi = c.A.to(dev), c.W.to(dev), gc.A.to(dev), gc.Wi.to(dev)
        want0, wantg = c.Ebf.to(dev), geglu_want(gc.Ebf, dev)
        for tile in tiles:
            plain0, plaing = _bf(dev, M, N), _bf(dev, M, N // 2)
            impl.gemm4(A, W, plain0.c, None, None, 0, max(tile, 128), None)
            impl.gemm4(Ag, Wi, plaing.c, None, None, 3, max(tile, 128), None)
            for ks in splits:
                req = ks if ks > 0 else int(impl.splitk_ks(M, N, K, tile))
                used, kc = split_count(K, req)
                tag = f"{cls} M {M} N {N} K {K} tile {tile} ks {ks}"
                ws = Out(dev, used * M, N, F32)                      # `used` planes of M rows, then the guard rows
                got = int(impl.splitk_part(A, W, ws.c.view(-1), tile, req))
                if got != used:
                    rep.fail(f"split count: {tag}: the launcher used {got} splits, the ceil formula gives {used}")
                    continue
                lo = torch.arange(used) * kc
                hi = (lo + kc).clamp(max=K // 64)
                check_out(rep, f"split-K planes: {tag}", ws, (P[hi] - P[lo]).float().reshape(used * M, N).to(dev))
                for epi, a, w, want, plain in ((0, A, W, want0, plain0), (3, Ag, Wi, wantg, plaing)):
                    ws2 = Out(dev, used * M, N, F32)
                    out = _bf(dev, M, N // 2 if epi == 3 else N)
                    impl.splitk(a, w, out.c, ws2.c.view(-1), epi, tile, req)
                    check_out(rep, f"split-K reduced epi {epi}: {tag}", out, want)
                    if not ws2.guard_ok():
                        rep.fail(f"split-K reduced epi {epi}: {tag}: wrote behind its last plane")
                    if not torch.equal(out.got().view(torch.int16), plain.got().view(torch.int16)):
                        rep.fail(f"split-K reduced epi {epi}: {tag}: differs from the unsplit kernel")
                rep.count("partial planes checked", used)
    return rep


# ---- ring GEMM -------------------------------------------------------------------------------------------------------
# fewer K tiles than ring stages; no multiple of the stage count; every variant's unroll; wrap-around; the model's
RING_KS = (128, 384, 512, 1152, 3584)
RING_MS = (1, 17, 130)
RING_N = {0: 896, 3: 256, 4: 1024}              # 896 = 2^7 * 7 divides by every bn, 112 included; RoPE: Hq = 2, Hkv = 1
RING_PLAIN = ((16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 32), (64, 64), (128, 32), (64, 128), (128, 64),
              (128, 128))
RING_N112 = tuple((bm, 112) for bm in (16, 32, 48, 64, 96, 128, 144, 192, 256))
RING_PAIR = RING_PLAIN[1:]


def ring_admitted(epi: int, N: int, K: int) -> List[Tuple[int, int, int]]:
    """The (bm, bn, variant) the ring GEMM is documented to take at (N, K), a restatement of the rules in
    csrc/gemm_ring.hip's comments: K a multiple of 128; N of bn; the 112-column tiles with the 144 KB ring (variant 1)
    only; variant 2 where 4 or 8 K tiles per stage fit four stages in 144 KB -- ``(bm + bn) * 128 * ku * 4 <= 144 KB``
    -- go deeper than variant 1's two, and divide K."""
    out = []
    for bm, bn in (RING_PLAIN + RING_N112 if epi == 0 else RING_PAIR):
        for var in (0, 1, 2):
            if K % 128 or N % bn or (bn == 112 and var != 1):
                continue
            if var == 2:
                ku = next((u for u in (8, 4) if (bm + bn) * 128 * u * 4 <= 144 * 1024), 0)
                ku1 = 2 if (bm + bn) * 128 * 2 * 3 <= 144 * 1024 else 1
                if ku <= ku1 or K % (64 * ku):
                    continue
            out.append((bm, bn, var))
    return out


def run_ring(impl, dev, epi: int, K: int, Ms: Sequence[int] = RING_MS) -> GReport:
    """Every tile of ``impl.ring_tiles(epi)`` x variants 0 / 1 / 2 that ``impl.ring_ok`` admits -- which must be the
    documented set -- at N = ``RING_N[epi]``."""
    rep = GReport()
    N = RING_N[epi]
    for im, M in enumerate(Ms):
        cls = "wide" if K > 640 else CLASSES[(im + K // 128) % 3]
        c = gate_case(cls, M, N, K) if epi == 3 else case(cls, M, N, K)
        A = c.A.to(dev)
        W = (c.Wi if epi == 3 else c.W).to(dev)
        if epi == 4:
            Hq, Hkv = N // HD - 2, 1
            want = tuple(t.to(dev) for t in rope_want(c.Ebf, M, Hq, Hkv))
        else:
            want = geglu_want(c.Ebf, dev) if epi == 3 else c.Ebf.to(dev)
        ran = []
        for bm, bn in impl.ring_tiles(epi):
            for var in (0, 1, 2):
                if not impl.ring_ok(M, N, K, epi, bm, bn, var):
                    continue
                ran.append((bm, bn, var))
                what = f"ring epi {epi}: {cls} M {M} N {N} K {K} tile {bm}x{bn} variant {var}"
                if epi == 4:
                    run_rope(rep, what, impl, dev, "ring", (bm, bn, var), A, W, M, Hq, Hkv, want)
                else:
                    out = _bf(dev, M, N // 2 if epi == 3 else N)
                    impl.gemm_ring(A, W, out.c, epi, bm, bn, var, None)
                    check_out(rep, what, out, want)
        if sorted(ran) != sorted(ring_admitted(epi, N, K)):
            rep.fail(f"ring epi {epi} N {N} K {K} M {M}: ring_ok admits {len(ran)} tile / variant combinations, the "
                     f"documented rule {len(ring_admitted(epi, N, K))}")
        rep.count("tile / variant combinations run", len(ran))
        rep.count("bf16 ties among the checked outputs", c.n_ties * len(ran))
    return rep


# ---- gemm_nt ---------------------------------------------------------------------------------------------------------
NT_KS = (32, 96, 160, 640)                      # the first three end in the zero-filled half tile
NT_NS = (1, 130, 200, 256)
NT_MS = (1, 129, 257)


def run_gemm_nt(impl, dev, K: int, Ms: Sequence[int] = NT_MS, Ns: Sequence[int] = NT_NS) -> GReport:
    rep = GReport()
    for im, M in enumerate(Ms):
        for i_n, N in enumerate(Ns):
            cls = CLASSES[(im + i_n + NT_KS.index(K)) % 3]
            c = case(cls, M, N, K)
            A, W = c.A.to(dev), c.W.to(dev)
            for epi, want in ((0, c.Ebf), (1, c.E.float()), (2, c.jump)):
                out = (_bf if epi == 0 else _f32)(dev, M, N)
                b, th = (c.bias.to(dev), c.thr.to(dev)) if epi == 2 else (None, None)
                impl.gemm_nt(A, W, out.c, b, th, epi)
                check_out(rep, f"gemm_nt epi {epi}: {cls} M {M} N {N} K {K}", out, want.to(dev))
            rep.count("bf16 ties among the checked outputs", c.n_ties)
            rep.count("pre == thr among the checked outputs", c.n_eq)
    return rep


# ---- lora_t ----------------------------------------------------------------------------------------------------------
LORA_N, LORA_LDT, LORA_NSR, LORA_NR, LORA_R = 192, 224, 176, 64, 16
LORA_KS = (128, 512, 640, 1024)                 # 1 / 1 / 5 / 2 chunks of the T chain
LORA_MS = (1, 17, 130)
LORA_TILES = tuple((bm, bn) for bn in (32, 64, 96) for bm in (16, 32, 64, 128) if (bm, bn) != (128, 96))


def lora_chunks(K: int) -> int:
    return K // 512 if K % 512 == 0 else K // 128


@functools.lru_cache(maxsize=None)
def lora_case(M: int, K: int) -> SimpleNamespace:
    """A ``wide`` case at N = 192 with adapters in ``[-1, 3]`` (four of 16 columns in every 64; -1 the base model),
    ``nsr`` = 176 < N: ``want`` holds ``rn_bf16(exact)`` on a row's own columns below ``nsr`` and +0 elsewhere."""
    c = case(("wide", "scaled", "small")[M % 3], M, LORA_N, K)
    g = torch.Generator().manual_seed(M + K)
    ad = torch.randint(-1, LORA_NR // LORA_R, (M,), generator=g, dtype=torch.int32)
    if M >= 4:
        ad[1], ad[2] = -1, LORA_NR // LORA_R - 1
    col = torch.arange(LORA_N)
    keep = (col[None] < LORA_NSR) & (((col % LORA_NR) // LORA_R)[None] == ad.long()[:, None]) & (ad[:, None] >= 0)
    return SimpleNamespace(c=c, ad=ad, keep=keep, want=torch.where(keep, c.Ebf, torch.zeros_like(c.Ebf)))


def run_lora_t(impl, dev, K: int, Ms: Sequence[int] = LORA_MS) -> GReport:
    """Every ``lora_t_ok`` tile (which must be the documented eleven), unsplit and with the fp32 chunk sums folded by
    the second kernel, into a T that is 32 columns wider than N: masked columns exactly +0, owned columns
    ``rn_bf16(exact)``, the columns past N and the rows past M untouched."""
    rep = GReport()
    for M in Ms:
        lc = lora_case(M, K)
        x, a, ad, want = lc.c.A.to(dev), lc.c.W.to(dev), lc.ad.to(dev), lc.want.to(dev)
        tiles = [(bm, bn) for bn in (32, 64, 96) for bm in (16, 32, 48, 64, 96, 128)
                 if impl.lora_t_ok(M, LORA_N, K, bm, bn)]
        if sorted(tiles) != sorted(LORA_TILES):
            rep.fail(f"lora_t M {M} K {K}: lora_t_ok admits {sorted(tiles)}")
        for bm, bn in tiles:
            for split in (False, True):
                t = _bf(dev, M, LORA_N, LORA_LDT - LORA_N)
                part = torch.full((lora_chunks(K) * M * LORA_N if split else 0,), NAN, device=dev)
                impl.lora_t(x, a, t.buf[:M], ad, LORA_NSR, LORA_NR, LORA_R, bm, bn, part)
                check_out(rep, f"lora_t: M {M} K {K} tile {bm}x{bn} split {int(split)}", t, want)
                rep.count("launches")
        rep.count("masked columns checked as +0", int((~lc.keep).sum()) * 2 * len(tiles))
    return rep


# ---- fused head and lens ---------------------------------------------------------------------------------------------
HEAD_V, HEAD_K, HEAD_MS, HEAD_CAPS = 1024, 192, (1, 300), (30.0, 0.0)
# W rows made identical: inside one 128-column slice; across two slices of one tile; across the 256-column tile
# boundary; the last row of the vocabulary
HEAD_TIES = {"slice": (5, 7), "slices": (40, 200), "tiles": (250, 260), "last": (900, HEAD_V - 1)}


@functools.lru_cache(maxsize=None)
def head_case(M: int) -> SimpleNamespace:
    """``small`` operands times 2^-3 (logits of sd 4.3) with planted ties: row ``m`` is of kind ``(m + 2) % 5`` --
    ``slice``, ``slices``, ``tiles``, ``last`` or none -- and has its first 64 features aligned with the kind's
    duplicated W rows, which lifts both to about 32, above the rest of the row.  Asserts from the reference alone that
    rows of every kind (of kind ``tiles`` at M = 1) have exactly that pair as their maxima, under both caps."""
    V, K = HEAD_V, HEAD_K
    op = operands("small", M, V, K, GEGLU_SHIFT)
    ai, wi = op.ai.clone(), op.wi.clone()
    kinds = list(HEAD_TIES)
    for lo, hi in HEAD_TIES.values():
        wi[hi] = wi[lo]
    kind = [(m + 2) % 5 for m in range(M)]
    for m in range(M):
        if kind[m] < 4:
            ai[m, :64] = 2 * torch.sign(wi[HEAD_TIES[kinds[kind[m]]][0], :64])
    A, W = torch.ldexp(ai.double(), torch.tensor(-GEGLU_SHIFT)).to(BF), wi.double().to(BF)
    assert int((ai.abs().double() @ wi.abs().double().t()).max()) < 2 ** 24
    E = exact(A, W)
    Ebf = rn_bf16(E)
    g = torch.Generator().manual_seed(M)
    tgt = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    tgt[::7] = -1
    tgt[1::9] = 7
    c = SimpleNamespace(A=A, W=W, E=E, Ebf=Ebf, tgt=tgt, kind=kind, M=M)
    c.ref = {}
    for cap in HEAD_CAPS:
        z = ref._capped(Ebf, cap, True).double()                   # bf16 values, exact
        zmax, zmin = z.max(-1).values, z.min(-1).values
        lse = torch.logsumexp(z, -1)
        amax = torch.from_numpy(np.argmax(z.numpy(), axis=-1)).long()
        seen = set()
        for m in range(M):
            top = (z[m] == zmax[m]).nonzero().reshape(-1).tolist()
            if kind[m] < 4 and top == list(HEAD_TIES[kinds[kind[m]]]):
                seen.add(kinds[kind[m]])
        assert seen == (set(kinds) if M >= 5 else {kinds[kind[0]]}), (M, cap, seen)
        ok = tgt >= 0
        ct = torch.gather(z, 1, tgt.long().clamp(0, V - 1)[:, None])[:, 0]
        # the span fed to the exponential: max - min with a running maximum, max |c| without; the larger covers both
        span = torch.maximum(zmax - zmin, z.abs().max(-1).values)
        c.ref[cap] = SimpleNamespace(amax=amax, nll_self=lse - zmax, ok=ok, bound=lse_bound(lse, span, cap, True),
                                     nll_tgt=torch.where(ok, lse - ct, torch.zeros(M, dtype=F64)))
    return c


def run_head_lens(impl, dev, M: int) -> GReport:
    """The fused vocab head at caps 30 and 0 -- ``nxt`` the lowest index among the maxima of the capped
    ``rn_bf16(exact)`` logits, NLLs within ``lse_bound``, exactly 0 without a target -- and the lens epilogue."""
    rep = GReport()
    c = head_case(M)
    A, W, tgt = c.A.to(dev), c.W.to(dev), c.tgt.to(dev)
    for cap in HEAD_CAPS:
        r = c.ref[cap]
        nxt, ns, nt = Out(dev, M, 1, torch.int32), _f32(dev, M, 1), _f32(dev, M, 1)
        impl.head(A, W, cap, tgt, nxt.c.view(M), ns.c.view(M), nt.c.view(M))
        check_out(rep, f"head nxt: M {M} cap {cap:g}", nxt, r.amax.to(torch.int32).to(dev)[:, None])
        check_bound(rep, f"head nll_self: M {M} cap {cap:g}", ns.got().reshape(M), r.nll_self, r.bound)
        gt = nt.got().reshape(M).cpu().double()
        check_bound(rep, f"head nll_tgt: M {M} cap {cap:g}", gt[r.ok], r.nll_tgt[r.ok], r.bound[r.ok])
        if not bool((gt[~r.ok] == 0).all()):
            rep.fail(f"head nll_tgt: M {M} cap {cap:g}: not exactly 0 on a row without a target")
        if not (ns.guard_ok() and nt.guard_ok()):
            rep.fail(f"head NLLs: M {M} cap {cap:g}: a guard cell outside the output was written")
        rep.count("rows with a planted tie", sum(k < 4 for k in c.kind))
    lg, lse = _bf(dev, M, HEAD_V), _f32(dev, M, 1)
    impl.lens(A, W, lg.c, lse.c.view(M))
    check_out(rep, f"lens logits: M {M}", lg, c.Ebf.to(dev))
    l64, bound = lens_want(c.Ebf)
    check_bound(rep, f"lens lse: M {M}", lse.got().reshape(M), l64, bound)
    if not lse.guard_ok():
        rep.fail(f"lens lse: M {M}: a guard cell outside the output was written")
    return rep


# ---- dispatch --------------------------------------------------------------------------------------------------------
DISPATCH_SHAPE = (777, 512, 192)
DISPATCH_CHOICES = ("g256", "g128", "gs", "k256", "k128")
# the ring GEMM needs K % 128 == 0, which 192 is not: its choice strings run at the nearest K that is
DISPATCH_RING_K, DISPATCH_RING = 256, ("r64x64", "r128x128b")
DISPATCH_SPLIT = ((0, 512, 256), (512, 777, 128))          # a forced "gs" row split: (r0, r1, tile rows)


def run_dispatch(impl, dev) -> GReport:
    """``tb_gemm`` under every forced choice against one expectation; then each launch of a two-launch row split alone
    on a fresh output, whose rows outside the launch's slice are its guard rows."""
    rep = GReport()
    M, N, K = DISPATCH_SHAPE
    for choices, k in ((DISPATCH_CHOICES, K), (DISPATCH_RING, DISPATCH_RING_K)):
        c = case("wide", M, N, k)
        A, W, want = c.A.to(dev), c.W.to(dev), c.Ebf.to(dev)
        for ch in choices:
            out = _bf(dev, M, N)
            impl.tb_gemm(A, W, out.c, None, None, 0, ch)
            check_out(rep, f"tb_gemm {ch}: M {M} N {N} K {k}", out, want)
    c = case("wide", M, N, K)
    A, W, want = c.A.to(dev), c.W.to(dev), c.Ebf.to(dev)
    for r0, r1, tile in DISPATCH_SPLIT:
        out = _bf(dev, M, N)
        out.ibuf[:M] = SENT16
        impl.run_rows(A, W, out.c, 0, r0, r1, tile)
        w = torch.full_like(want, 0).view(torch.int16).fill_(SENT16).view(BF)
        w[r0:r1] = want[r0:r1]
        check_out(rep, f"row split [{r0}, {r1}) tile {tile}", out, w)
    return rep


# ---- the secondary criterion: uniform operands -----------------------------------------------------------------------
UNI_KS = (64, 192, 320)
UNI_RING_KS = (128, 256)                        # the ring GEMM needs K % 128 == 0
UNI_M, UNI_N = 257, 256
UNI_RING = ((64, 64, 0), (128, 128, 1), (32, 32, 2))      # variant 2 of this tile takes K % 256 == 0


@functools.lru_cache(maxsize=None)
def uniform_case(K: int) -> SimpleNamespace:
    g = torch.Generator().manual_seed(4242 + K)
    A = (torch.rand(UNI_M, K, generator=g) * 2 - 1).to(BF)
    W = (torch.rand(UNI_N, K, generator=g) * 2 - 1).to(BF)
    E, S = exact(A, W), A.double().abs() @ W.double().abs().t()
    u = K * 2.0 ** -23
    b32 = u / (1 - u) * S
    return SimpleNamespace(A=A, W=W, E=E, b32=b32, b16=b32 + 2.0 ** -8 * (E.abs() + b32))


def run_uniform(impl, dev, K: int) -> GReport:
    """Uniform (-1, 1) bf16 operands.  fp32 store: ``|C - E64| <= gamma S`` with ``gamma = K 2^-23 / (1 - K 2^-23)``,
    ``S = sum |a_k| |w_k|`` -- K exact products and at most K additions, each off by at most one ulp (2^-23 relative,
    which covers a truncating adder) of a partial sum no larger than S.  bf16 store: that plus half a bf16 step of the
    fp32 value, at most ``2^-8 (|E64| + gamma S)``."""
    rep = GReport()
    c = uniform_case(K)
    A, W = c.A.to(dev), c.W.to(dev)
    M, N = UNI_M, UNI_N
    if K % 64 == 0 and K not in UNI_RING_KS:
        for tile in (256, 128):
            o32, o16 = _f32(dev, M, N), _bf(dev, M, N)
            impl.gemm4(A, W, o32.c, None, None, 1, tile, None)
            impl.gemm4(A, W, o16.c, None, None, 0, tile, None)
            check_bound(rep, f"gemm4 fp32: K {K} tile {tile}", o32.got(), c.E, c.b32)
            check_bound(rep, f"gemm4 bf16: K {K} tile {tile}", o16.got(), c.E, c.b16)
        o32, o16 = _f32(dev, M, N), _bf(dev, M, N)
        impl.gemm_nt(A, W, o32.c, None, None, 1)
        impl.gemm_nt(A, W, o16.c, None, None, 0)
        check_bound(rep, f"gemm_nt fp32: K {K}", o32.got(), c.E, c.b32)
        check_bound(rep, f"gemm_nt bf16: K {K}", o16.got(), c.E, c.b16)
    if K in UNI_RING_KS:
        for bm, bn, var in UNI_RING:
            assert impl.ring_ok(M, N, K, 0, bm, bn, var) or (var == 2 and K % 256)
            if not impl.ring_ok(M, N, K, 0, bm, bn, var):
                continue
            o16 = _bf(dev, M, N)
            impl.gemm_ring(A, W, o16.c, 0, bm, bn, var, None)
            check_bound(rep, f"ring bf16: K {K} tile {bm}x{bn} variant {var}", o16.got(), c.E, c.b16)
    return rep


# ---- the width of the accumulation -----------------------------------------------------------------------------------
WIDTH_SHAPE = (129, 256, 1024)                  # K 127^2 = 16 516 096 < 2^24


def run_width(impl, dev) -> GReport:
    """Class ``tall``: positive integers 64 .. 127 at K = 1024.  Every output lies in [2^22, 2^24) -- most of them past
    2^23, where the last bit of an fp32 significand is the units bit -- and half of them are odd, so an accumulator with
    fewer than 24 significant bits anywhere along the chain cannot return them all.  This is what the exactness of the
    other classes (sums of 10 to 18 bits) assumes of the bf16 MFMA, asked directly: the fp32 store and the split-K
    planes of gemm4, the fp32 store of ``gemm_nt``, and the bf16 stores (ring included) as the single rounding of the
    exact value."""
    rep = GReport()
    M, N, K = WIDTH_SHAPE
    c = case("tall", M, N, K)
    assert s_max(c) < 2 ** 24 and float(c.E.min()) >= 2.0 ** 22
    rep.count("outputs of 2^23 or more", int((c.E >= 2.0 ** 23).sum()))
    rep.count("odd outputs", int((torch.remainder(c.E, 2) == 1).sum()))
    A, W, want32, want16 = c.A.to(dev), c.W.to(dev), c.E.float().to(dev), c.Ebf.to(dev)
    inner = run_gemm4(impl, dev, K, [("tall", M, N)], epis=(0, 1, 2))
    rep.failures += inner.failures
    for k, v in inner.used.items():
        rep.use(k, v)
    for epi, want in ((0, want16), (1, want32)):
        out = (_bf if epi == 0 else _f32)(dev, M, N)
        impl.gemm_nt(A, W, out.c, None, None, epi)
        check_out(rep, f"gemm_nt epi {epi}: tall", out, want)
    for bm, bn, var in UNI_RING:
        out = _bf(dev, M, N)
        impl.gemm_ring(A, W, out.c, 0, bm, bn, var, None)
        check_out(rep, f"ring epi 0: tall tile {bm}x{bn} variant {var}", out, want16)
    P = split_prefix("tall", M, N, K)
    for tile in SPLIT_TILES:
        used, kc = split_count(K, 4)
        ws = Out(dev, used * M, N, F32)
        assert int(impl.splitk_part(A, W, ws.c.view(-1), tile, 4)) == used
        lo = torch.arange(used) * kc
        planes = (P[lo + kc] - P[lo]).float().reshape(used * M, N)
        check_out(rep, f"split-K planes: tall tile {tile}", ws, planes.to(dev))
        ws, out = Out(dev, used * M, N, F32), _bf(dev, M, N)
        impl.splitk(A, W, out.c, ws.c.view(-1), 0, tile, 4)
        check_out(rep, f"split-K reduced epi 0: tall tile {tile}", out, want16)
    return rep


# ---- the reference implementation and its mutants --------------------------------------------------------------------
class RefImpl:
    """The callables a runner needs, computed in float64 on the CPU -- and, with one keyword set, with one planted
    defect:

    ``gemm4(A, W, C, bias, thr, epi, tile, a2)``, ``gemm_ring(A, W, C, epi, bm, bn, var, a2)``, ``gemm_nt(A, W, C, bias,
    thr, epi)``, ``splitk_part(A, W, ws, tile, ks) -> splits``, ``splitk(A, W, C, ws, epi, tile, ks)``, ``splitk_ks(M,
    N, K, tile)``, ``qkv_rope(family, tile, A, W, pos, slot, cos, sin, q, kc, vc, Hq, Hkv, a2)``, ``lora_t(x, a_all, t,
    adapter, nsr, nr, r, bm, bn, part)``, ``lens(x, W, logits, lse)``, ``head(x, W, cap, tgt, nxt, nll_self, nll_tgt)``,
    ``tb_gemm(A, W, out, bias, thr, epi, choice)``, ``run_rows(A, W, out, epi, r0, r1, tile)``, ``ring_tiles(epi)``,
    ``ring_ok(M, N, K, epi, bm, bn, var)``, ``lora_t_ok(M, N, K, bm, bn)``, ``set_pipe(on) -> previous``.

    Defects: ``drop_term`` one k term of one element; ``drop_last_ktile`` the last 64-deep K tile for the rows of a
    ragged last row tile; ``swap_chunks`` two 16-byte K chunks swapped in A only; ``shift_col`` the output shifted one
    column inside a 16-column block; ``transpose4`` a 4 x 4 accumulator sub-block transposed; ``pack`` ``"trunc"`` /
    ``"away"``; ``jump_ge``; ``stale_grid = G``: with G persistent workgroups, tile ``t >= G`` starts from tile
    ``t - G``'s accumulators; ``double_ktile`` a split starts one K tile early; ``guard_write`` one write behind the
    output; ``tie_high`` the highest index among the maxima; ``acc_bits = b``: accumulators of ``b`` significant bits
    (modelled as one rounding of the finished sum)."""

    def __init__(self, drop_term=False, drop_last_ktile=False, swap_chunks=False, shift_col=False, transpose4=False,
                 pack="rn", jump_ge=False, stale_grid=0, double_ktile=False, guard_write=False, tie_high=False,
                 acc_bits=0):
        self.acc_bits = acc_bits
        self.drop_term, self.drop_last_ktile, self.swap_chunks = drop_term, drop_last_ktile, swap_chunks
        self.shift_col, self.transpose4, self.pack, self.jump_ge = shift_col, transpose4, pack, jump_ge
        self.stale_grid, self.double_ktile, self.guard_write = stale_grid, double_ktile, guard_write
        self.tie_high = tie_high
        self.pipe = 1

    # -- the accumulators
    def _acc(self, A, W, a2=None, bm=128, k_lo=0, k_hi=None) -> torch.Tensor:
        X = A.reshape(-1, A.shape[-1]) if a2 is None else torch.cat([A, a2], 1)
        X, Wd = X.double(), W.double()
        M, K = X.shape
        N = Wd.shape[0]
        k_hi = K if k_hi is None else k_hi
        if self.swap_chunks and K >= 16:
            X = X.clone()
            X[:, 0:8], X[:, 8:16] = X[:, 8:16].clone(), X[:, 0:8].clone()
        acc = X[:, k_lo:k_hi] @ Wd[:, k_lo:k_hi].t()
        if self.drop_term:
            m, n, k = M // 2, N // 3, K - 1
            if k_lo <= k < k_hi:
                acc[m, n] -= X[m, k] * Wd[n, k]
        if self.drop_last_ktile and M % bm and k_hi == K:
            r0 = (M // bm) * bm
            acc[r0:] -= X[r0:, K - 64:] @ Wd[:, K - 64:].t()
        if self.shift_col and N >= 16:
            acc[:, :16] = acc[:, :16].roll(-1, 1)
        if self.transpose4 and M >= 4 and N >= 4:
            acc[:4, :4] = acc[:4, :4].t().clone()
        if self.stale_grid:
            G, nbn = self.stale_grid, N // 256
            pad = torch.zeros(-(-M // 256) * 256, N, dtype=F64)
            pad[:M] = acc
            t4 = pad.view(-1, 256, nbn, 256).permute(0, 2, 1, 3).reshape(-1, 256, 256)     # [tile, 256, 256]
            for t in range(G, t4.shape[0]):
                t4[t] += t4[t - G]
            acc = t4.view(-1, nbn, 256, 256).permute(0, 2, 1, 3).reshape(-1, N)[:M].contiguous()
        if self.acc_bits:
            m, e = torch.frexp(acc)
            acc = torch.ldexp(torch.round(torch.ldexp(m, torch.tensor(self.acc_bits))), e - self.acc_bits)
        return acc

    def _pack(self, x: torch.Tensor) -> torch.Tensor:
        return {"rn": rn_bf16, "trunc": pack_trunc, "away": pack_away}[self.pack](x)

    def _store(self, C: torch.Tensor, val: torch.Tensor) -> None:
        C.copy_(val.reshape(C.shape))
        if self.guard_write:
            torch.as_strided(C, (1,), (1,), C.storage_offset() + C.numel()).fill_(1.0)

    def _epi(self, acc, epi, bias=None, thr=None):
        if epi == 0:
            return self._pack(acc)
        if epi == 1:
            return acc.float()
        if epi == 2:
            pre = acc + (0 if bias is None else bias.double())
            th = torch.zeros(()) if thr is None else thr.double()
            return torch.where(pre >= th if self.jump_ge else pre > th, pre, torch.zeros_like(pre)).float()
        F = acc.shape[1] // 2
        return ref.geglu(self._pack(acc[:, torch.argsort(interleave(F))]))

    # -- the kernels
    def gemm4(self, A, W, C, bias, thr, epi, tile, a2=None):
        self._store(C, self._epi(self._acc(A, W, a2, tile), epi, bias, thr))

    def gemm_ring(self, A, W, C, epi, bm, bn, var, a2=None):
        assert self.ring_ok(A.shape[0], W.shape[0], W.shape[1], epi, bm, bn, var)
        self._store(C, self._epi(self._acc(A, W, a2, bm), epi))

    def gemm_nt(self, A, W, C, bias, thr, epi):
        self._store(C, self._epi(self._acc(A, W, None, 128), epi, bias, thr))

    def splitk_ks(self, M, N, K, tile):
        nwg, NT = (N // 256) * -(-M // tile), K // 64
        return split_count(K, max(1, min(256 // max(nwg, 1), NT // 4)))[0]

    def splitk_part(self, A, W, ws, tile, ks):
        M, N, K = A.shape[0], W.shape[0], W.shape[1]
        used, kc = split_count(K, ks)
        for s in range(used):
            lo = s * kc * 64 - (64 if self.double_ktile and s > 0 else 0)
            plane = self._acc(A, W, None, tile, lo, min((s + 1) * kc * 64, K))
            ws[s * M * N: (s + 1) * M * N] = plane.float().reshape(-1)
        return used

    def splitk(self, A, W, C, ws, epi, tile, ks):
        M, N = A.shape[0], W.shape[0]
        used = self.splitk_part(A, W, ws, tile, ks)
        self._store(C, self._epi(ws[: used * M * N].view(used, M, N).double().sum(0), epi))

    def qkv_rope(self, family, tile, A, W, pos, slot, cos, sin, q, kc, vc, Hq, Hkv, a2=None):
        bm = tile if family == "g4" else tile[0]
        qkv = self._pack(self._acc(A, W, a2, bm))
        self._store(q, ref.rope_qkv_cache(qkv, pos, slot, cos, sin, kc, vc, Hq, Hkv, HD))

    def lora_t(self, x, a_all, t, adapter, nsr, nr, r, bm, bn, part):
        N = a_all.shape[0]
        v = self._pack(self._acc(x, a_all, None, bm))
        col = torch.arange(N)
        keep = (col[None] < nsr) & (((col % nr) // r)[None] == adapter.long()[:, None]) & (adapter[:, None] >= 0)
        t[:, :N] = torch.where(keep, v, torch.zeros_like(v))

    def lens(self, x, W, logits, lse):
        lg = self._pack(self._acc(x, W, None, 256))
        self._store(logits, lg)
        lse.copy_(torch.logsumexp(lg.float(), -1))

    def head(self, x, W, cap, tgt, nxt, nll_self, nll_tgt):
        c = ref._capped(self._pack(self._acc(x, W, None, 256)), cap, True)
        V = c.shape[-1]
        a = (V - 1 - torch.argmax(c.flip(-1), -1)) if self.tie_high else torch.argmax(c, -1)
        lse = torch.logsumexp(c, -1)
        nxt.copy_(a.to(torch.int32))
        nll_self.copy_(lse - c.max(-1).values)
        ct = torch.gather(c, 1, tgt.long().clamp(0, V - 1)[:, None])[:, 0]
        nll_tgt.copy_(torch.where(tgt >= 0, lse - ct, torch.zeros_like(ct)))

    def tb_gemm(self, A, W, out, bias, thr, epi, choice):
        self.gemm4(A, W, out, bias, thr, epi, 128 if choice.endswith("128") else 256)

    def run_rows(self, A, W, out, epi, r0, r1, tile):
        self.gemm4(A[r0:r1], W, out[r0:r1], None, None, epi, tile)

    # -- what the launchers say about themselves
    def ring_tiles(self, epi):
        return list(RING_PLAIN + RING_N112 if epi == 0 else RING_PAIR)

    def ring_ok(self, M, N, K, epi, bm, bn, var):
        return (bm, bn, var) in ring_admitted(epi, N, K)

    def lora_t_ok(self, M, N, K, bm, bn):
        return (bm, bn) in LORA_TILES and N % bn == 0 and K >= 128 and K % 128 == 0

    def set_pipe(self, on):
        old, self.pipe = self.pipe, int(on)
        return old
