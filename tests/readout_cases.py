"""Criteria, seeded inputs and case runners for the vocabulary readouts of csrc/lens.hip (tests/test_readouts_cpu.py
and tests/test_readouts_gpu.py).  Everything here runs on the CPU; a runner takes the implementation under test as an
object with the functions of ``taboo_brittleness_amd.ops`` (``argmax_rows``, ``row_lse``, ``xent_rows``,
``decode_head``, ``decode_head_stats``, ``gather_probs``, ``lens_colsum``, ``topk_rows``) and the device to put the
inputs on, so the same cases hold the HIP kernels (``ops`` on the GPU), ops/reference.py (``reference_impl`` on the
CPU) and deliberately wrong stand-ins (``stream_mutant`` and friends) to the same criteria.

All references are float64.  Under ``emulate_bf16=True`` the capped logits ``c(z)`` are bf16 values, which
``ref.softcap_bf16`` produces exactly, so their float64 log-sum-exp is the true value.

Criteria (each derived where it is defined, none measured):

* integer outputs -- greedy tokens, top-k indices -- are exact: the lowest index among the maxima of ``c(z)``, the
  stable descending order for a top-k (values bit-equal);
* ``lse_bound``: a log-sum-exp or an NLL within ``2^-20 (4 + span) + 2^-22 |lse|`` of the float64 value;
* ``prob_window``: a probability ``exp(z - lse)`` within a relative ``2^-20 (4 + |z - lse|)`` of float64, or, rounded,
  a bf16 value between the rounded ends of that interval;
* ``colsum_window``: a column sum between the sums of its terms' window ends, plus the fp32 accumulation error.

A runner returns a :class:`Report`: the list of violated criteria (empty for a correct implementation) and, per
output, the largest error seen as a fraction of its bound.  The builders return CPU tensors, seeded per case and
cached: the tests share them and must not write to them.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from rounding_cases import bf16_ulps, in_window, rn_bf16
from taboo_brittleness_amd import ops as _ops
from taboo_brittleness_amd.ops import reference as ref

BF = torch.bfloat16
F64 = torch.float64
NAN = float("nan")

CAPS = (30.0, 50.0, 0.0)                       # Gemma-2's final cap, its attention cap (no table kernel), none
FIXED_CAP_MAX = 40.0                           # csrc/lens.hip DH_FIXED_CAP: decode_head sums exp(c) with no running max

# V >> 3 = 0, 0, 1, 1, 511, 512, 513, 2047, 2048, 2049, 4099: both sides of one trip of the 512-thread stream and of one
# trip of its 4-deep unrolled form, with and without a V % 8 tail; the odd widths misalign every row but the first
STREAM_WIDTHS = (1, 7, 8, 9, 4095, 4096, 4104, 16376, 16384, 16397, 32795)


class Report:
    """What a runner found: ``failures`` (one line per violated criterion) and ``used`` (output name -> the largest
    error seen as a fraction of its bound; for exact outputs the number of mismatches)."""

    def __init__(self) -> None:
        self.failures: List[str] = []
        self.used: Dict[str, float] = {}

    def fail(self, msg: str) -> None:
        self.failures.append(msg)

    def use(self, key: str, frac: float) -> None:
        self.used[key] = max(self.used.get(key, 0.0), float(frac))

    def failed(self, *words: str) -> bool:
        """Whether a failure line contains all of ``words``."""
        return any(all(w in f for w in words) for f in self.failures)

    def assert_ok(self, what: str) -> None:
        for k in sorted(self.used):
            counted = k.endswith("mismatches") or k.endswith("RN(p64)")
            print(f"{what}: {k}: " + (f"{int(self.used[k])}" if counted else f"{self.used[k]:.4f} of the bound"))
        assert not self.failures, f"{what}: {len(self.failures)} criteria violated:\n" + "\n".join(self.failures[:20])


def _cpu(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu()


# ---- criteria ---------------------------------------------------------------------------------------------------
def lse_bound(lse64: torch.Tensor, span: torch.Tensor, cap: float = 0.0, emulate: bool = True) -> torch.Tensor:
    """Largest accepted ``|got - lse64|`` for a log-sum-exp (or an NLL) of one row: ``2^-20 (4 + span) + 2^-22
    |lse64|``, plus ``cap 2^-20`` where the cap runs through the fp32 ``fast_tanh`` (``emulate`` False, ``cap > 0``).

    ``span`` is the largest ``|x|`` the kernel feeds to its exponential: ``max c - min c`` for the kernels that keep a
    running maximum, ``max |c|`` for decode_head_f_kernel, which sums ``exp(c)`` as it is.  ``__expf(x)`` is
    ``v_exp_f32`` of the fp32 product ``x log2 e``: the product's rounding is a relative ``2^-24 |x|`` of the result,
    the instruction adds an ulp or two; the per-thread fp32 sums at these widths (at most 64 terms per thread, 9 merge
    levels) add at most ``64 * 2^-24`` relative; all relative errors of the sum become absolute errors of its
    logarithm.  The final ``M + log S`` rounds once at ``|lse|``.  That is about ``2^-24 (6 + span) + 2^-24 |lse|``;
    the bound carries 16x over the first part and 4x over the second, and is still 15-75x below the ``atol`` of 1e-3
    it replaces (27x on a ``4 randn`` row under cap 30).  An NLL ``lse - c[t]`` gets the same bound: ``c[t]`` is exact under ``emulate``, and the subtraction
    rounds at ``|nll| <= span + |lse|``.  Without ``emulate``, ``fast_tanh`` is ``1 - 2 / (e^{2y} + 1)`` with a few fp32
    ulp of 1 in error, which ``cap`` scales: every ``c`` moves by at most a few ``cap 2^-24``, and so do lse and NLL."""
    b = 2.0 ** -20 * (4.0 + span) + 2.0 ** -22 * lse64.abs()
    if cap > 0 and not emulate:
        b = b + cap * 2.0 ** -20
    return b


_D_SAT = 128.0


def prob_window(z: torch.Tensor, lse32: torch.Tensor, round_bf16: bool):
    """``(lo, hi, p64, err)`` for ``p = exp(z - lse)``: with ``d = fl32(z - lse32)`` -- the subtraction the kernel and
    the reference both do, exact operands -- ``p64 = exp(d)`` in float64 and ``e = 2^-20 (4 + min(|d|, 128))``, accept
    ``p64 (1 - e) - 2^-120 <= got <= p64 (1 + e) + 2^-120`` (``err = p64 e + 2^-120``).  ``__expf(d)`` rounds ``d log2
    e`` (relative ``2^-24 |d|`` of the result) and ``v_exp_f32`` adds an ulp or two: ``e`` carries 16x over that.  Past
    ``|d| = 128`` the result is below 2^-184 and flushed; the ``2^-120`` covers flushed subnormals.  With ``round_bf16``
    ``lo`` / ``hi`` are the bf16 values ``RN(..)`` of those ends (one rounding of the float64 value), and ``got`` must
    be a bf16 value between them; otherwise they are float64."""
    assert z.dtype == torch.float32 and lse32.dtype == torch.float32
    d = (z - lse32).double()
    p = torch.exp(d)
    e = 2.0 ** -20 * (4.0 + d.abs().clamp(max=_D_SAT))
    lo, hi = p * (1.0 - e) - 2.0 ** -120, p * (1.0 + e) + 2.0 ** -120
    if round_bf16:
        lo, hi = rn_bf16(lo), rn_bf16(hi)
    return lo, hi, p, p * e + 2.0 ** -120


def _inside(got: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, round_bf16: bool) -> torch.Tensor:
    """Elementwise: fp32 ``got`` inside a :func:`prob_window`; with ``round_bf16`` it must also be a bf16 value."""
    if round_bf16:
        gb = got.to(BF)
        return (gb.float() == got) & in_window(gb, lo, hi)
    gd = got.double()
    return (gd >= lo) & (gd <= hi)


def check_ints(rep: Report, what: str, got: torch.Tensor, want: torch.Tensor, labels: Sequence[str]) -> None:
    got, want = _cpu(got).reshape(-1).long(), want.reshape(-1).long()
    bad = (got != want).nonzero().reshape(-1).tolist()
    rep.use(what + " mismatches", len(bad))
    for r in bad:
        rep.fail(f"{what} row {r} ({labels[r]}): got {int(got[r])}, want {int(want[r])}")


def check_exact(rep: Report, what: str, got: torch.Tensor, want: torch.Tensor, labels: Sequence[str]) -> None:
    """fp32 values that must equal ``want`` (float64 holding fp32 values, possibly -inf) exactly."""
    got, want = _cpu(got).reshape(-1).double(), want.reshape(-1)
    bad = (~(got == want)).nonzero().reshape(-1).tolist()
    rep.use(what + " mismatches", len(bad))
    for r in bad:
        rep.fail(f"{what} row {r} ({labels[r]}): got {float(got[r])!r}, want exactly {float(want[r])!r}")


def check_lse(rep: Report, what: str, got: torch.Tensor, want64: torch.Tensor, bound: torch.Tensor,
              labels: Sequence[str], exact0: Optional[torch.Tensor] = None) -> None:
    """``|got - want64| <= bound`` per row; rows flagged in ``exact0`` must be exactly 0 instead."""
    got = _cpu(got).reshape(-1).double()
    frac = (got - want64).abs() / bound
    for r in range(got.numel()):
        if exact0 is not None and bool(exact0[r]):
            if not float(got[r]) == 0.0:
                rep.fail(f"{what} row {r} ({labels[r]}): got {float(got[r])!r}, want exactly 0")
            continue
        f = float(frac[r])
        if not f <= 1.0:                                  # NaN fails
            rep.fail(f"{what} row {r} ({labels[r]}): got {float(got[r])!r}, want {float(want64[r])!r} +- "
                     f"{float(bound[r]):.3e} ({f:.3g} of the bound)")
        else:
            rep.use(what, f)


def check_probs(rep: Report, what: str, got: torch.Tensor, z: torch.Tensor, lse32: torch.Tensor, ok: torch.Tensor,
                round_bf16: bool) -> None:
    """``got [R, K]`` against :func:`prob_window` of the gathered logits ``z [R, K]`` and ``lse32 [R]``; where ``ok``
    is False (an id outside ``[0, V)``) exactly 0."""
    got = _cpu(got).float()
    lo, hi, p, err = prob_window(z, lse32.reshape(-1, 1), round_bf16)
    good = torch.where(ok, _inside(got, lo, hi, round_bf16), got == 0)
    for r, k in (~good).nonzero().tolist():
        rep.fail(f"{what} [{r}, {k}]: got {float(got[r, k])!r}, " + (
            f"want in [{float(lo[r, k])!r}, {float(hi[r, k])!r}]" + (" as a bf16 value" if round_bf16 else "")
            if bool(ok[r, k]) else "want exactly 0 (id out of range)"))
    sel = ok & good
    if bool(sel.any()):
        if round_bf16:
            rep.use(what + " bf16 steps off RN(p64)", int(bf16_ulps(got.to(BF), rn_bf16(p))[sel].max()))
        else:
            rep.use(what, float(((got.double() - p).abs() / err)[sel].max()))


def term_windows(z: torch.Tensor, lse32: torch.Tensor, excl: torch.Tensor, mask: Optional[torch.Tensor],
                 round_bf16: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(LO, HI) [R, V]`` float64: :func:`prob_window` of every element of the bf16 rows ``z``, exactly 0 at a row's
    excluded ids and on masked rows."""
    R, V = z.shape
    lo, hi, _p, _e = prob_window(z.float(), lse32.reshape(R, 1), round_bf16)
    lo, hi = lo.double(), hi.double()
    for r in range(R):
        for e in excl[r].tolist():
            if 0 <= e < V:
                lo[r, e] = hi[r, e] = 0.0
        if mask is not None and not int(mask[r]):
            lo[r] = 0.0
            hi[r] = 0.0
    return lo, hi


def colsum_window(LO: torch.Tensor, HI: torch.Tensor, rows: Sequence[int], start: Optional[torch.Tensor]):
    """``(lo, hi) [V]`` for the sum of the term windows over ``rows`` onto ``start [V]``: ``[sum LO + start - delta,
    sum HI + start + delta]`` with ``delta = n_rows 2^-24 (sum HI + |start|)``: the kernel adds the rows one after the
    other in fp32, each add rounding at no more than the final magnitude (the terms are not negative)."""
    V = LO.shape[1]
    s = torch.zeros(V, dtype=F64) if start is None else start.double()
    idx = torch.tensor(list(rows), dtype=torch.long)
    lo, hi = LO[idx].sum(0), HI[idx].sum(0)
    delta = len(rows) * 2.0 ** -24 * (hi + s.abs())
    return lo + s - delta, hi + s + delta


def check_colsum(rep: Report, what: str, got: torch.Tensor, LO: torch.Tensor, HI: torch.Tensor,
                 rows: Sequence[int], start: Optional[torch.Tensor]) -> None:
    """One ``[V]`` result against :func:`colsum_window`; over no rows it must equal the start (or 0) exactly.  The
    fraction recorded is the distance from the window's centre over its half-width.  It reaches 1 legitimately: with
    one row onto a start the half-width is one fp32 rounding of the sum, and with ``round_bf16`` a term's window is
    often two neighbouring bf16 values, of which the result is one."""
    got = _cpu(got).double()
    lo, hi = colsum_window(LO, HI, rows, start)
    if not rows:
        lo = hi = torch.zeros_like(got) if start is None else start.double()
    bad = ~((got >= lo) & (got <= hi))
    if bool(bad.any()):
        v = int(bad.nonzero()[0])
        rep.fail(f"{what}: {int(bad.sum())} columns outside the window, first column {v}: got {float(got[v])!r}, "
                 f"want in [{float(lo[v])!r}, {float(hi[v])!r}]")
    elif rows:
        mid, half = (lo + hi) / 2, (hi - lo) / 2
        sel = half > 0
        if bool(sel.any()):
            rep.use(what.split(":")[0], float(((got - mid).abs() / half)[sel].max()))


def check_bits(rep: Report, what: str, a: torch.Tensor, b: torch.Tensor) -> None:
    a, b = _cpu(a).contiguous().view(torch.int32), _cpu(b).contiguous().view(torch.int32)
    if not torch.equal(a, b):
        rep.fail(f"{what}: {int((a != b).sum())} of {a.numel()} values differ in their bits")


# ---- streamed row kernels ---------------------------------------------------------------------------------------
def hazard_columns(V: int) -> List[int]:
    """The columns of a ``V``-wide row next to a boundary of the stream: the first vector's ends, the first column of
    the next, both sides of the 512- and the 2048-vector trip, the last vector column, the first tail column and the
    last column -- those that exist."""
    nv = V >> 3
    c = {0, 7, 8, 8 * 511, 8 * 512, 8 * 2047, 8 * 2048, 8 * nv - 1, 8 * nv, V - 1}
    return sorted(x for x in c if 0 <= x < V)


def boundary_vectors(V: int) -> List[int]:
    """The 16-B vectors (8 columns each) of a row that sit at a trip boundary of the stream, those that exist."""
    nv = V >> 3
    return sorted({j for j in (0, 511, 512, 2047, 2048, nv - 1) if 0 <= j < nv})


@functools.lru_cache(maxsize=None)
def stream_rows(V: int):
    """``(z [R, V] bf16, labels, tie_col)``: two ``random`` rows (``4 randn``); one ``planted@h`` row per hazard column
    ``h`` holding the row maximum plus 2 (over half of the row's mass at the narrow widths; at the widest, where the
    ``4 randn`` tail is heavy and the cap compresses the top, still 19 %, so leaving it out moves the lse by 0.2 or
    more, thousands of times the bound); ``sat_tie``: 300, 200 and 250 at the three highest
    hazard columns and 225 at a lower column that is no hazard (``tie_col``, where one exists), all of which cap to the
    same value at cap 30 and 50, so the lowest index must win, while without a cap the 300 does; ``sat_neg``: every
    logit in [-300, -200], so every capped value is ``-cap``; ``equal``: every logit 1.5 (lse = c + ln V; a rounding
    error would be systematic); ``far_neg``: every logit -100; ``lens``: one logit at +300, the others -300."""
    g = torch.Generator().manual_seed(77000 + V)
    hz = hazard_columns(V)
    rows, labels = [], []

    def rnd():
        return 4 * torch.randn(V, generator=g)

    for _ in range(2):
        rows.append(rnd())
        labels.append("random")
    for h in hz:
        x = rnd()
        x[h] = x.max() + 2
        rows.append(x)
        labels.append(f"planted@{h}")
    x = rnd()
    members = hz[-3:]
    low = [c for c in range(min(members) // 2, -1, -1) if c not in hz][:1]
    for c, v in zip(members, (300.0, 200.0, 250.0)):
        x[c] = v
    for c in low:
        x[c] = 225.0
    rows.append(x)
    labels.append("sat_tie")
    rows.append(-(200 + 100 * torch.rand(V, generator=g)))
    labels.append("sat_neg")
    rows.append(torch.full((V,), 1.5))
    labels.append("equal")
    rows.append(torch.full((V,), -100.0))
    labels.append("far_neg")
    x = torch.full((V,), -300.0)
    x[hz[-2] if len(hz) > 1 else 0] = 300.0
    rows.append(x)
    labels.append("lens")
    return torch.stack(rows).to(BF), tuple(labels), (low[0] if low else members[0])


def capped64(z: torch.Tensor, cap: float, emulate: bool) -> torch.Tensor:
    """The capped logits of bf16 ``z`` in float64: exact bf16 values under ``emulate``, ``cap tanh(z / cap)`` in
    float64 otherwise."""
    if not cap > 0:
        return z.double()
    return ref.softcap_bf16(z.float(), cap).double() if emulate else torch.tanh(z.double() / cap) * cap


def row_reference(z: torch.Tensor, cap: float, emulate: bool) -> Dict[str, torch.Tensor]:
    """float64 reference of bf16 rows: ``c`` capped logits, ``lse``, ``cmax``, ``amax`` (numpy's argmax: the first of
    the maxima), ``span_online = max c - min c`` and ``span_fixed = max |c|``."""
    c = capped64(z, cap, emulate)
    cmax, cmin = c.max(-1).values, c.min(-1).values
    return {"c": c, "lse": torch.logsumexp(c, -1), "cmax": cmax,
            "amax": torch.from_numpy(np.argmax(c.numpy(), axis=-1)).long(),
            "span_online": cmax - cmin, "span_fixed": c.abs().max(-1).values}


@functools.lru_cache(maxsize=None)
def stream_ref(V: int, cap: float, emulate: bool) -> Dict[str, torch.Tensor]:
    return row_reference(stream_rows(V)[0], cap, emulate)


@functools.lru_cache(maxsize=None)
def stream_targets(V: int, cap: float, j: int) -> torch.Tensor:
    """Target ids, one per row: row ``r`` takes kind ``(r + 3 j) % 7`` of -1, V, 0, V - 1, a tail column (the first,
    or V - 1 without a tail), the ``sat_tie`` row's lowest member and the row's own argmax; on pass 0 the ``sat_tie``
    row gets its lowest member."""
    _z, labels, tie = stream_rows(V)
    am = stream_ref(V, cap, True)["amax"]
    nv8 = (V >> 3) * 8
    t = []
    for r, lab in enumerate(labels):
        kinds = (-1, V, 0, V - 1, nv8 if nv8 < V else V - 1, tie, int(am[r]))
        t.append(tie if (lab == "sat_tie" and j == 0) else kinds[(r + 3 * j) % 7])
    return torch.tensor(t, dtype=torch.int32)


STATS_OFF = 5000


def _f32(fill: bool, dev, *shape) -> Dict[str, torch.Tensor]:
    """``out=`` of an fp32 result: NaN-filled with ``fill``, so that an element the kernel does not write shows (the
    allocator may hand back a block that still holds the previous call's correct values); nothing otherwise."""
    return {"out": torch.full(shape, NAN, device=dev)} if fill else {}


def _head_outs(fill: bool, dev, R: int) -> Dict[str, torch.Tensor]:
    if not fill:
        return {}
    return {"nxt": torch.full((R,), -7, dtype=torch.int32, device=dev), "nll_self": torch.full((R,), NAN, device=dev),
            "nll_tgt": torch.full((R,), NAN, device=dev)}


def _check_head(rep, tag, impl, g, dev, z_ref, tgt, cap, labels, stats_off: Optional[int], fill: bool = False):
    """decode_head (and, with ``stats_off`` and a cap the fixed-offset kernel takes, decode_head_stats) on the device
    rows ``g`` against the float64 row reference ``z_ref`` with teacher targets ``tgt``.  Returns decode_head's
    ``nll_tgt``."""
    V = g.shape[-1]
    R = g.shape[0]
    fixed = 0 < cap <= FIXED_CAP_MAX
    bound = lse_bound(z_ref["lse"], z_ref["span_fixed" if fixed else "span_online"], cap, True)
    ok = (tgt >= 0) & (tgt < V)
    ct = torch.gather(z_ref["c"], 1, tgt.long().clamp(0, V - 1)[:, None])[:, 0]
    nxt, ns, nt = impl.decode_head(g, cap, tgt.to(dev), **_head_outs(fill, dev, R))
    check_ints(rep, f"decode_head nxt {tag}", nxt, z_ref["amax"], labels)
    check_lse(rep, f"decode_head nll_self {tag}", ns, z_ref["lse"] - z_ref["cmax"], bound, labels)
    check_lse(rep, f"decode_head nll_tgt {tag}", nt, z_ref["lse"] - ct, bound, labels, exact0=~ok)
    if stats_off is None or not fixed:
        return nt
    # global targets: local -1 alternates between -1 and an id just below this slice, local V lies beyond it
    tg = torch.where(tgt < 0, torch.where(torch.arange(tgt.numel()) % 2 == 0, -1, stats_off - 1), tgt + stats_off)
    st = impl.decode_head_stats(g, tg.to(torch.int32).to(dev), stats_off, cap, **_f32(fill, dev, R, 4))
    if st is None:
        rep.fail(f"decode_head_stats {tag}: returned None")
        return nt
    st = _cpu(st)
    check_lse(rep, f"decode_head_stats lse {tag}", st[:, 0], z_ref["lse"], bound, labels)
    check_exact(rep, f"decode_head_stats best {tag}", st[:, 1], z_ref["cmax"], labels)
    check_exact(rep, f"decode_head_stats id {tag}", st[:, 2], (z_ref["amax"] + stats_off).double(), labels)
    check_exact(rep, f"decode_head_stats target {tag}", st[:, 3],
                torch.where(ok, ct, torch.full_like(ct, -math.inf)), labels)
    return nt


def run_stream(impl, dev, V: int, caps: Sequence[float] = CAPS, fill: bool = False, bits: bool = False) -> Report:
    """argmax_rows, row_lse and xent_rows (``emulate_bf16`` both ways), decode_head and decode_head_stats on
    :func:`stream_rows` at every cap.  ``fill``: hand every call sentinel-filled outputs (``ops`` only).  ``bits``
    (``ops`` only; the reference sums in another order): also the identities that hold because the kernels share one
    row pass -- under ``emulate_bf16`` (and either way at cap 0) xent_rows is row_lse minus the capped target logit
    (the bf16 value itself at cap 0, ``ops.softcap_values`` otherwise) and exactly 0 for a target out of range, and
    where decode_head keeps a running maximum (no cap, or one above ``FIXED_CAP_MAX``) its ``nll_tgt`` is that
    xent_rows; all bit for bit."""
    rep = Report()
    z, labels, _tie = stream_rows(V)
    g = z.to(dev)
    R = z.shape[0]
    for cap in caps:
        r1 = stream_ref(V, cap, True)
        ao = {"out": torch.full((R,), -7, dtype=torch.int32, device=dev)} if fill else {}
        check_ints(rep, f"argmax_rows cap {cap:g}", impl.argmax_rows(g, cap, **ao), r1["amax"], labels)
        xent_emu = {}
        for emu in (True, False):
            rr = stream_ref(V, cap, emu)
            tag = f"cap {cap:g} emulate {int(emu)}"
            bound = lse_bound(rr["lse"], rr["span_online"], cap, emu)
            lse = impl.row_lse(g, cap, emu, **_f32(fill, dev, R))
            check_lse(rep, f"row_lse {tag}", lse, rr["lse"], bound, labels)
            for j in (0, 1):
                tgt = stream_targets(V, cap, j)
                ok = (tgt >= 0) & (tgt < V)
                ct = torch.gather(rr["c"], 1, tgt.long().clamp(0, V - 1)[:, None])[:, 0]
                x = impl.xent_rows(g, tgt.to(dev), cap, emu, **_f32(fill, dev, R))
                check_lse(rep, f"xent_rows {tag}", x, rr["lse"] - ct, bound, labels, exact0=~ok)
                if emu:
                    xent_emu[j] = x
                if bits and (emu or not cap > 0):
                    zt = torch.gather(g, 1, tgt.long().clamp(0, V - 1)[:, None].to(dev))[:, 0]
                    want = torch.where(ok, _cpu(lse) - _cpu(_ops.softcap_values(zt, cap)), torch.zeros(R))
                    check_bits(rep, f"xent_rows {tag} target pass {j}: row_lse minus the capped target logit", x, want)
        for j in (0, 1):
            nt = _check_head(rep, f"cap {cap:g}", impl, g, dev, r1, stream_targets(V, cap, j), cap, labels,
                             STATS_OFF if j == 0 else None, fill)
            if bits and not 0 < cap <= FIXED_CAP_MAX:
                check_bits(rep, f"decode_head nll_tgt cap {cap:g} target pass {j}: xent_rows emulate 1", nt,
                           xent_emu[j])
    return rep


# ---- decode_head over more rows than workgroups -------------------------------------------------------------------
PERSIST_V = 4109
PERSIST_CAP = 30.0


@functools.lru_cache(maxsize=None)
def persist_case(R: int):
    """``(z [R, 4109] bf16, labels, tgt, tgt_global, off)``: every row a different ``4 randn`` draw, every 7th with a
    planted maximum at a hazard column in turn, every 11th a saturated tie; local targets in ``[-1, V]``; for the
    stats pass ``off`` = 1000 and global targets below it, inside ``[off, off + V)`` and beyond."""
    V = PERSIST_V
    g = torch.Generator().manual_seed(4109 + R)
    hz = hazard_columns(V)
    z = 4 * torch.randn(R, V, generator=g)
    labels = []
    for r in range(R):
        lab = "random"
        if r % 7 == 3:
            h = hz[(r // 7) % len(hz)]
            z[r, h] = z[r].max() + 2
            lab = f"planted@{h}"
        if r % 11 == 5:
            a, b = hz[(r // 11) % len(hz)], 1 + (37 * r) % (V - 1)
            z[r, a] = 200.0
            z[r, b] = 300.0
            lab = f"sat_tie@{min(a, b)}"
        labels.append(lab)
    tgt = torch.randint(-1, V + 1, (R,), generator=g, dtype=torch.int32)
    off = 1000
    tg = torch.randint(0, off + V + 500, (R,), generator=g, dtype=torch.int32)
    tg[::9] = -1
    return z.to(BF), tuple(labels), tgt, tg, off


def run_persist(impl, dev, R: int, fill: bool = False) -> Report:
    """decode_head and decode_head_stats over ``R`` rows of V = 4109 at cap 30: with ``R`` above the grid of the
    persistent kernel, rows that share a workgroup are each held to the float64 reference."""
    rep = Report()
    z, labels, tgt, tg, off = persist_case(R)
    V, cap = PERSIST_V, PERSIST_CAP
    rr = row_reference(z, cap, True)
    g = z.to(dev)
    _check_head(rep, f"R {R}", impl, g, dev, rr, tgt, cap, labels, None, fill)
    st = impl.decode_head_stats(g, tg.to(dev), off, cap, **_f32(fill, dev, R, 4))
    if st is None:
        rep.fail("decode_head_stats: returned None")
        return rep
    st = _cpu(st)
    bound = lse_bound(rr["lse"], rr["span_fixed"], cap, True)
    tl = tg.long() - off
    ok = (tg >= 0) & (tl >= 0) & (tl < V)
    ct = torch.gather(rr["c"], 1, tl.clamp(0, V - 1)[:, None])[:, 0]
    assert int(ok.sum()) > 0 and int((tl < 0).sum()) > 0 and int((tl >= V).sum()) > 0
    check_lse(rep, f"decode_head_stats lse R {R}", st[:, 0], rr["lse"], bound, labels)
    check_exact(rep, f"decode_head_stats best R {R}", st[:, 1], rr["cmax"], labels)
    check_exact(rep, f"decode_head_stats id R {R}", st[:, 2], (rr["amax"] + off).double(), labels)
    check_exact(rep, f"decode_head_stats target R {R}", st[:, 3], torch.where(ok, ct, torch.full_like(ct, -math.inf)),
                labels)
    return rep


# ---- gather_probs -------------------------------------------------------------------------------------------------
GATHER_WIDTHS = (9, 3000, 32795)
GATHER_ROWMAP = (3, 0, 0, 4, 1)                # repeated and permuted rows; row 2 is never read


@functools.lru_cache(maxsize=None)
def gather_case(V: int):
    """``(z [5, V] bf16, lse32 [5], ids [5, 4])``: ``4 randn`` rows, row r with one logit at 36 + 2 r (p within e^-8
    of 1, and no two rows share an lse); ``lse32`` the float64 log-sum-exp rounded to fp32, which the implementation
    under test is fed, so that the criterion isolates this kernel; ids: -1 or V, the row's maximum, one random id
    twice -- on row 2 the maximum twice, V and -1."""
    g = torch.Generator().manual_seed(99000 + V)
    R = 5
    z = 4 * torch.randn(R, V, generator=g)
    top = [0, V - 1, V // 2, 8 * (V // 8) - 1, 7 % V]
    ids = torch.empty(R, 4, dtype=torch.int32)
    for r in range(R):
        z[r, top[r]] = 36.0 + 2 * r
        c = int(torch.randint(0, V, (1,), generator=g))
        ids[r] = torch.tensor([-1 if r % 2 == 0 else V, top[r], c, c])
    ids[2] = torch.tensor([top[2], top[2], V, -1])
    z = z.to(BF)
    return z, torch.logsumexp(z.double(), -1).float(), ids


def run_gather(impl, dev, V: int, fill: bool = False) -> Report:
    rep = Report()
    z, lse, ids = gather_case(V)
    g, l, i = z.to(dev), lse.to(dev), ids.to(dev)
    ok = (ids >= 0) & (ids < V)
    rm = torch.tensor(GATHER_ROWMAP, dtype=torch.int32)
    for rb in (False, True):
        zz = torch.gather(z.float(), 1, ids.long().clamp(0, V - 1))
        check_probs(rep, f"gather_probs round_bf16 {int(rb)}",
                    impl.gather_probs(g, l, i, round_bf16=rb, **_f32(fill, dev, 5, 4)), zz, lse, ok, rb)
        zm = torch.gather(z.float()[rm.long()], 1, ids.long().clamp(0, V - 1))
        check_probs(rep, f"gather_probs rowmap round_bf16 {int(rb)}",
                    impl.gather_probs(g, l, i, round_bf16=rb, rowmap=rm.to(dev), **_f32(fill, dev, 5, 4)), zm,
                    lse[rm.long()], ok, rb)
    return rep


# ---- lens_colsum --------------------------------------------------------------------------------------------------
# a workgroup covers 256 groups of 8 columns: one group, a partial group, two, both sides of a block, a partial group
# in a second block, and odd widths (misaligned float4 / 16-B accesses on every row but the first)
COLSUM_WIDTHS = (1, 7, 8, 9, 2047, 2048, 2049, 2055, 4099)
COLSUM_B, COLSUM_T = 3, 4
COLSUM_MASK = (0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)      # a skipped first row, a skipped last row, all skipped
COLSUM_ROWMAP = (3, 0, 0, 4, 1, 1, 2, 2, 4, 3, 0, 1)
COLSUM_OFFS = ((0, 0, 6, 12), (0, 6, 6, 12), (0, 6, 12, 12))


@functools.lru_cache(maxsize=None)
def colsum_case(V: int):
    """``(z [12, V] bf16, lse32, excl [12, 2], pc, start [3, V])``.  Rows are ``randn`` with one planted logit
    ``ceil(ln 40 V) + 1`` at column ``pc[r]``, which holds over 90 % of the row's mass; rows 2k and 2k + 1 share
    the column, taken in turn from V - 1 (the partial last group where V % 8 != 0), 0 (a full group from V = 8 on),
    the first column of the last group, 7, 2047, 2048, 8 and the last column of the last full group.  Row 2k
    excludes its planted column -- as (pc, pc), (pc, other), (V, pc), (pc, -1) in turn -- and row 2k + 1 does not:
    it excludes (-1, V) or (other, -1), ``other`` a neighbouring column of ordinary mass."""
    g = torch.Generator().manual_seed(88000 + V)
    R = COLSUM_B * COLSUM_T
    hz = []
    for c in (V - 1, 0, 8 * (V // 8), 7, 2047, 2048, 8, 8 * (V // 8) - 1):
        if 0 <= c < V and c not in hz:
            hz.append(c)
    z = torch.randn(R, V, generator=g)
    pc = [hz[(r // 2) % len(hz)] for r in range(R)]
    big = math.ceil(math.log(40 * V)) + 1.0
    excl = torch.empty(R, 2, dtype=torch.int32)
    for r in range(R):
        z[r, pc[r]] = big
        other = (pc[r] + 1) % V
        if r % 2 == 0:
            excl[r] = torch.tensor(((pc[r], pc[r]), (pc[r], other), (V, pc[r]), (pc[r], -1))[(r // 2) % 4])
        else:
            excl[r] = torch.tensor(((-1, V), (other, -1))[(r // 2) % 2])
    z = z.to(BF)
    lse = torch.logsumexp(z.double(), -1)
    p = torch.exp(z.double()[torch.arange(R), pc] - lse)
    assert float(p.min()) > 0.9
    return z, lse.float(), excl, tuple(pc), torch.randn(COLSUM_B, V, generator=g)


def run_colsum(impl, dev, V: int, rb: bool, bits: bool) -> Report:
    """Dense (masked, overwriting a NaN-filled ``acc`` and accumulating onto a start, with ``cum``), packed with empty
    sequences, and through a ``rowmap``, all against :func:`colsum_window`; with ``bits`` also the identities that
    hold because the kernel adds row by row (the reference sums in another order)."""
    rep = Report()
    B, T = COLSUM_B, COLSUM_T
    z, lse, excl, pc, start = colsum_case(V)
    g, l, e = z.to(dev), lse.to(dev), excl.to(dev)
    mask = torch.tensor(COLSUM_MASK, dtype=torch.uint8)
    tag = f"round_bf16 {int(rb)}"

    def nan(*shape):
        return torch.full(shape, NAN, device=dev)

    # dense, masked: overwrite, then accumulate
    LO, HI = term_windows(z, lse, excl, mask, rb)
    for accum in (False, True):
        s0 = start if accum else None
        acc, cum = (start.to(dev).clone() if accum else nan(B, V)), nan(B, T + 1, V)
        out = impl.lens_colsum(g, l, mask.to(dev), e, B, T, acc=acc, accumulate=accum, round_bf16=rb, cum=cum)
        what = f"lens_colsum dense accumulate {int(accum)} {tag}"
        for b in range(B):
            sb = None if s0 is None else s0[b]
            live = [r for r in range(b * T, b * T + T) if COLSUM_MASK[r]]
            check_colsum(rep, f"{what}: acc[{b}]", out[b], LO, HI, live if live else [], sb)
            for t in range(T + 1):
                rows = [r for r in range(b * T, b * T + t) if COLSUM_MASK[r]]
                check_colsum(rep, f"{what}: cum[{b}, {t}]", cum[b, t], LO, HI, rows, sb)
        if bits:
            check_bits(rep, f"{what}: cum[:, T] against acc", cum[:, T], out)
    # dense with every row live: the window, and the two launch identities
    ones = torch.ones(B * T, dtype=torch.uint8)
    LO1, HI1 = term_windows(z, lse, excl, None, rb)
    full = impl.lens_colsum(g, l, ones.to(dev), e, B, T, round_bf16=rb)
    for b in range(B):
        check_colsum(rep, f"lens_colsum dense all rows {tag}: acc[{b}]", full[b], LO1, HI1, range(b * T, b * T + T),
                     None)
    if bits:
        uni = torch.arange(0, B * T + 1, T, dtype=torch.int32)
        check_bits(rep, f"lens_colsum {tag}: packed uniform offs against dense all ones",
                   impl.lens_colsum(g, l, None, e, B, T, round_bf16=rb, offs=uni.to(dev)), full)
        m1 = torch.tensor([1, 0, 0, 0] * B, dtype=torch.uint8)
        two = impl.lens_colsum(g, l, m1.to(dev), e, B, T, acc=nan(B, V), accumulate=False, round_bf16=rb)
        two = impl.lens_colsum(g, l, (1 - m1).to(dev), e, B, T, acc=two, accumulate=True, round_bf16=rb)
        check_bits(rep, f"lens_colsum {tag}: two launches against one", two, full)
    # packed, with an empty first / middle / last sequence
    for offs in COLSUM_OFFS:
        o = torch.tensor(offs, dtype=torch.int32).to(dev)
        for accum in (False, True):
            acc = start.to(dev).clone() if accum else nan(B, V)
            out = impl.lens_colsum(g, l, None, e, B, 0, acc=acc, accumulate=accum, round_bf16=rb, offs=o)
            for b in range(B):
                check_colsum(rep, f"lens_colsum packed {offs} accumulate {int(accum)} {tag}: acc[{b}]", out[b], LO1,
                             HI1, range(offs[b], offs[b + 1]), start[b] if accum else None)
    # packed through a rowmap over the first five rows; logical row r excludes its physical row's planted column
    rm = torch.tensor(COLSUM_ROWMAP, dtype=torch.int32)
    exm = torch.tensor([(pc[p], -1) if r % 2 == 0 else (-1, V) for r, p in enumerate(COLSUM_ROWMAP)], dtype=torch.int32)
    zm, lm = z[rm.long()], lse[rm.long()]
    LOm, HIm = term_windows(zm, lm, exm, None, rb)
    offs = (0, 5, 5, 12)
    o = torch.tensor(offs, dtype=torch.int32).to(dev)
    out = impl.lens_colsum(g[:5].contiguous(), l[:5].contiguous(), None, exm.to(dev), B, 0, round_bf16=rb, offs=o,
                           rowmap=rm.to(dev))
    for b in range(B):
        check_colsum(rep, f"lens_colsum rowmap {tag}: acc[{b}]", out[b], LOm, HIm, range(offs[b], offs[b + 1]), None)
    if bits:
        check_bits(rep, f"lens_colsum {tag}: rowmap against materialised rows", out,
                   impl.lens_colsum(zm.to(dev), lm.to(dev), None, exm.to(dev), B, 0, round_bf16=rb, offs=o))
    return rep


# ---- topk_rows ----------------------------------------------------------------------------------------------------
TOPK_WIDTHS = (64, 4096, 4097, 4100)           # one chunk; the widest single chunk; chunked unaligned / aligned
TOPK_KS = (1, 8, 9, 16, 17, 64)                # both ends of the 8-, 16- and 64-entry candidate lists
TOPK_LABELS = ("random", "ties", "constant", "few_finite", "one_chunk", "chunk_edges")


@functools.lru_cache(maxsize=None)
def topk_case(V: int, K: int) -> torch.Tensor:
    """``x [6, V]`` fp32 (fewer than 512 rows, so a row wider than 4096 is split into 2048-column chunks): a
    ``randn`` row; one quantised to quarters (many ties inside the best K); a constant row (indices 0 .. K - 1); a
    row with K // 2 finite values (the -inf entries follow in index order); the K best at consecutive columns inside
    one chunk; the best of the row at the chunk edges (both sides of every multiple of the chunk length ``ceil(V / C)``
    rounded up to 4, of 2048 and of 4096, and the row's ends), one each."""
    g = torch.Generator().manual_seed(55000 + 100 * V + K)
    x = torch.randn(6, V, generator=g)
    x[1] = (x[1] * 4).round() / 4
    x[2] = 0.75
    keep = torch.randperm(V, generator=g)[: K // 2]
    fin = x[3, keep].clone()
    x[3] = -math.inf
    x[3, keep] = fin
    c0 = min(1368 + 5, V - K)
    x[4, c0:c0 + K] = 100 + torch.randn(K, generator=g)
    C = 1 if V <= 4096 else (V + 2047) // 2048
    CH = (((V + C - 1) // C) + 3) & ~3
    edges = sorted({c for m in (CH, 2048, 4096) for k in range(0, V // m + 2) for c in (k * m - 1, k * m)
                    if 0 <= c < V} | {0, V - 1})
    for i, c in enumerate(edges[:K]):
        x[5, c] = 50.0 + i
    return x


def topk_expected(x: torch.Tensor, K: int):
    """``(vals, idx)`` of the stable descending order (numpy's stable argsort of ``-x``)."""
    order = np.argsort(-x.numpy(), axis=-1, kind="stable")[:, :K]
    idx = torch.from_numpy(order.copy()).long()
    return torch.gather(x, 1, idx), idx.to(torch.int32)


def check_topk(rep: Report, what: str, vals: torch.Tensor, idx: torch.Tensor, x: torch.Tensor, K: int,
               labels: Sequence[str]) -> None:
    wv, wi = topk_expected(x, K)
    vals, idx = _cpu(vals), _cpu(idx)
    for r in range(x.shape[0]):
        if not torch.equal(idx[r].long(), wi[r].long()):
            k = int((idx[r].long() != wi[r].long()).nonzero()[0])
            rep.fail(f"{what} row {r} ({labels[r]}): index {k} is {int(idx[r, k])}, want {int(wi[r, k])}")
        elif not torch.equal(vals[r].view(torch.int32), wv[r].view(torch.int32)):
            rep.fail(f"{what} row {r} ({labels[r]}): values differ in their bits from x[idx]")


def run_topk(impl, dev, V: int, Ks: Sequence[int] = TOPK_KS) -> Report:
    rep = Report()
    for K in Ks:
        x = topk_case(V, K)
        vals, idx = impl.topk_rows(x.to(dev), K)
        check_topk(rep, f"topk_rows V {V} K {K}", vals, idx, x, K, TOPK_LABELS)
    return rep


@functools.lru_cache(maxsize=None)
def topk_all_case() -> torch.Tensor:
    """K == V at V = 5: a ``randn`` row, a constant row, a row with two -inf."""
    x = torch.randn(3, 5, generator=torch.Generator().manual_seed(5))
    x[1] = -2.0
    x[2, 1] = x[2, 3] = -math.inf
    return x


def run_topk_all(impl, dev) -> Report:
    rep = Report()
    x = topk_all_case()
    vals, idx = impl.topk_rows(x.to(dev), 5)
    check_topk(rep, "topk_rows K == V == 5", vals, idx, x, 5, ("random", "constant", "two_inf"))
    return rep


# ---- implementations ----------------------------------------------------------------------------------------------
def reference_stats(logits, tgt, off, cap, out=None):
    """decode_head_stats from ops/reference.py in fp32 (``ops.decode_head_stats`` has no CPU path)."""
    V = logits.shape[-1]
    c = ref._capped(logits, cap, True)
    t = tgt.long() - off
    ok = (tgt >= 0) & (t >= 0) & (t < V)
    ct = torch.gather(c, 1, t.clamp(0, V - 1)[:, None])[:, 0]
    st = torch.stack([ref.row_lse(logits, cap, True), c.max(-1).values, (ref.argmax_rows(logits, cap) + off).float(),
                      torch.where(ok, ct, torch.full_like(ct, -math.inf))], 1)
    return st if out is None else out.copy_(st)


def reference_impl() -> SimpleNamespace:
    """ops/reference.py in fp32, through the CPU dispatch of ``ops``."""
    return SimpleNamespace(argmax_rows=_ops.argmax_rows, row_lse=_ops.row_lse, xent_rows=_ops.xent_rows,
                           decode_head=_ops.decode_head, decode_head_stats=reference_stats,
                           gather_probs=_ops.gather_probs, lens_colsum=_ops.lens_colsum, topk_rows=_ops.topk_rows)


def stream_mutant(cap_tail: bool = True, drop_vec: Optional[int] = None, tie_high: bool = False,
                  neighbour_max: bool = False) -> SimpleNamespace:
    """The streamed readouts in fp32 with one planted bug: ``cap_tail`` False skips the softcap on the ``V % 8`` tail
    columns; ``drop_vec = j`` leaves the 8 columns of vector ``j`` out of every reduction; ``tie_high`` resolves an
    argmax tie to the highest index; ``neighbour_max`` computes ``lse = M + log sum exp(c - M)`` in fp32 with the
    maximum ``M`` of the row before (a stale per-row maximum).  With the defaults nothing is wrong."""

    def capped(lg, cap, emu):
        c = ref._capped(lg, cap, emu).clone()
        V = c.shape[-1]
        nv8 = (V >> 3) * 8
        if not cap_tail and cap > 0:
            c[:, nv8:] = lg.float()[:, nv8:]
        if drop_vec is not None and 8 * drop_vec + 8 <= nv8:
            c[:, 8 * drop_vec: 8 * drop_vec + 8] = -math.inf
        return c

    def lse_of(c):
        if neighbour_max:
            M = c.max(-1).values.roll(1)
            return M + torch.log(torch.exp(c - M[:, None]).sum(-1))
        return torch.logsumexp(c, -1)

    def amax_of(c):
        V = c.shape[-1]
        a = (V - 1 - torch.argmax(c.flip(-1), -1)) if tie_high else torch.argmax(c, -1)
        return a.to(torch.int32)

    def nll_of(c, tgt):
        V = c.shape[-1]
        t = tgt.long()
        ok = (t >= 0) & (t < V)
        ct = torch.gather(c, 1, t.clamp(0, V - 1)[:, None])[:, 0]
        return torch.where(ok, lse_of(c) - ct, torch.zeros_like(ct))

    def decode_head(lg, cap, tgt=None):
        c = capped(lg, cap, True)
        nxt = amax_of(c)
        return nxt, lse_of(c) - c.max(-1).values, None if tgt is None else nll_of(c, tgt)

    def decode_head_stats(lg, tgt, off, cap):
        c = capped(lg, cap, True)
        V = c.shape[-1]
        t = tgt.long() - off
        ok = (tgt >= 0) & (t >= 0) & (t < V)
        ct = torch.gather(c, 1, t.clamp(0, V - 1)[:, None])[:, 0]
        return torch.stack([lse_of(c), c.max(-1).values, (amax_of(c) + off).float(),
                            torch.where(ok, ct, torch.full_like(ct, -math.inf))], 1)

    return SimpleNamespace(
        argmax_rows=lambda lg, cap=0.0: amax_of(capped(lg, cap, True)),
        row_lse=lambda lg, cap=0.0, emulate_bf16=False: lse_of(capped(lg, cap, emulate_bf16)),
        xent_rows=lambda lg, tgt, cap=0.0, emulate_bf16=True: nll_of(capped(lg, cap, emulate_bf16), tgt),
        decode_head=decode_head, decode_head_stats=decode_head_stats)


def gather_mutant(force_round: Optional[bool] = None, neighbour_lse: bool = False) -> SimpleNamespace:
    """gather_probs of the reference with ``round_bf16`` forced to ``force_round`` whatever the caller passes, or,
    under a ``rowmap``, with the lse of the row after the mapped one."""

    def gather_probs(lg, lse, ids, round_bf16=False, rowmap=None):
        rb = round_bf16 if force_round is None else force_round
        if rowmap is not None and neighbour_lse:
            r = rowmap.long()
            return ref.gather_probs(lg[r], lse[(r + 1) % lse.numel()], ids, rb).view(ids.shape)
        return _ops.gather_probs(lg, lse, ids, round_bf16=rb, rowmap=rowmap)

    return SimpleNamespace(gather_probs=gather_probs)


def colsum_mutant(ignore_excl: Optional[int] = None, ignore_mask: bool = False, drop_start: bool = False,
                  force_round: Optional[bool] = None) -> SimpleNamespace:
    """lens_colsum of the reference with exclusion slot ``ignore_excl`` (0 or 1) ignored, the mask ignored, the start
    value dropped under ``accumulate``, or ``round_bf16`` forced."""

    def lens_colsum(lg, lse, mask, excl, B, T, acc=None, accumulate=False, round_bf16=False, offs=None, cum=None,
                    rowmap=None):
        if ignore_excl is not None:
            excl = excl.clone()
            excl[:, ignore_excl] = -1
        if ignore_mask:
            mask = None
        if drop_start:
            accumulate = False
        rb = round_bf16 if force_round is None else force_round
        return _ops.lens_colsum(lg, lse, mask, excl, B, T, acc=acc, accumulate=accumulate, round_bf16=rb, offs=offs,
                                cum=cum, rowmap=rowmap)

    return SimpleNamespace(lens_colsum=lens_colsum)


def topk_tie_high(x, k):
    """top-k with ties resolved towards the higher index."""
    V = x.shape[-1]
    vals, idx = ref.topk_rows(x.flip(-1), k)
    return vals, (V - 1 - idx).to(torch.int32)
