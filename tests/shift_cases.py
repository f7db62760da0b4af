"""Criterion, seeded inputs and the case runner for the output-shift readout ``ops.head_shift`` (csrc/lens.hip
head_shift_kernel): tests/test_head_shift_cpu.py holds ops/reference.py and deliberately wrong stand-ins to it,
tests/test_head_shift_gpu.py the HIP kernel.  Same pattern as tests/readout_cases.py, whose ``Report``, ``lse_bound``,
``capped64``, ``hazard_columns`` and ``STREAM_WIDTHS`` are used as they are.  Everything here runs on the CPU; the
runner takes the implementation as a function ``head_shift(logits, base, rowmap, cap, kl=None, kl_rev=None)`` and the
device to put the inputs on.

Truth.  For an edited row ``z`` and its baseline row ``y`` the capped logits ``q = c(z)``, ``p = c(y)`` are bf16 values
that ``ref.softcap_bf16`` produces exactly, so in float64 ::

    kl     = KL(base || edit) = sum_v P_v (p_v - q_v) - (lse p - lse q),   P = softmax p
    kl_rev = KL(edit || base) = sum_v Q_v (q_v - p_v) + (lse p - lse q),   Q = softmax q

is the true value to about 1e-13.

Criterion (``shift_bound``; derived here, not measured).  An implementation in fp32 computes ``A / S_p - (ln S_p - ln
S_q)`` with ``S_p = sum e^p``, ``S_q = sum e^q``, ``A = sum e^p (p - q)`` (the kernel literally; the reference the same
quantities scaled by ``e^-lse``).

* ``ln S_p`` and ``ln S_q`` are log-sum-exps of a fixed-offset sum, each within ``lse_bound(lse, span)`` of its truth
  with ``span = max |c|`` (readout_cases.lse_bound: the exponential's relative error ``2^-24 (2 + span)``, the
  accumulation, the logarithm's rounding at ``|lse|``; its 4x margin on the ``|lse|`` term also covers the rounding of
  the difference of the two logarithms, one more ``2^-24 max |lse|``).  Together: ``lse_bound_p + lse_bound_q`` -- the
  ``2 lse_bound`` of the design.
* ``A / S_p``.  Write ``T = sum_v P_v |p_v - q_v|``.  Every term ``e^{p_v} (p_v - q_v)`` carries the exponential's
  relative error ``e_x = 2^-24 (2 + span)`` (the product ``x log2 e`` rounds at ``2^-24 |x|`` of the result,
  ``v_exp_f32`` adds up to two ulp), the difference's rounding ``2^-24`` (exact when the two bf16 values are within
  2^16 of each other) and the product's ``2^-24``; adding the terms up adds ``n 2^-24`` of ``sum |term|`` for an
  accumulation ``n`` additions deep.  So ``|A^ - A| <= S_p T (e_x + (n + 2) 2^-24)``.  ``S_p`` (all terms positive) is off
  by a relative ``e_x + n 2^-24``, the quotient rounds once more, and ``|A / S_p| <= T``: ::

      |A^/S^ - A/S| <= T 2^-24 (2 (2 + span) + 2 n + 3)  =  T 2^-24 (2 span + 2 n + 7)        to first order.

  The depth ``n``: a lane of the kernel adds ``4 ceil(V / 4096)`` packed pairs (8 logits of each of its
  ``ceil(V / 4096)`` vectors, two lanes of a packed add), folds the two halves, adds at most one tail column, then 6
  butterfly steps and 7 waves: ``n(V) = 4 ceil(V / 4096) + 15``.  The bound uses ``eps(V, span) = 2^-22 (span + n(V) +
  4)``: twice the first-order value, for the second-order terms.  (torch's pairwise fp32 sums are shallower than
  ``n(V)`` at these widths; its ``exp(p - lse)`` feeds the exponential at most ``span + |lse|``, covered by the
  factor 2 while ``|lse| <= span + n(V)``, which holds for every case here.)

  shift_bound = lse_bound(lse_p, span_p) + lse_bound(lse_q, span_q) + eps(V, span) T,      span = max(span_p, span_q)

with ``T`` taken under ``P`` for ``kl`` and under ``Q`` for ``kl_rev``.  Rows of identical bits must give exactly 0.0
twice (every term of ``A`` is zero and the two sums run in the same order), and so must a row whose ``rowmap`` entry
lies outside ``[0, Rb)``.  Nothing is clamped, so a result may be a tiny negative number inside the bound.

Cases (``shift_case``): ``Rb = 2`` baseline rows, ``R`` in {1, 3, 5} edited rows through the rowmaps ``ROWMAPS[R]``
(R = 5: a reversed order, -1, an index past the table, a repeat), per kind of row pair:

* ``identical``: the edited row is its baseline row (rows with no valid baseline are random);
* ``one_entry``: the edited row is its baseline row with one logit raised to the row maximum plus 2, at a hazard
  column of the stream (the last column, i.e. the ``V % 8`` tail where there is one, first);
* ``negation``: the baseline row is ``100 randn`` (mostly saturated), the edited row its negation -- the largest
  ``|p - q|`` everywhere and the worst cancellation between ``A / S_p`` and the log difference;
* ``gain1`` / ``gain16``: independent ``g randn`` rows.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Sequence

import torch

from readout_cases import BF, NAN, STREAM_WIDTHS, Report, capped64, hazard_columns, lse_bound  # noqa: F401
from taboo_brittleness_amd.ops import reference as ref

SHIFT_CAPS = (30.0, 40.0)
SHIFT_RB = 2
# R -> rowmap into the 2 baseline rows: a non-zero single index; out of range + reversed; reversed, -1, past the table
# and a repeat
ROWMAPS = {1: (1,), 3: (1, 2, 0), 5: (1, -1, 0, 2, 1)}
KINDS = ("identical", "one_entry", "negation", "gain1", "gain16")


def depth(V: int) -> int:
    """Additions on the longest chain of the kernel's per-row sums (see the module docstring)."""
    return 4 * math.ceil(V / 4096) + 15


def eps(V: int, span: torch.Tensor) -> torch.Tensor:
    return 2.0 ** -22 * (span + depth(V) + 4.0)


def shift_truth(z: torch.Tensor, y: torch.Tensor, cap: float) -> Dict[str, torch.Tensor]:
    """float64 truth and bounds for edited rows ``z [R, V]`` against baseline rows ``y [R, V]`` (bf16, already
    gathered): ``kl``, ``kl_rev``, ``bound``, ``bound_rev``, ``T``, ``T_rev``."""
    q, p = capped64(z, cap, True), capped64(y, cap, True)
    lq, lp = torch.logsumexp(q, -1), torch.logsumexp(p, -1)
    P, Q = torch.exp(p - lp[:, None]), torch.exp(q - lq[:, None])
    d = p - q
    T, Tr = (P * d.abs()).sum(-1), (Q * d.abs()).sum(-1)
    sp, sq = p.abs().max(-1).values, q.abs().max(-1).values
    lb = lse_bound(lp, sp, cap, True) + lse_bound(lq, sq, cap, True)
    e = eps(z.shape[-1], torch.maximum(sp, sq))
    return {"kl": (P * d).sum(-1) - (lp - lq), "kl_rev": (lp - lq) - (Q * d).sum(-1), "bound": lb + e * T,
            "bound_rev": lb + e * Tr, "T": T, "T_rev": Tr}


@functools.lru_cache(maxsize=None)
def shift_case(V: int, kind: str, R: int):
    """``(logits [R, V] bf16, base [2, V] bf16, rowmap [R] int32, labels)``, seeded; shared by the tests, not to be
    written to."""
    g = torch.Generator().manual_seed(31000 + 7 * V + 100003 * KINDS.index(kind) + R)
    rm = ROWMAPS[R]
    gain = {"negation": 100.0, "gain16": 16.0, "gain1": 1.0}.get(kind, 4.0)
    base = (gain * torch.randn(SHIFT_RB, V, generator=g)).to(BF)
    logits = (gain * torch.randn(R, V, generator=g)).to(BF)
    hz = hazard_columns(V)
    labels = []
    for r, b in enumerate(rm):
        if not 0 <= b < SHIFT_RB:
            labels.append(f"{kind} unmapped({b})")
            continue
        if kind == "identical":
            logits[r] = base[b]
        elif kind == "one_entry":
            h = hz[-1 - (r % len(hz))]                 # row 0: the last column
            logits[r] = base[b]
            logits[r, h] = (base[b].float().max() + 2).to(BF)
            labels.append(f"one_entry@{h} base {b}")
            continue
        elif kind == "negation":
            logits[r] = -base[b]
        labels.append(f"{kind} base {b}")
    return logits, base, torch.tensor(rm, dtype=torch.int32), tuple(labels)


@functools.lru_cache(maxsize=None)
def case_truth(V: int, kind: str, R: int, cap: float):
    """:func:`shift_truth` of a case's mapped rows (unmapped rows against baseline row 0; they must give 0 anyway),
    plus ``ok`` (the row has a baseline) and ``same`` (its bits equal its baseline's)."""
    z, y, rm, _ = shift_case(V, kind, R)
    ok = (rm >= 0) & (rm < SHIFT_RB)
    yy = y[rm.long().clamp(0, SHIFT_RB - 1)]
    t = shift_truth(z, yy, cap)
    t["ok"] = ok
    t["same"] = ok & (z.view(torch.int16) == yy.view(torch.int16)).all(-1)
    return t


def check_shift(rep: Report, what: str, got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor, exact0: torch.Tensor,
                labels: Sequence[str]) -> None:
    got = got.detach().cpu().reshape(-1).double()
    for r in range(got.numel()):
        if bool(exact0[r]):
            if not float(got[r]) == 0.0:
                rep.fail(f"{what} row {r} ({labels[r]}): got {float(got[r])!r}, want exactly 0")
            continue
        f = float((got[r] - want[r]).abs() / bound[r])
        if not f <= 1.0:                                   # NaN fails
            rep.fail(f"{what} row {r} ({labels[r]}): got {float(got[r])!r}, want {float(want[r])!r} +- "
                     f"{float(bound[r]):.3e} ({f:.3g} of the bound)")
        else:
            rep.use(what.split(" V ")[0], f)


def run_shift(head_shift, dev, V: int, caps: Sequence[float] = SHIFT_CAPS, kinds: Sequence[str] = KINDS,
              Rs: Sequence[int] = (1, 3, 5), fill: bool = True) -> Report:
    """``head_shift`` on every case of width ``V``.  ``fill``: hand it NaN-filled outputs, so that an element it does
    not write shows."""
    rep = Report()
    for kind in kinds:
        for R in Rs:
            z, y, rm, labels = shift_case(V, kind, R)
            gz, gy, gm = z.to(dev), y.to(dev), rm.to(dev)
            for cap in caps:
                t = case_truth(V, kind, R, cap)
                outs = {"kl": torch.full((R,), NAN, device=dev), "kl_rev": torch.full((R,), NAN, device=dev)} if fill else {}
                kl, klr = head_shift(gz, gy, gm, cap, **outs)
                tag = f"{kind} V {V} R {R} cap {cap:g}"
                zero = ~t["ok"] | t["same"]
                check_shift(rep, f"kl {tag}", kl, t["kl"], t["bound"], zero, labels)
                check_shift(rep, f"kl_rev {tag}", klr, t["kl_rev"], t["bound_rev"], zero, labels)
    return rep


# ---- deliberately wrong stand-ins -----------------------------------------------------------------------------
def shift_mutant(drop_tail: bool = False, swap_sum: bool = False, ignore_map: bool = False):
    """The reference in fp32 with one planted bug: ``drop_tail`` leaves the ``V % 8`` tail columns out of every sum;
    ``swap_sum`` normalises ``A`` by ``sum e^q`` where ``sum e^p`` belongs (and takes that sum's logarithm);
    ``ignore_map`` compares row ``r`` with baseline row ``r % Rb`` whatever the rowmap says."""

    def head_shift(logits, base, rowmap, cap, kl=None, kl_rev=None):
        R, V = logits.shape
        Rb = base.shape[0]
        rm = rowmap.long()
        if ignore_map:
            rm = torch.arange(R) % Rb
        ok = (rm >= 0) & (rm < Rb)
        q = ref._capped(logits, cap, True)
        p = ref._capped(base, cap, True)[rm.clamp(0, Rb - 1)]
        if drop_tail:
            q, p = q[:, : (V >> 3) * 8], p[:, : (V >> 3) * 8]
        if q.shape[1] == 0:
            a = b = torch.zeros(R)
        else:
            lq = torch.logsumexp(q, -1)
            lp = lq if swap_sum else torch.logsumexp(p, -1)
            d = p - q
            a = (torch.exp(p - lp[:, None]) * d).sum(-1) - (lp - lq)
            b = (lp - lq) - (torch.exp(q - lq[:, None]) * d).sum(-1)
        a, b = torch.where(ok, a, torch.zeros_like(a)), torch.where(ok, b, torch.zeros_like(b))
        if kl is not None:
            kl.copy_(a)
            kl_rev.copy_(b)
            return kl, kl_rev
        return a, b

    return head_shift
