"""Criterion, seeded inputs, the case runner and the mutants for the output-movers readout ``ops.head_movers``
(csrc/lens.hip head_movers_kernel): tests/test_head_movers_cpu.py holds ops/reference.py and deliberately wrong
stand-ins to it, tests/test_head_movers_gpu.py the HIP kernel.  Same pattern as tests/shift_cases.py;
``readout_cases.Report``, ``capped64``, ``hazard_columns``, ``STREAM_WIDTHS`` and ``shift_cases.depth`` are used as they
are.  Everything here runs on the CPU; the runner takes the implementation as a function ``head_movers(logits, base,
rowmap, rows, cap, k, ids=None, **outs)`` and the device to put the inputs on.

Truth.  For an edited row ``z`` and its baseline row ``y`` the capped logits ``q = c(z)``, ``p = c(y)`` are bf16 values
that ``ref.softcap_bf16`` produces exactly, so the float64 softmaxes ``P``, ``Q`` and ``D = Q - P`` are true to about
1e-16 of ``P + Q``.

Criterion for values (``movers_eps``; derived here, not measured).  The kernel computes ``d^_v = fl(e^_q,v r^_q) -
fl(e^_p,v r^_p)`` with ``r^_p = fl(1 / S^_p)``, ``S^_p = sum e^_p`` in fp32.  Per probability:

* the exponential: ``e^_v = e^{p_v} (1 + a)``, ``|a| <= e_x = 2^-24 (2 + span)`` with ``span = max |c|`` over both rows
  (the product ``x log2 e`` rounds at ``2^-24 |x|`` of the result, ``v_exp_f32`` adds up to two ulp; shift_cases);
* the sum of positive terms: ``S^ = S (1 + s)``, ``|s| <= e_x + n(V) 2^-24`` for an accumulation ``n(V) =
  shift_cases.depth(V)`` additions deep (the kernel's pass 1 is head_shift_kernel's, statement for statement);
* the reciprocal and the product round once each: ``2^-24`` twice.

So ``|P^_v - P_v| <= P_v 2^-24 (2 (2 + span) + n + 2) = P_v 2^-24 (2 span + n + 6)`` to first order, the same for ``Q``,
and the difference rounds at ``2^-24 |Q^ - P^| <= 2^-24 (P + Q)``: ::

    |d^_v - D_v| <= (P_v + Q_v) 2^-24 (2 span + n + 7)                                   to first order.

The bound is ``eps_v = delta(V, span) (P_v + Q_v) + 2^-124`` with ``delta = 2^-22 (span + n(V) + 4)``: at least twice
the first-order factor (``2^-24 (4 span + 4 n + 16)``), for the second-order terms.  The absolute term is the
kernel's own and is not in the relative model: under a cap of 40 a saturated row has ``e^-40 / (V e^40 / 2)`` near
``1e-39``, below the smallest normal fp32 number ``2^-126``, so each of the two products and their difference may lose
up to ``2^-126`` to gradual underflow or a flush to zero -- ``3 * 2^-126 <= 2^-124``.  (torch's fp32 softmax feeds its
exponential ``x - max``, at most ``2 span`` in magnitude, with a correctly rounded multiply-free ``exp``; its pairwise
sums are shallower than ``n(V)``; the factor 2 covers it, as in shift_cases.)

``tv = 1/2 sum |d^_v|`` is within ``1/2 sum_v eps_v + n(V) 2^-24 TV + 2^-24 TV`` of ``TV = 1/2 sum |D_v|``: the terms'
own errors, the accumulation of non-negative terms ``n(V)`` deep (the order of head_shift_kernel's sums), one
rounding of the halved result (the halving itself is exact).

Criterion for lists (``check_list``; ``up`` as written, ``dn`` mirrored through ``D -> -D``).  The filled slots come
first; unfilled slots hold id ``-1`` and value ``+0.0``.  Every listed id lies in ``[0, V)`` and is listed once; its
value is within ``eps`` of ``D`` at its id and has the list's sign; the list is sorted by (value descending, id
ascending).  Then

* for a listed id ``i`` and any id ``u`` that is not listed, or listed later: ``D_u <= D_i + eps_i + eps_u``;
* a list shorter than ``k`` leaves out no ``v`` with ``D_v > eps_v``;
* for two columns ``i < u`` on the same path of pass 2 (both in the 16-byte body, or both in the ``V % 8`` tail) with
  identical ``(p, q)`` bits, ``u`` listed implies ``i`` listed before it: the per-column value is a pure function of
  those bits and the path, and the order's tie-break is the id.

``dp_track`` is within ``eps`` of ``D`` at its id, exactly 0 for an id outside ``[0, V)``, and equal in its bits to the
list's value where the implementation lists that id.  A selected row without a baseline (``rows[i]`` outside ``[0,
R)``, ``rowmap[r]`` outside ``[0, Rb)``) and a row whose bits equal its baseline's give ``tv = +0.0``, empty lists and
``dp_track = +0.0``, bit for bit.

Cases (``movers_case``): ``Rb = 2`` baseline rows, ``R = 5`` edited rows with the rowmap ``ROWMAP`` (-1 and an index
past the table among them), selected through ``ROWS[Rs]``, ``Rs`` in {1, 3, 5} (a non-zero single row; an unmapped
row and a negative entry; an entry past ``R``, an unmapped row and a repeat), ``k`` in {1, 3, 8}, caps 30 and 40.
``ids [Rs, 4]``: a column the truth lists, one it does not, ``-1`` and ``V``.  Kinds:

* ``identical``: the edited row is its baseline row -- everything exactly zero or empty;
* ``planted``: the base is ``4 randn``; ``g = min(k + 1, V // 2)`` gainer and as many loser columns, taken from
  ``hazard_columns(V)`` first and then from a seeded permutation, gainers going from -4 to ``max + 1 + 0.5 j``, losers
  from ``max + 1.25 + 0.5 j`` to -4.  The first ``min(k, g - 1)`` ids of either list must equal the float64 truth's
  exactly (all ``k`` from ``V = 18`` on; a narrower row has no ``k + 1`` columns to plant).  This is a condition:
  ``planted_gap`` gives the smallest gap between neighbouring truth values among those ``g`` columns over ``eps_i +
  eps_u``, and tests/test_head_movers_cpu.py asserts it is large at every width and both caps;
* ``one_entry``: the edited row is its baseline row with one hazard column raised to the row maximum plus 2: ``up`` is
  exactly that column and ``k - 1`` empty slots (every other column's probability falls, by a fifth at the least);
  ``dn`` goes by the tolerance rule;
* ``tie``: two body columns (7 and the last body column; 0 and 7 in a one-vector body) given -4 -> ``max + 2``, and,
  where ``V % 8 >= 2``, the first and the last tail column given -4 -> ``max + 1.5``: identical ``(p, q)`` inside each
  pair, the largest gains of the row, the body pair's above the tail pair's by a factor ``e^0.5``.  The list starts
  with the body pair, then the tail pair, the lower id first, exactly;
* ``negation`` (``100 randn`` against its negation, saturated) and ``gain1`` / ``gain16`` (independent rows): the
  tolerance and tie rules.
"""
from __future__ import annotations

import functools
from typing import Dict, Optional, Sequence

import torch

from readout_cases import BF, NAN, STREAM_WIDTHS, Report, capped64, hazard_columns  # noqa: F401
from shift_cases import depth
from taboo_brittleness_amd.ops import reference as ref

MOVERS_CAPS = (30.0, 40.0)
MOVERS_RB = 2
MOVERS_R = 5
ROWMAP = (1, -1, 0, 2, 1)                      # row 1: no baseline (-1); row 3: an index past the table
# Rs -> selected rows: a non-zero single row; the past-table row, a mapped row, a negative entry; a row, a row, an
# entry past R, the unmapped row, a repeat (the entries without a row sit where row i itself has a baseline)
ROWS = {1: (2,), 3: (3, 2, -1), 5: (4, 0, 5, 1, 4)}
KS = (1, 3, 8)
KINDS = ("identical", "planted", "one_entry", "tie", "negation", "gain1", "gain16")
T_IDS = 4
TINY = 2.0 ** -124


def delta(V: int, span: torch.Tensor) -> torch.Tensor:
    return 2.0 ** -22 * (span + depth(V) + 4.0)


def movers_truth(z: torch.Tensor, y: torch.Tensor, cap: float) -> Dict[str, torch.Tensor]:
    """float64 truth and bounds for edited rows ``z [n, V]`` against baseline rows ``y [n, V]`` (bf16, already
    gathered): ``D``, ``eps`` ``[n, V]``, ``tv``, ``tv_bound`` ``[n]``."""
    V = z.shape[-1]
    q, p = capped64(z, cap, True), capped64(y, cap, True)
    P, Q = torch.softmax(p, -1), torch.softmax(q, -1)
    D = Q - P
    span = torch.maximum(p.abs().max(-1).values, q.abs().max(-1).values)
    eps = delta(V, span)[:, None] * (P + Q) + TINY
    tv = 0.5 * D.abs().sum(-1)
    return {"D": D, "eps": eps, "tv": tv, "tv_bound": 0.5 * eps.sum(-1) + (depth(V) + 1) * 2.0 ** -24 * tv}


def truth_list(D: torch.Tensor, k: int) -> torch.Tensor:
    """The float64 truth's list of one row ``D [V]``: the ``k`` largest ``D > 0`` by (value descending, id ascending),
    ``-1`` in the slots that stay empty."""
    vals, idx = torch.sort(D, descending=True, stable=True)
    out = torch.full((k,), -1, dtype=torch.long)
    n = min(k, int((vals > 0).sum()))
    out[:n] = idx[:n]
    return out


def planted_columns(V: int, k: int, b: int):
    """``(gainers, losers)`` of baseline row ``b``: ``g = min(k + 1, V // 2)`` columns each, hazard columns first."""
    g = min(k + 1, V // 2)
    gen = torch.Generator().manual_seed(52000 + 11 * V + 3 * k + b)
    hz = hazard_columns(V)
    rest = [c for c in torch.randperm(V, generator=gen).tolist() if c not in hz]
    cols = (hz + rest)[: 2 * g]
    return cols[0::2][:g], cols[1::2][:g]


def tie_columns(V: int):
    """``(body pair or None, tail pair or None)`` of the ``tie`` kind."""
    nv = V >> 3
    body = None if nv < 1 else ((7, 8 * nv - 1) if nv >= 2 else (0, 7))
    tail = (8 * nv, V - 1) if V % 8 >= 2 else None
    return body, tail


@functools.lru_cache(maxsize=None)
def movers_case(V: int, kind: str, Rs: int, k: int):
    """``(logits [5, V] bf16, base [2, V] bf16, rowmap [5] int32, rows [Rs] int32, labels [Rs])``, seeded; shared by
    the tests, not to be written to.  ``labels[i]`` names selected row ``i``."""
    g = torch.Generator().manual_seed(41000 + 7 * V + 100003 * KINDS.index(kind) + 13 * Rs + k)
    gain = {"negation": 100.0, "gain16": 16.0, "gain1": 1.0}.get(kind, 4.0)
    base = (gain * torch.randn(MOVERS_RB, V, generator=g)).float()
    logits = (gain * torch.randn(MOVERS_R, V, generator=g)).float()
    hz = hazard_columns(V)
    mxs = {}
    if kind == "planted":
        for b in range(MOVERS_RB):
            mxs[b] = float(base[b].to(BF).float().max())        # the random row's maximum, before planting
            up, dn = planted_columns(V, k, b)
            for c in up:
                base[b, c] = -4.0
            for j, c in enumerate(dn):
                base[b, c] = mxs[b] + 1.25 + 0.5 * j
    if kind == "tie":
        body, tail = tie_columns(V)
        for b in range(MOVERS_RB):
            for c in (body or ()) + (tail or ()):
                base[b, c] = -4.0
    base = base.to(BF)
    logits = logits.to(BF)
    row_lab = []
    for r, b in enumerate(ROWMAP):
        if not 0 <= b < MOVERS_RB:
            row_lab.append(f"{kind} unmapped({b})")
            continue
        lab = f"{kind} base {b}"
        if kind == "identical":
            logits[r] = base[b]
        elif kind == "planted":
            logits[r] = base[b]
            up, dn = planted_columns(V, k, b)
            for j, c in enumerate(up):
                logits[r, c] = mxs[b] + 1.0 + 0.5 * j
            for c in dn:
                logits[r, c] = -4.0
        elif kind == "one_entry":
            h = hz[-1 - (r % len(hz))]                         # row 0: the last column
            logits[r] = base[b]
            logits[r, h] = (base[b].float().max() + 2).to(BF)
            lab = f"one_entry@{h} base {b}"
        elif kind == "tie":
            logits[r] = base[b]
            body, tail = tie_columns(V)
            mx = base[b].float().max()
            for c in body or ():
                logits[r, c] = (mx + 2).to(BF)
            for c in tail or ():
                logits[r, c] = (mx + 1.5).to(BF)
        elif kind == "negation":
            logits[r] = -base[b]
        row_lab.append(lab)
    rows = ROWS[Rs]
    labels = tuple(row_lab[r] if 0 <= r < MOVERS_R else f"{kind} no row({r})" for r in rows)
    return logits, base, torch.tensor(ROWMAP, dtype=torch.int32), torch.tensor(rows, dtype=torch.int32), labels


@functools.lru_cache(maxsize=None)
def case_truth(V: int, kind: str, Rs: int, k: int, cap: float):
    """:func:`movers_truth` of a case's selected rows (rows without a baseline against baseline row 0; they must give
    zeros anyway), plus ``ok`` (the selected row has a baseline), ``same`` (its bits equal its baseline's), ``pb`` /
    ``qb`` (the rows' bf16 bits as int32, for the tie rule) and ``ids [Rs, 4]`` (int32): a column the truth lists (its
    top gainer; the top loser without one; 0 without either), one it lists nowhere (the column of the smallest
    ``|D|`` outside both truth lists; -1 if every column is listed), -1 and V."""
    z, y, rm, rows, _ = movers_case(V, kind, Rs, k)
    rok = (rows >= 0) & (rows < MOVERS_R)
    b = rm[rows.long().clamp(0, MOVERS_R - 1)]
    ok = rok & (b >= 0) & (b < MOVERS_RB)
    zz = z[rows.long().clamp(0, MOVERS_R - 1)]
    yy = y[b.long().clamp(0, MOVERS_RB - 1)]
    t = movers_truth(zz, yy, cap)
    t["ok"] = ok
    t["same"] = ok & (zz.view(torch.int16) == yy.view(torch.int16)).all(-1)
    t["pb"], t["qb"] = yy.view(torch.int16).int(), zz.view(torch.int16).int()
    ids = torch.empty(Rs, T_IDS, dtype=torch.int32)
    t["up"], t["dn"] = [], []
    for i in range(Rs):
        up, dn = truth_list(t["D"][i], k), truth_list(-t["D"][i], k)
        t["up"].append(up)
        t["dn"].append(dn)
        listed = set(up.tolist()) | set(dn.tolist())
        first = int(up[0]) if int(up[0]) >= 0 else (int(dn[0]) if int(dn[0]) >= 0 else 0)
        a = t["D"][i].abs().clone()
        a[[c for c in listed if c >= 0]] = float("inf")
        other = int(a.argmin()) if bool((a < float("inf")).any()) else -1
        ids[i] = torch.tensor([first, other, -1, V])
    t["ids"] = ids
    return t


def planted_gap(V: int, Rs: int, k: int, cap: float) -> float:
    """The room of the ``planted`` condition: over the live rows and both lists, the smallest gap between
    neighbouring truth values among the first ``min(k, g - 1) + 1`` entries, as a multiple of ``eps_i + eps_u``
    (``inf`` where nothing is compared)."""
    t = case_truth(V, "planted", Rs, k, cap)
    g = min(k + 1, V // 2)
    m = min(k, g - 1)
    room = float("inf")
    for i in range(Rs):
        if not bool(t["ok"][i]) or m < 1:
            continue
        for sign in (1.0, -1.0):
            vals, idx = torch.sort(sign * t["D"][i], descending=True, stable=True)
            e = t["eps"][i][idx]
            for j in range(m):
                room = min(room, float((vals[j] - vals[j + 1]) / (e[j] + e[j + 1])))
    return room


# ---- checks --------------------------------------------------------------------------------------------------
def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.detach().cpu().contiguous().view(torch.int32)


def check_list(rep: Report, what: str, ids: torch.Tensor, vals: torch.Tensor, D: torch.Tensor, eps: torch.Tensor,
               sign: float, pb: torch.Tensor, qb: torch.Tensor) -> int:
    """One row's list ``ids / vals [k]`` (on the CPU) against the criterion for lists; ``sign`` -1 for ``dn``.
    Returns the number of filled slots."""
    V, k = D.numel(), ids.numel()
    ids = ids.long()
    Ds, v = sign * D, sign * vals.double()
    filled = int((ids >= 0).sum())
    n0 = rep.failures.__len__()
    if bool((ids[:filled] < 0).any()) or bool((ids[filled:] != -1).any()):
        rep.fail(f"{what}: filled slots do not come first / an unfilled id is not -1: {ids.tolist()}")
        return filled
    if bool(_bits(vals[filled:].float()).any()):
        rep.fail(f"{what}: an unfilled slot's value is not +0.0: {vals.tolist()}")
    li = ids[:filled]
    if bool((li >= V).any()) or len(set(li.tolist())) != filled:
        rep.fail(f"{what}: ids out of range or repeated: {ids.tolist()}")
        return filled
    lv = v[:filled]
    frac = (lv - Ds[li]).abs() / eps[li]
    for a in range(filled):
        if not float(frac[a]) <= 1.0:
            rep.fail(f"{what} slot {a} id {int(li[a])}: value {float(vals[a])!r}, want {float(D[li[a]])!r} +- "
                     f"{float(eps[li[a]]):.3e} ({float(frac[a]):.3g} of the bound)")
        if not float(lv[a]) > 0.0:
            rep.fail(f"{what} slot {a} id {int(li[a])}: value {float(vals[a])!r} has not the list's sign")
        prev, cur = float(lv[a - 1]), float(lv[a])
        if a and not (prev > cur or (prev == cur and int(li[a - 1]) < int(li[a]))):
            rep.fail(f"{what} slots {a - 1}, {a}: not sorted by (value, id): {vals.tolist()} {ids.tolist()}")
    if filled and len(rep.failures) == n0:
        rep.use(what.split(" V ")[0] + " values", float(frac.max()))
    # a listed id against every id not listed, or listed later
    free = torch.ones(V, dtype=torch.bool)
    low = Ds - eps                                              # the least an implementation may have seen
    for a in range(filled):
        free[li[a]] = False
        if bool(free.any()):
            u = int(torch.where(free, low, torch.full_like(low, -float("inf"))).argmax())
            if not float(low[u]) <= float(Ds[li[a]] + eps[li[a]]):
                rep.fail(f"{what} slot {a} id {int(li[a])} (D {float(D[li[a]])!r}): id {u} with D {float(D[u])!r} is "
                         f"not listed before it")
    if filled < k and bool(free.any()):
        miss = free & (Ds > eps)
        if bool(miss.any()):
            u = int(miss.nonzero()[0])
            rep.fail(f"{what}: {filled} of {k} slots filled, yet id {u} with D {float(D[u])!r} > eps "
                     f"{float(eps[u]):.3e} is left out ({int(miss.sum())} such ids)")
    # equal (p, q) bits on the same path: the lower id first
    nv8 = (V >> 3) * 8
    ar = torch.arange(V)
    for a in range(filled):
        u = int(li[a])
        same = (pb == pb[u]) & (qb == qb[u]) & (ar < u) & ((ar < nv8) == (u < nv8))
        same[li[:a]] = False
        if bool(same.any()):
            rep.fail(f"{what} slot {a} id {u}: id {int(same.nonzero()[0])} has the same (p, q) bits on the same path "
                     f"and is not listed before it")
    return filled


def check_row(rep: Report, tag: str, i: int, label: str, out, t, k: int, ids: torch.Tensor, V: int) -> None:
    """Selected row ``i`` of the outputs ``out`` (CPU tensors) against the truth ``t`` of its case."""
    tv, up_id, up_dp, dn_id, dn_dp, dpt = out
    what = f"{tag} row {i} ({label})"
    if not bool(t["ok"][i]) or bool(t["same"][i]):
        zero = (not _bits(tv[i:i + 1]).any() and not _bits(up_dp[i]).any() and not _bits(dn_dp[i]).any()
                and not _bits(dpt[i]).any() and bool((up_id[i] == -1).all()) and bool((dn_id[i] == -1).all()))
        if not zero:
            rep.fail(f"{what}: want tv +0.0, empty lists and dp_track +0.0 exactly, got tv {float(tv[i])!r}, up "
                     f"{up_id[i].tolist()} {up_dp[i].tolist()}, dn {dn_id[i].tolist()} {dn_dp[i].tolist()}, dp_track "
                     f"{dpt[i].tolist()}")
        return
    D, eps = t["D"][i], t["eps"][i]
    f = float((tv[i].double() - t["tv"][i]).abs() / t["tv_bound"][i])
    if not f <= 1.0:
        rep.fail(f"tv {what}: got {float(tv[i])!r}, want {float(t['tv'][i])!r} +- {float(t['tv_bound'][i]):.3e} "
                 f"({f:.3g} of the bound)")
    else:
        rep.use("tv", f)
    check_list(rep, f"up {what}", up_id[i], up_dp[i], D, eps, 1.0, t["pb"][i], t["qb"][i])
    check_list(rep, f"dn {what}", dn_id[i], dn_dp[i], D, eps, -1.0, t["pb"][i], t["qb"][i])
    for j in range(ids.shape[1]):
        c = int(ids[i, j])
        if not 0 <= c < V:
            if _bits(dpt[i, j:j + 1]).any():
                rep.fail(f"dp_track {what} id {c}: got {float(dpt[i, j])!r}, want exactly +0.0 (id out of range)")
            continue
        f = float((dpt[i, j].double() - D[c]).abs() / eps[c])
        if not f <= 1.0:
            rep.fail(f"dp_track {what} id {c}: got {float(dpt[i, j])!r}, want {float(D[c])!r} +- {float(eps[c]):.3e} "
                     f"({f:.3g} of the bound)")
        else:
            rep.use("dp_track", f)
        for li, lv in ((up_id[i], up_dp[i]), (dn_id[i], dn_dp[i])):
            hit = (li == c).nonzero().reshape(-1)
            if hit.numel():
                rep.use("tracked ids found listed", 1.0)
                if not torch.equal(_bits(lv[hit[:1]]), _bits(dpt[i, j:j + 1])):
                    rep.fail(f"dp_track {what} id {c}: {float(dpt[i, j])!r} differs in its bits from the list's "
                             f"{float(lv[hit[0]])!r}")
    kind = label.split()[0].split("@")[0]
    if kind == "planted":
        m = min(k, min(k + 1, V // 2) - 1)
        for name, got, want in (("up", up_id[i], t["up"][i]), ("dn", dn_id[i], t["dn"][i])):
            if got[:m].long().tolist() != want[:m].tolist():
                rep.fail(f"{name} {what}: planted ids {got[:m].tolist()}, want the truth's {want[:m].tolist()} exactly")
    if kind == "one_entry" and V > 1:
        h = int(label.split("@")[1].split()[0])
        if up_id[i].tolist() != [h] + [-1] * (k - 1):
            rep.fail(f"up {what}: ids {up_id[i].tolist()}, want exactly [{h}] and {k - 1} empty slots")
    if kind == "tie":
        body, tail = tie_columns(V)
        want = (list(body or ()) + list(tail or ()))[:k]
        if up_id[i][: len(want)].tolist() != want:
            rep.fail(f"up {what}: tie ids {up_id[i].tolist()}, want {want} first, the lower id of each pair first")


def _outs(dev, Rs: int, k: int, T: int) -> Dict[str, torch.Tensor]:
    """NaN / -7 filled outputs, so that an element the implementation does not write shows."""
    f = lambda *s: torch.full(s, NAN, device=dev)                                   # noqa: E731
    n = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)                 # noqa: E731
    return {"tv": f(Rs), "up_id": n(Rs, k), "up_dp": f(Rs, k), "dn_id": n(Rs, k), "dn_dp": f(Rs, k),
            "dp_track": f(Rs, T)}


def run_movers(head_movers, dev, V: int, caps: Sequence[float] = MOVERS_CAPS, kinds: Sequence[str] = KINDS,
               Rss: Sequence[int] = (1, 3, 5), ks: Sequence[int] = KS, fill: bool = True) -> Report:
    """``head_movers`` on every case of width ``V``.  ``fill``: hand it sentinel-filled outputs."""
    rep = Report()
    for kind in kinds:
        for Rs in Rss:
            for k in ks:
                z, y, rm, rows, labels = movers_case(V, kind, Rs, k)
                gz, gy, gm, gr = z.to(dev), y.to(dev), rm.to(dev), rows.to(dev)
                for cap in caps:
                    t = case_truth(V, kind, Rs, k, cap)
                    outs = _outs(dev, Rs, k, T_IDS) if fill else {}
                    out = head_movers(gz, gy, gm, gr, cap, k, t["ids"].to(dev), **outs)
                    out = tuple(o.detach().cpu() for o in out)
                    tag = f"{kind} V {V} Rs {Rs} k {k} cap {cap:g}"
                    shapes = [tuple(o.shape) for o in out]
                    if shapes != [(Rs,), (Rs, k), (Rs, k), (Rs, k), (Rs, k), (Rs, T_IDS)]:
                        rep.fail(f"{tag}: output shapes {shapes}")
                        continue
                    for i in range(Rs):
                        check_row(rep, tag, i, labels[i], out, t, k, t["ids"], V)
    return rep


# ---- deliberately wrong stand-ins ------------------------------------------------------------------------------
def movers_mutant(drop_tail: bool = False, tie_high: bool = False, no_sums: bool = False, ignore_map: bool = False,
                  ignore_rows: bool = False, list_zeros: bool = False, swap_lists: bool = False):
    """The reference in fp32 with one planted bug: ``drop_tail`` leaves the ``V % 8`` tail columns out of the sums and
    the lists; ``tie_high`` prefers the higher id among equal values; ``no_sums`` takes ``e^q - e^p`` for the
    difference, without the two sums; ``ignore_map`` compares row ``r`` with baseline row ``r % Rb`` whatever the
    rowmap says; ``ignore_rows`` reads row ``i`` for selected row ``i`` whatever ``rows`` says; ``list_zeros`` lists
    zero-valued entries where ``-1`` belongs; ``swap_lists`` returns the losers as gainers and the gainers as losers.
    With the defaults nothing is wrong."""

    def head_movers(logits, base, rowmap, rows, cap, k, ids=None, **outs):
        R, V = logits.shape
        Rb, Rs = base.shape[0], rows.numel()
        T = 0 if ids is None else ids.shape[1]
        rs = rows.long()
        if ignore_rows:
            rs = torch.arange(Rs) % R
        rok = (rs >= 0) & (rs < R)
        rc = rs.clamp(0, R - 1)
        bm = (rc % Rb) if ignore_map else rowmap.long()[rc]
        ok = rok & (bm >= 0) & (bm < Rb)
        q = ref._capped(logits, cap, True)[rc]
        p = ref._capped(base, cap, True)[bm.clamp(0, Rb - 1)]
        nv8 = (V >> 3) * 8 if drop_tail else V
        d = torch.zeros(Rs, V)
        if nv8:
            if no_sums:
                d[:, :nv8] = torch.exp(q[:, :nv8]) - torch.exp(p[:, :nv8])
            else:
                d[:, :nv8] = torch.softmax(q[:, :nv8], -1) - torch.softmax(p[:, :nv8], -1)
        d = torch.where(ok[:, None], d, torch.zeros_like(d))
        tv = 0.5 * d.abs().sum(-1)
        kk = min(k, V)
        res = []
        for sign in (1.0, -1.0):
            x = sign * d
            if tie_high:
                vals, idx = torch.sort(x.flip(-1), dim=-1, descending=True, stable=True)
                idx = V - 1 - idx
            else:
                vals, idx = torch.sort(x, dim=-1, descending=True, stable=True)
            vals, idx = vals[:, :kk], idx[:, :kk].to(torch.int32)
            hit = (vals >= 0) if list_zeros else (vals > 0)
            oi = torch.full((Rs, k), -1, dtype=torch.int32)
            ov = torch.zeros(Rs, k)
            oi[:, :kk] = torch.where(hit, idx, torch.full_like(idx, -1))
            ov[:, :kk] = torch.where(hit, sign * vals, torch.zeros_like(vals))
            res.append((oi, ov))
        if swap_lists:
            res = res[::-1]
        dpt = torch.zeros(Rs, T)
        if T:
            tt = ids.long()
            g = torch.gather(d, 1, tt.clamp(0, V - 1))
            dpt = torch.where((tt >= 0) & (tt < V), g, torch.zeros_like(g))
        out = (tv, res[0][0], res[0][1], res[1][0], res[1][1], dpt)
        for name, v in zip(("tv", "up_id", "up_dp", "dn_id", "dn_dp", "dp_track"), out):
            if outs.get(name) is not None:
                outs[name].copy_(v)
        return out

    return head_movers
