"""The criteria of tests/test_readouts_gpu.py, checked against themselves on the CPU (tests/readout_cases.py): first
ops/reference.py in fp32 meets every bound on every case, so the bounds leave room for a correct fp32 implementation;
then every assertion is turned against a result with one planted bug, which it must reject at every width where the
bug can show; last, the tolerances these criteria replace would have let two of those bugs through."""
import pytest
import torch

import readout_cases as rd
from rounding_cases import all_bf16, bf16_step, bf16_ulps

CPU = torch.device("cpu")


# ---- the reference stays inside the bounds ------------------------------------------------------------------------
@pytest.mark.parametrize("V", rd.STREAM_WIDTHS)
def test_reference_meets_stream_criteria(V):
    rd.run_stream(rd.reference_impl(), CPU, V, fill=True).assert_ok(f"reference V {V}")


def test_reference_meets_persist_criteria():
    """515 rows: 2 x 256 compute units + 3."""
    rd.run_persist(rd.reference_impl(), CPU, 515, fill=True).assert_ok("reference persist")


@pytest.mark.parametrize("V", rd.GATHER_WIDTHS)
def test_reference_meets_gather_criteria(V):
    rd.run_gather(rd.reference_impl(), CPU, V, fill=True).assert_ok(f"reference V {V}")


@pytest.mark.parametrize("rb", [False, True])
@pytest.mark.parametrize("V", rd.COLSUM_WIDTHS)
def test_reference_meets_colsum_criteria(V, rb):
    rd.run_colsum(rd.reference_impl(), CPU, V, rb, bits=False).assert_ok(f"reference V {V}")


@pytest.mark.parametrize("V", rd.TOPK_WIDTHS)
def test_reference_meets_topk_criteria(V):
    rd.run_topk(rd.reference_impl(), CPU, V).assert_ok(f"reference V {V}")
    rd.run_topk_all(rd.reference_impl(), CPU).assert_ok("reference")


def test_cases_cover_what_they_claim():
    """The widths give the vector counts they were chosen for; a planted maximum carries enough of its row that
    leaving it out moves the lse by over a thousand times the bound, at every width past 1 and every cap; the
    saturated tie is one at caps 30 and 50 and none without a cap."""
    assert [V >> 3 for V in rd.STREAM_WIDTHS] == [0, 0, 1, 1, 511, 512, 513, 2047, 2048, 2049, 4099]
    least = 1.0
    for V in rd.STREAM_WIDTHS[1:]:
        z, labels, tie = rd.stream_rows(V)
        for cap in rd.CAPS:
            r = rd.stream_ref(V, cap, True)
            bound = rd.lse_bound(r["lse"], r["span_online"], cap, True)
            for i, lab in enumerate(labels):
                if lab.startswith("planted@"):
                    share = float(torch.exp(r["cmax"][i] - r["lse"][i]))
                    least = min(least, share)
                    assert int(r["amax"][i]) == int(lab[8:])
                    assert -torch.log1p(torch.tensor(-share, dtype=torch.float64)) > 1000 * bound[i], (V, cap, lab)
            s = labels.index("sat_tie")
            n_max = int((r["c"][s] == r["cmax"][s]).sum())
            assert (n_max >= 2 and int(r["amax"][s]) == tie) if cap > 0 else n_max == 1, (V, cap)
    print(f"smallest share of a planted maximum in its row: {least:.3f}")
    assert least > 0.15


def test_prob_window_over_every_logit():
    """fp32 ``exp(z - lse)`` lies inside ``prob_window`` for every finite bf16 logit up to 80 (past it fp32
    overflows), plain and rounded; the rounded window is one or two bf16 values wide wherever the probability is a
    normal number, and a value one bf16 step outside it is rejected."""
    z = all_bf16().float()
    z = z[torch.isfinite(z) & (z <= 80)]
    lse = torch.tensor([3.7109375])
    p = torch.exp(z - lse)
    for rb in (False, True):
        lo, hi, p64, _err = rd.prob_window(z, lse, rb)
        got = p.to(torch.bfloat16).float() if rb else p
        assert bool(rd._inside(got, lo, hi, rb).all())
    normal = p64 > 2.0 ** -100
    assert int(bf16_ulps(lo, hi)[normal].max()) <= 1
    above = bf16_step(hi, 1).float()
    assert not bool(rd._inside(above, lo, hi, True)[normal].any())


# ---- planted bugs are rejected ------------------------------------------------------------------------------------
_LSE_OPS = ("row_lse", "xent_rows", "decode_head nll_self", "decode_head_stats lse")


@pytest.mark.parametrize("V", [V for V in rd.STREAM_WIDTHS if V % 8])
def test_rejects_softcap_skipped_on_the_tail(V):
    rep = rd.run_stream(rd.stream_mutant(cap_tail=False), CPU, V, caps=(30.0, 50.0))
    if V == 1:      # the one planted logit may be too small for the cap to change it, and every NLL is 0; `lens` fails
        assert rep.failed("row_lse", "lens") and rep.failed("decode_head_stats lse", "lens"), rep.failures
        return
    for op in _LSE_OPS:
        assert rep.failed(op, "cap 30", "planted@"), (op, rep.failures)
    assert rep.failed("row_lse", "cap 50", "planted@")
    assert not rd.run_stream(rd.stream_mutant(cap_tail=False), CPU, V, caps=(0.0,)).failures


@pytest.mark.parametrize("V", [V for V in rd.STREAM_WIDTHS if V >= 8])
def test_rejects_a_dropped_vector_at_every_boundary(V):
    for j in rd.boundary_vectors(V):
        rep = rd.run_stream(rd.stream_mutant(drop_vec=j), CPU, V, caps=(30.0,))
        for op in _LSE_OPS + ("argmax_rows", "decode_head nxt", "decode_head_stats id"):
            assert any(rep.failed(op, f"(planted@{c})") for c in (8 * j, 8 * j + 7)), (V, j, op, rep.failures)


@pytest.mark.parametrize("V", rd.STREAM_WIDTHS[1:])
def test_rejects_a_tie_resolved_upwards(V):
    rep = rd.run_stream(rd.stream_mutant(tie_high=True), CPU, V, caps=(30.0, 50.0))
    for op in ("argmax_rows", "decode_head nxt", "decode_head_stats id"):
        assert rep.failed(op, "sat_tie") and rep.failed(op, "equal") and rep.failed(op, "sat_neg"), (op, rep.failures)
    assert rep.failed("argmax_rows cap 50", "sat_tie") and rep.failed("decode_head nxt cap 50", "sat_tie")


@pytest.mark.parametrize("V", rd.STREAM_WIDTHS)
def test_rejects_a_maximum_taken_from_the_row_before(V):
    rep = rd.run_stream(rd.stream_mutant(neighbour_max=True), CPU, V, caps=(0.0,))
    for op in ("row_lse", "xent_rows", "decode_head nll_self"):
        assert rep.failed(op, "lens"), (op, rep.failures)


def test_rejects_a_stale_row_in_the_persistent_case():
    """Every row of the 515 is different, so a workgroup that reported its first row's results for its second fails
    on all three outputs."""
    ok = rd.reference_impl()

    def stale(lg, cap, tgt=None):
        nxt, ns, nt = ok.decode_head(lg, cap, tgt)
        return nxt.roll(512), ns.roll(512), nt.roll(512)

    def stale_stats(lg, tgt, off, cap):
        return ok.decode_head_stats(lg, tgt, off, cap).roll(512, 0)

    rep = rd.run_persist(rd.SimpleNamespace(decode_head=stale, decode_head_stats=stale_stats), CPU, 515)
    for op in ("decode_head nxt", "decode_head nll_self", "decode_head nll_tgt", "decode_head_stats lse",
               "decode_head_stats best", "decode_head_stats id", "decode_head_stats target"):
        assert rep.failed(op), (op, rep.failures[:5])


@pytest.mark.parametrize("V", rd.GATHER_WIDTHS)
def test_rejects_gather_bugs(V):
    rep = rd.run_gather(rd.gather_mutant(force_round=False), CPU, V)
    assert rep.failed("round_bf16 1") and not rep.failed("round_bf16 0"), rep.failures
    rep = rd.run_gather(rd.gather_mutant(force_round=True), CPU, V)
    assert rep.failed("round_bf16 0") and not rep.failed("round_bf16 1"), rep.failures
    rep = rd.run_gather(rd.gather_mutant(neighbour_lse=True), CPU, V)
    assert rep.failed("rowmap round_bf16 0") and rep.failed("rowmap round_bf16 1"), rep.failures
    assert all("rowmap" in f for f in rep.failures)

    def nonzero_outside(lg, lse, ids, round_bf16=False, rowmap=None):
        return rd.reference_impl().gather_probs(lg, lse, ids.clamp(0, V - 1), round_bf16=round_bf16, rowmap=rowmap)

    rep = rd.run_gather(rd.SimpleNamespace(gather_probs=nonzero_outside), CPU, V)
    assert rep.failed("out of range")


@pytest.mark.parametrize("rb", [False, True])
@pytest.mark.parametrize("V", rd.COLSUM_WIDTHS)
def test_rejects_colsum_bugs(V, rb):
    for slot in (0, 1):
        rep = rd.run_colsum(rd.colsum_mutant(ignore_excl=slot), CPU, V, rb, bits=False)
        assert rep.failed("dense accumulate 0") and rep.failed("packed") and rep.failed("rowmap") == (slot == 0), \
            (slot, rep.failures)
    rep = rd.run_colsum(rd.colsum_mutant(ignore_mask=True), CPU, V, rb, bits=False)
    assert rep.failed("dense accumulate 0", "acc[2]") and rep.failed("dense accumulate 1", "acc[2]"), rep.failures
    assert all("dense accumulate" in f for f in rep.failures)
    rep = rd.run_colsum(rd.colsum_mutant(drop_start=True), CPU, V, rb, bits=False)
    assert rep.failed("dense accumulate 1") and rep.failed("packed", "accumulate 1"), rep.failures
    assert all("accumulate 1" in f for f in rep.failures)
    if V > 1:                        # at V = 1 every probability is exactly 1 and rounding it changes nothing
        rep = rd.run_colsum(rd.colsum_mutant(force_round=not rb), CPU, V, rb, bits=False)
        assert rep.failed("dense") and rep.failed("packed") and rep.failed("rowmap"), rep.failures


def test_rejects_an_acc_that_is_not_overwritten():
    """``accumulate=False`` onto a NaN-filled ``acc``: an implementation that adds to it fails."""
    ok = rd.reference_impl()

    def adds(lg, lse, mask, excl, B, T, acc=None, accumulate=False, **kw):
        return ok.lens_colsum(lg, lse, mask, excl, B, T, acc=acc, accumulate=acc is not None, **kw)

    rep = rd.run_colsum(rd.SimpleNamespace(lens_colsum=adds), CPU, 2049, False, bits=False)
    assert rep.failed("dense accumulate 0") and rep.failed("packed", "accumulate 0")


def test_rejects_topk_ties_resolved_upwards():
    rep = rd.run_topk(rd.SimpleNamespace(topk_rows=rd.topk_tie_high), CPU, 4097, Ks=(1, 9, 64))
    for K in (1, 9, 64):
        assert rep.failed(f"K {K} ", "constant"), rep.failures
    assert rep.failed("K 9 ", "ties") and rep.failed("K 64 ", "few_finite")
    assert all(any(f"({lab})" in f for lab in ("constant", "ties", "few_finite")) for f in rep.failures)
    assert rd.run_topk_all(rd.SimpleNamespace(topk_rows=rd.topk_tie_high), CPU).failed("constant")


# ---- why the old tolerances were not enough -------------------------------------------------------------------------
def test_old_tolerances_pass_the_first_two_bugs_on_random_rows():
    """At V = 32795 -- the geometry of test_vocab_readouts and test_decode_head -- on the ``4 randn`` rows those tests
    use, a softcap skipped on the tail and a vector of ordinary mass dropped at an unroll boundary move lse and NLL by
    less than the ``atol`` of 1e-3 they were compared with; the derived bound rejects both on the planted rows
    (above).  The bound itself is 15 to 60 times below that ``atol`` on these rows."""
    V, cap = 32795, 30.0
    z, labels, _tie = rd.stream_rows(V)
    rnd = [i for i, lab in enumerate(labels) if lab == "random"]
    want = rd.stream_ref(V, cap, True)
    tgt = torch.zeros(len(labels), dtype=torch.int32)
    ct =torch.gather(want["c"], 1, tgt.long().clamp(0, V - 1)[:, None])[:, 0]
    bound = rd.lse_bound(want["lse"], want["span_online"], cap, True)[rnd]
    print(f"bound on the random rows: {float(bound.min()):.2e} .. {float(bound.max()):.2e}")
    assert 1e-3 / 60 < float(bound.min()) and float(bound.max()) < 1e-3 / 15
    for mut in (rd.stream_mutant(cap_tail=False), rd.stream_mutant(drop_vec=512), rd.stream_mutant(drop_vec=2047)):
        lse = mut.row_lse(z, cap, True).double()
        nll = mut.xent_rows(z, tgt, cap, True).double()
        dl = (lse - want["lse"]).abs()[rnd]
        dn = (nll - (want["lse"] - ct)).abs()[rnd]
        print(f"moved lse by {float(dl.max()):.2e}, NLL by {float(dn.max()):.2e}")
        assert float(dl.max()) <= 1e-3 and float(dn.max()) <= 2e-3
        assert float(dl.min()) > 0
