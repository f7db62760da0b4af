"""Output movers on the MI355X: ``ops.head_movers`` (csrc/lens.hip head_movers_kernel) against the criteria of
tests/movers_cases.py at every stream width, the exact zeros of identical rows, the independence of a row's bits from
the launch around it, the tracked ids' floats, the inputs that raise, and the sweep with
``intervention.output_movers`` across its reuse levels, with the switch off and beside the output shift."""
import pytest
import torch

from movers_cases import MOVERS_CAPS, case_truth, movers_case, run_movers
from readout_cases import STREAM_WIDTHS
from taboo_brittleness_amd import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("V", STREAM_WIDTHS)
def test_kernel_meets_the_criteria(gpu, V):
    """Every kind of row pair, Rs in {1, 3, 5} of five rows against two baseline rows, k in {1, 3, 8}, caps 30 and 40,
    NaN / -7 filled outputs."""
    rep = run_movers(ops.head_movers, gpu, V)
    rep.assert_ok(f"head_movers kernel V {V}")
    assert V == 1 or rep.used.get("tracked ids found listed") == 1.0


@pytest.mark.parametrize("V", STREAM_WIDTHS)
def test_identical_rows_give_exact_zero(gpu, V):
    """Rows of equal bits -- random, saturated, and at the far rows of a table, where odd widths misalign the two
    rows differently -- give tv = +0.0, empty lists and dp_track = +0.0, bit for bit."""
    g = torch.Generator().manual_seed(V)
    base = torch.cat([4 * torch.randn(3, V, generator=g), 100 * torch.randn(2, V, generator=g)]).to(BF).to(gpu)
    rm = _i32([4, 0, 3, 1, 2, 2, 0], gpu)
    logits = base[rm.long()].contiguous()
    rows = _i32([6, 0, 2, 4, 1, 3, 5, 0], gpu)
    ids = torch.randint(0, V, (8, 8), generator=g, dtype=torch.int32).to(gpu)
    for cap in MOVERS_CAPS:
        for k in (1, 8):
            outs = {"tv": torch.full((8,), float("nan"), device=gpu),
                    "up_id": torch.full((8, k), -7, dtype=torch.int32, device=gpu),
                    "up_dp": torch.full((8, k), float("nan"), device=gpu),
                    "dn_id": torch.full((8, k), -7, dtype=torch.int32, device=gpu),
                    "dn_dp": torch.full((8, k), float("nan"), device=gpu),
                    "dp_track": torch.full((8, 8), float("nan"), device=gpu)}
            tv, ui, ud, di, dd, dpt = ops.head_movers(logits, base, rm, rows, cap, k, ids, **outs)
            assert not _bits(tv).any() and not _bits(ud).any() and not _bits(dd).any(), (cap, k)
            assert not _bits(dpt).any(), (cap, k)
            assert bool((ui == -1).all()) and bool((di == -1).all()), (cap, k)


@pytest.mark.parametrize("V", (9, 4104, 16397, 32795))
def test_row_bits_do_not_depend_on_the_launch(gpu, V):
    """One (edited row, baseline row) pair launched alone, as row 3 of 5 against a larger table, through permuted
    ``rows`` / ``rowmap``, and among more selected rows than the persistent grid has workgroups: the same bits in
    every output each time."""
    k = 8
    z, y, _rm, _rows, _ = movers_case(V, "gain16", 5, k)
    ids1 = case_truth(V, "gain16", 5, k, 30.0)["ids"][:1]
    ids1 = torch.cat([ids1, torch.tensor([[0, V - 1, V // 2, 7 % V]], dtype=torch.int32)], 1).to(gpu)     # T = 8
    z, y = z.to(gpu), y.to(gpu)
    g = torch.Generator().manual_seed(5 * V)
    more = (4 * torch.randn(4, V, generator=g)).to(BF).to(gpu)
    junk = torch.randint(-1, V + 1, (8,), generator=g, dtype=torch.int32).to(gpu)[None]
    for cap in MOVERS_CAPS:
        alone = ops.head_movers(z[4:5].contiguous(), y[1:2].contiguous(), _i32([0], gpu), _i32([0], gpu), cap, k, ids1)
        assert float(alone[0]) > 0 and int(alone[1][0, 0]) >= 0 and int(alone[3][0, 0]) >= 0
        assert V == 9 or (int(alone[1][0, k - 1]) >= 0 and int(alone[3][0, k - 1]) >= 0)
        tab = torch.cat([more[:2], y[1:2], more[2:]]).contiguous()                # the baseline row is row 2 of 5
        lg5 = torch.cat([more[:3], z[4:5], more[3:]]).contiguous()                # the edited row is row 3 of 5
        for rm, rows in (([0, 1, 3, 2, 4], [0, 1, 2, 3, 4]), ([4, 3, -1, 2, 2], [4, 3, 0]),
                         ([1, 1, 1, 2, 0], [7, 2, 3, 3])):
            at = rows.index(3)
            idn = junk.repeat(len(rows), 1).contiguous()
            idn[at] = ids1[0]
            got = ops.head_movers(lg5, tab, _i32(rm, gpu), _i32(rows, gpu), cap, k, idn)
            for a, b in zip(alone, got):
                assert torch.equal(_bits(a[0]), _bits(b[at])), (cap, rm, rows)
        Rs = 1100                                                                 # > 2 workgroups per CU
        got = ops.head_movers(z[4:5].contiguous(), y[1:2].contiguous(), _i32([0], gpu),
                              torch.zeros(Rs, dtype=torch.int32, device=gpu), cap, k, ids1.expand(Rs, 8).contiguous())
        for a, b in zip(alone, got):
            assert bool((_bits(b).reshape(Rs, -1) == _bits(a[0]).reshape(1, -1)).all()), cap
        # a shorter list is the longer list's head, and the tracked values do not depend on k or T
        short = ops.head_movers(z[4:5].contiguous(), y[1:2].contiguous(), _i32([0], gpu), _i32([0], gpu), cap, 3,
                                ids1[:, :2].contiguous())
        assert torch.equal(_bits(short[0]), _bits(alone[0]))
        for j in (1, 2, 3, 4):
            assert torch.equal(_bits(short[j]), _bits(alone[j][:, :3].contiguous())), (cap, j)
        assert torch.equal(_bits(short[5]), _bits(alone[5][:, :2].contiguous()))


@pytest.mark.parametrize("V", (9, 4104, 16397, 32795))
def test_tracked_value_of_a_listed_id_is_the_lists_float(gpu, V):
    """``dp_track`` at every id the kernel lists -- body and tail columns, gainers and losers -- equals the list's
    value bit for bit."""
    k = 8
    for kind in ("gain16", "planted", "tie"):
        z, y, rm, rows, _ = movers_case(V, kind, 5, k)
        z, y, rm, rows = z.to(gpu), y.to(gpu), rm.to(gpu), rows.to(gpu)
        for cap in MOVERS_CAPS:
            tv, ui, ud, di, dd, _ = ops.head_movers(z, y, rm, rows, cap, k)
            for li, lv in ((ui, ud), (di, dd)):
                dpt = ops.head_movers(z, y, rm, rows, cap, k, li.contiguous())[5]
                live = li >= 0
                assert int(live.sum()) > 0
                assert torch.equal(_bits(dpt)[live.cpu()], _bits(lv)[live.cpu()]), (kind, cap)
                assert not _bits(dpt)[~live.cpu()].any()


def test_unsupported_inputs_raise(gpu):
    lg = torch.zeros(2, 64, dtype=BF, device=gpu)
    rm = torch.zeros(2, dtype=torch.int32, device=gpu)
    rows = _i32([1, 0], gpu)
    ids = torch.zeros(2, 3, dtype=torch.int32, device=gpu)
    out = ops.head_movers(lg, lg, rm, rows, 30.0, 2, ids)
    assert not out[0].any() and bool((out[1] == -1).all()) and not out[5].any()
    err = (RuntimeError, ValueError)
    for cap in (0.0, -1.0, 50.0):                                                  # no f kernel for these
        with pytest.raises(err):
            ops.head_movers(lg, lg, rm, rows, cap, 2, ids)
    with pytest.raises(err):
        ops.head_movers(lg, lg.cpu(), rm, rows, 30.0, 2, ids)
    with pytest.raises(err):
        ops.head_movers(lg, lg, rm, rows.cpu(), 30.0, 2, ids)
    with pytest.raises(err):
        ops.head_movers(lg, lg, rm, rows, 30.0, 2, ids.cpu())
    with pytest.raises(err):
        ops.head_movers(lg, lg[:, :32].contiguous(), rm, rows, 30.0, 2, ids)
    with pytest.raises(err):
        ops.head_movers(lg, lg, rm.long(), rows, 30.0, 2, ids)
    with pytest.raises(err):
        ops.head_movers(lg, lg, rm, rows.long(), 30.0, 2, ids)
    with pytest.raises(err):
        ops.head_movers(lg.float(), lg, rm, rows, 30.0, 2, ids)
    for k in (0, 9):
        with pytest.raises(err):
            ops.head_movers(lg, lg, rm, rows, 30.0, k, ids)
    with pytest.raises(err):
        ops.head_movers(lg, lg, rm, rows, 30.0, 2, torch.zeros(2, 9, dtype=torch.int32, device=gpu))
    e = ops.head_movers(lg, lg, rm, rows[:0], 30.0, 2, ids[:0])
    assert [tuple(o.shape) for o in e] == [(0,), (0, 2), (0, 2), (0, 2), (0, 2), (0, 3)]


# -------------------------------------------------------------------------------------------------- sweep
METHODS = ("sae_targeted", "sae_random", "proj_targeted")
NEW_KEYS = ("movers_up", "movers_dn", "tv_out_spike_mean", "movers_up_share", "movers_dn_share", "secret_loss_share",
            "secret_in_losers", "decoy_in_gainers", "top_gainer")


@pytest.fixture(scope="module")
def movers_sweeps(gpu):
    """The tiny-model sweep (in-tree GEMMs: batch-invariant) with ``intervention.output_movers`` at every reuse level
    switched one at a time, an all-no-op run forced through the tail, a run without the switch, one with the output
    shift alone and one with both, each under spies on ``ops.head_movers`` and on the model's unembedding; computed
    once."""
    from dataclasses import replace

    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.gemma2 import Gemma2Model
    from taboo_brittleness_amd.models.spec import GEMMA2_TINY
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.models.weights import random_gemma2
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from taboo_brittleness_amd.runtime import gemm_dispatch as GD

    spec = replace(GEMMA2_TINY, vocab_size=2048, layers=4, sliding_window=8)
    old = GD.mode()
    GD.set_mode("tb")
    base = ["experiment.max_new_tokens=12", "intervention.budgets=[1, 4]", "intervention.ranks=[1, 4]",
            "intervention.random_trials=2", "intervention.proj_random_trials=1"]
    mv = ["intervention.output_movers=true"]
    sh = ["intervention.output_shift=true"]
    mg = Gemma2Model(random_gemma2(spec, dtype=BF, seed=5, norm_std=0.1, device=gpu, post_norm_gain=8.0), gpu)
    tok = SyntheticTokenizer(vocab_size=spec.vocab_size)
    key = lambda r: (r["word"], r["prompt_idx"], r["method"], r["budget"], r["trial"])   # noqa: E731
    out, runners, calls, unembeds = {}, {}, {}, {}
    real, real_logits = ops.head_movers, mg.logits
    try:
        for name, extra, flags in (("default", mv, {}), ("no_skip", mv, dict(skip_noop_spikes=False)),
                                   ("no_trie", mv, dict(trie_decode=False)), ("no_dedup", mv, dict(_no_dedup=True)),
                                   ("noop", mv + ["intervention.alpha=0.0"], dict(skip_noop_spikes=False)),
                                   ("switch_off", [], {}), ("shift_only", sh, {}), ("both", sh + mv, {})):
            cfg = load_config(None, base + extra)
            sae = JumpReLUSAE.random(spec.hidden, 1024, seed=2, device=gpu)
            r = SweepRunner(cfg, mg, tok, sae, batch=64, device=gpu, layer=2, kv_pairs=8)
            for k, v in flags.items():
                if k == "_no_dedup":                     # lens rows one by one, the trie decode still on
                    r._lens_row_keys = lambda *a, **kw: None
                else:
                    setattr(r, k, v)
            n, nl = [0], [0]

            def spy(*a, _n=n, **kw):
                _n[0] += 1
                return real(*a, **kw)

            def spy_logits(*a, _n=nl, **kw):
                _n[0] += 1
                return real_logits(*a, **kw)

            ops.head_movers = spy
            mg.logits = spy_logits
            methods = ("sae_targeted",) if name == "noop" else METHODS
            pairs = r.build_pairs(["ship"], cfg.prompts[:3], methods)
            r.run_baselines(pairs)
            res = r.run_cells(pairs, r.make_cells(pairs, methods))
            out[name] = {key(x): x for x in res}
            runners[name] = (r, pairs)
            calls[name] = n[0]
            unembeds[name] = nl[0]
    finally:
        ops.head_movers = real
        del mg.logits
        GD.set_mode(old)
    return out, runners, calls, unembeds


def _same(a, b):
    return a == b or (a != a and b != b)


def test_sweep_fields_are_bit_equal_across_reuse_levels(movers_sweeps):
    """The no-op spike skip, the prefix-trie decode and the lens row dedup change which rows share a launch, never a
    row's bits: the new fields are equal as floats and ids, bit for bit."""
    out, runners, calls, _ = movers_sweeps
    ref_ = out["default"]
    st = runners["default"][0].stats
    assert st["tf_rows"] > 0 and st["diverged"] > 0 and calls["default"] > 0 and st["movers_rows"] > 0
    assert runners["no_skip"][0].stats["movers_rows"] > st["movers_rows"]      # the skip did skip selected rows
    for name in ("no_skip", "no_trie", "no_dedup"):
        assert set(out[name]) == set(ref_)
        for k, r in out[name].items():
            assert r["response_ids"] == ref_[k]["response_ids"], (name, k)
            for f in NEW_KEYS:
                assert _same(r[f], ref_[k][f]), (name, k, f, r[f], ref_[k][f])
    assert any(r["tv_out_spike_mean"] > 1e-4 and r["top_gainer"] >= 0 for r in ref_.values())
    for r in ref_.values():
        assert 0.0 <= r["tv_out_spike_mean"] <= 1.0 + 1e-5
        for f in ("movers_up_share", "movers_dn_share", "secret_loss_share"):
            assert r[f] != r[f] or 0.0 <= r[f] <= 1.0 + 1e-4, (f, r[f])


def test_noop_cells_through_the_tail_are_exactly_zero(movers_sweeps):
    """``alpha = 0`` makes every edit an exact no-op; with the skip off the cells still run their tail from the first
    spike, in a batch of their own shape.  Its rows repeat the baseline pass's bits, so every total variation is
    exactly 0, every list empty and every share NaN."""
    out, runners, calls, _ = movers_sweeps
    r_, pairs = runners["noop"]
    assert r_.stats["tf_rows"] > 0 and r_.stats["diverged"] == 0 and calls["noop"] > 0 and len(out["noop"]) == 3 * 2
    assert r_.stats["movers_rows"] > 0
    base = {(p.word, p.pidx): p for p in pairs}
    for k, r in out["noop"].items():
        assert r["response_ids"] == base[k[0], k[1]].resp
        assert r["tv_out_spike_mean"] == 0.0 and r["top_gainer"] == -1, (k, r["tv_out_spike_mean"])
        assert not any(r["movers_up"]) and not any(r["movers_dn"]), k
        assert all(r[f] != r[f] for f in ("movers_up_share", "movers_dn_share", "secret_loss_share")), k
        assert r["secret_in_losers"] == 0.0 and r["decoy_in_gainers"] == 0.0


def test_switch_off_launches_nothing_and_keeps_the_records(movers_sweeps):
    from test_engine_gpu import FIELDS, _assert_records_equal

    out, runners, calls, _ = movers_sweeps
    r0, pairs = runners["switch_off"]
    assert calls["switch_off"] == 0 and not r0.output_movers and all(p.x_base is None for p in pairs)
    assert "movers_rows" not in r0.stats and "shift_base_pass_rows" not in r0.stats
    for k, r in out["switch_off"].items():
        assert set(out["default"][k]) - set(r) == set(NEW_KEYS) and not set(r) - set(out["default"][k]), k
        for f in r:                                          # every pre-existing field, bit for bit
            assert _same(r[f], out["default"][k][f]), (k, f)
    _assert_records_equal(out["switch_off"], out["default"],
                          fields=FIELDS + ("decoy_probs", "p_secret_final", "p_secret_max", "nll_self"))


def test_shift_and_movers_share_one_baseline_unembedding(movers_sweeps):
    """With both switches the ``kl_*`` fields are the shift-only run's, bit for bit, the movers fields the
    movers-only run's, and the model's unembedding runs as often as in the shift-only run: one baseline unembedding
    per head sub-chunk serves both kernels."""
    from test_head_shift_cpu import KEYS

    out, runners, calls, unembeds = movers_sweeps
    assert calls["both"] > 0 and calls["shift_only"] == 0
    assert unembeds["both"] == unembeds["shift_only"] > unembeds["switch_off"]
    assert unembeds["default"] <= unembeds["shift_only"]         # movers alone: only sub-chunks with a selected row
    for k, r in out["both"].items():
        for f in KEYS:
            assert r[f] == out["shift_only"][k][f], (k, f)
        for f in NEW_KEYS:
            assert _same(r[f], out["default"][k][f]), (k, f)
        assert set(r) == set(out["shift_only"][k]) | set(NEW_KEYS)
    assert not any(f in r for r in out["default"].values() for f in KEYS)
