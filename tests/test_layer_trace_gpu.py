"""Layer trace on the MI355X: ``ops.lens_track`` (csrc/lens_track.hip) against the derived criterion of
tests/layer_trace_cases.py at every row shape, exact zeros for skipped rows and absent ids, the independence of a
row's bits from the launch around it, the inputs that raise, and the sweep with ``intervention.layer_trace`` across its
reuse levels."""
from dataclasses import replace

import pytest
import torch

from layer_trace_cases import EPS, TRACE_CAPS, TRACE_D, TRACE_T, TRACE_U, run_trace, trace_case
from taboo_brittleness_amd import ops
from taboo_brittleness_amd.models.gemma2 import Gemma2Model
from taboo_brittleness_amd.models.spec import GEMMA2_TINY
from taboo_brittleness_amd.models.weights import random_gemma2
from test_layer_trace_cpu import KEYS, LISTS

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SPEC = replace(GEMMA2_TINY, vocab_size=2048, layers=4, sliding_window=8)      # the SPEC of tests/test_head_shift_gpu.py


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("D", TRACE_D)
@pytest.mark.parametrize("T", TRACE_T)
def test_kernel_meets_the_criterion(gpu, D, T):
    """M in {1, 5, 257} with unsorted, repeated and out-of-range row maps, caps 0 and 30, NaN-filled outputs: every
    element within its bound, skipped rows and the absent id exactly 0.0."""
    bad = run_trace(ops.lens_track, gpu, D, T)
    assert not bad, bad[:6]


@pytest.mark.parametrize("D", TRACE_D)
@pytest.mark.parametrize("T", TRACE_T)
def test_row_bits_do_not_depend_on_the_launch(gpu, D, T):
    """One row launched alone, as row 130 of 257 rows that all share its table block (the staged-table path), with its
    neighbours' row map changed (its wave falls back to the global-memory path), and as the last row of 257 (a
    workgroup of one row): the same bits each time, at both caps."""
    h, V, _ = trace_case(D, T, 257, seed=7)
    h, V = h.to(gpu), V.to(gpu)
    row = h[130:131].contiguous()
    for cap in TRACE_CAPS:
        for u in range(TRACE_U):
            alone = ops.lens_track(row, V, torch.tensor([u], dtype=torch.int32, device=gpu), EPS, cap)
            same = torch.full((257,), u, dtype=torch.int32, device=gpu)
            mid = ops.lens_track(h, V, same, EPS, cap)
            assert torch.equal(_bits(mid[130]), _bits(alone[0])), (cap, u, "middle of 257")
            for nb in ([129], [131], [128, 129, 131], list(range(112, 130)) + list(range(131, 160))):
                vr = same.clone()
                vr[nb] = torch.tensor([(u + 1 + i) % (TRACE_U + 2) - 1 for i in range(len(nb))], dtype=torch.int32,
                                      device=gpu)                       # other blocks, -1 and U among them
                got = ops.lens_track(h, V, vr, EPS, cap)
                assert torch.equal(_bits(got[130]), _bits(alone[0])), (cap, u, nb)
            vr = same.clone()
            vr[128] = -1                                  # its workgroup's first row is skipped: nothing is staged
            h2 = h.clone()
            h2[256] = h[130]
            last = ops.lens_track(h2, V, vr, EPS, cap)
            assert torch.equal(_bits(last[256]), _bits(alone[0])), (cap, u, "last row")
            assert torch.equal(_bits(last[130]), _bits(alone[0])), (cap, u, "beside a skipped row")


def test_unsupported_inputs_raise(gpu):
    h = torch.zeros(4, 64, dtype=BF, device=gpu)
    V = torch.zeros(2, 3, 64, device=gpu)
    vr = torch.zeros(4, dtype=torch.int32, device=gpu)
    out = ops.lens_track(h, V, vr, EPS, 30.0)
    assert out.shape == (4, 3) and not _bits(out).any()                  # zero rows: exactly 0.0
    for bad in (dict(V=V.cpu()), dict(vr=vr.long()), dict(V=V[:, :, :32].contiguous()), dict(h=h.float()),
                dict(V=torch.zeros(2, 9, 64, device=gpu)), dict(V=torch.zeros(2, 0, 64, device=gpu)),
                dict(h=torch.zeros(4, 60, dtype=BF, device=gpu), V=torch.zeros(2, 3, 60, device=gpu)),
                dict(h=torch.zeros(4, 4104, dtype=BF, device=gpu), V=torch.zeros(2, 3, 4104, device=gpu)),
                dict(out=torch.zeros(4, 2, device=gpu))):
        with pytest.raises(ValueError):
            ops.lens_track(bad.get("h", h), bad.get("V", V), bad.get("vr", vr), EPS, 30.0, out=bad.get("out"))
    assert ops.lens_track(h[:0], V, vr[:0], EPS, 30.0).numel() == 0
    none = ops.lens_track(h, V[:0], vr, EPS, 30.0)                       # U = 0: every row is out of range
    assert not _bits(none).any()


# -------------------------------------------------------------------------------------------------- sweep
METHODS = ("sae_targeted", "sae_random", "proj_targeted")


@pytest.fixture(scope="module")
def trace_sweeps(gpu):
    """The tiny-model sweep (in-tree GEMMs: batch-invariant) with ``intervention.layer_trace`` at every reuse level
    switched one at a time, an all-no-op run forced through the tail, and a run without the switch under a spy on
    ``ops.lens_track``; computed once."""
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from taboo_brittleness_amd.runtime import gemm_dispatch as GD

    old = GD.mode()
    GD.set_mode("tb")
    base = ["experiment.max_new_tokens=12", "intervention.budgets=[1, 4]", "intervention.ranks=[1, 4]",
            "intervention.random_trials=2", "intervention.proj_random_trials=1"]
    tr = ["intervention.layer_trace=true"]
    mg = Gemma2Model(random_gemma2(SPEC, dtype=BF, seed=5, norm_std=0.1, device=gpu, post_norm_gain=8.0), gpu)
    tok = SyntheticTokenizer(vocab_size=SPEC.vocab_size)
    key = lambda r: (r["word"], r["prompt_idx"], r["method"], r["budget"], r["trial"])   # noqa: E731
    out, runners, calls = {}, {}, {}
    real = ops.lens_track
    try:
        for name, extra, flags in (("default", tr, {}), ("no_skip", tr, dict(skip_noop_spikes=False)),
                                   ("no_trie", tr, dict(trie_decode=False)), ("no_dedup", tr, dict(_no_dedup=True)),
                                   ("noop", tr + ["intervention.alpha=0.0"], dict(skip_noop_spikes=False)),
                                   ("switch_off", [], {})):
            cfg = load_config(None, base + extra)
            sae = JumpReLUSAE.random(SPEC.hidden, 1024, seed=2, device=gpu)
            r = SweepRunner(cfg, mg, tok, sae, batch=64, device=gpu, layer=2, kv_pairs=8)
            for k, v in flags.items():
                if k == "_no_dedup":                     # lens rows one by one, the trie decode still on
                    r._lens_row_keys = lambda *a, **kw: None
                else:
                    setattr(r, k, v)
            n = [0]

            def spy(*a, _n=n, **kw):
                _n[0] += 1
                return real(*a, **kw)

            ops.lens_track = spy
            methods = ("sae_targeted",) if name == "noop" else METHODS
            pairs = r.build_pairs(["ship"], cfg.prompts[:3], methods)
            r.run_baselines(pairs)
            res = r.run_cells(pairs, r.make_cells(pairs, methods))
            out[name] = {key(x): x for x in res}
            runners[name] = (r, pairs)
            calls[name] = n[0]
    finally:
        ops.lens_track = real
        GD.set_mode(old)
    return out, runners, calls


def test_sweep_fields_are_bit_equal_across_reuse_levels(trace_sweeps):
    """The no-op spike skip, the prefix-trie decode and the lens row dedup change which rows share a launch, never a
    row's bits: the trace fields are equal as floats, bit for bit (nan where both are nan)."""
    out, runners, calls = trace_sweeps
    ref_ = out["default"]
    st = runners["default"][0].stats
    assert st["tf_rows"] > 0 and st["diverged"] > 0 and calls["default"] > 0 and st["trace_rows"] == 2 * st["tf_rows"]
    assert runners["no_skip"][0].stats["tf_rows"] > st["tf_rows"]              # the skip did skip rows
    for name in ("no_skip", "no_trie", "no_dedup"):
        assert set(out[name]) == set(ref_)
        for k, r in out[name].items():
            assert r["response_ids"] == ref_[k]["response_ids"], (name, k)
            for f in KEYS:
                a, b = r[f], ref_[k][f]
                assert a == b or (a != a and b != b), (name, k, f, a, b)
    assert any(abs(r["trace_dz_spike"][0]) > 1e-3 for r in ref_.values())
    assert all(len(r[f]) == 2 for r in ref_.values() for f in LISTS)


def test_noop_cells_through_the_tail_are_exactly_zero(trace_sweeps):
    """``alpha = 0`` makes every edit an exact no-op; with the skip off the cells still run their tail from the first
    spike, in a batch of their own shape.  Its rows repeat the baseline pass's bits at every block, so every
    difference is exactly 0."""
    out, runners, calls = trace_sweeps
    r_, pairs = runners["noop"]
    assert r_.stats["tf_rows"] > 0 and r_.stats["diverged"] == 0 and calls["noop"] > 0 and len(out["noop"]) == 3 * 2
    base = {(p.word, p.pidx): p for p in pairs}
    for k, r in out["noop"].items():
        assert r["response_ids"] == base[k[0], k[1]].resp
        assert all(v == 0.0 for f in LISTS if f != "trace_z_base_spike" for v in r[f]), (k, [r[f] for f in LISTS])
        assert r["trace_recovery"] != r["trace_recovery"] and any(v != 0.0 for v in r["trace_z_base_spike"])


def test_switch_off_launches_nothing_and_keeps_the_records(trace_sweeps):
    from test_engine_gpu import FIELDS, _assert_records_equal

    out, runners, calls = trace_sweeps
    r0, pairs = runners["switch_off"]
    assert calls["switch_off"] == 0 and not r0.layer_trace and all(p.z_base is None and p.x_base is None for p in pairs)
    assert not any(k.startswith("trace_") or k.startswith("shift_") for k in r0.stats)
    for k, r in out["switch_off"].items():
        assert set(out["default"][k]) - set(r) == set(KEYS) and not set(r) - set(out["default"][k]), k
    _assert_records_equal(out["switch_off"], out["default"],
                          fields=FIELDS + ("decoy_probs", "p_secret_final", "p_secret_max", "nll_self"))
