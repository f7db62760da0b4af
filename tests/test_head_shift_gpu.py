"""Output shift on the MI355X: ``ops.head_shift`` (csrc/lens.hip head_shift_kernel) against the criteria of
tests/shift_cases.py at every stream width, the exact zero of identical rows, the independence of a row's bits from
the launch around it, the inputs that raise, and the sweep with ``intervention.output_shift`` across its reuse
levels."""
from dataclasses import replace

import pytest
import torch

from readout_cases import STREAM_WIDTHS
from shift_cases import SHIFT_CAPS, run_shift, shift_case
from taboo_brittleness_amd import ops
from taboo_brittleness_amd.models.gemma2 import Gemma2Model
from taboo_brittleness_amd.models.spec import GEMMA2_TINY
from taboo_brittleness_amd.models.weights import random_gemma2
from test_head_shift_cpu import KEYS

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SPEC = replace(GEMMA2_TINY, vocab_size=2048, layers=4, sliding_window=8)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("V", STREAM_WIDTHS)
def test_kernel_meets_the_criteria(gpu, V):
    """Every kind of row pair, R in {1, 3, 5} against two baseline rows, caps 30 and 40, NaN-filled outputs."""
    run_shift(ops.head_shift, gpu, V).assert_ok(f"head_shift kernel V {V}")


@pytest.mark.parametrize("V", STREAM_WIDTHS)
def test_identical_rows_give_exact_zero(gpu, V):
    """Rows of equal bits -- random, saturated, and at the far rows of a table, where odd widths misalign the two
    rows differently -- give +0.0 twice, bit for bit."""
    g = torch.Generator().manual_seed(V)
    base = torch.cat([4 * torch.randn(3, V, generator=g), 100 * torch.randn(2, V, generator=g)]).to(BF).to(gpu)
    rm = torch.tensor([4, 0, 3, 1, 2, 2, 0], dtype=torch.int32, device=gpu)
    logits = base[rm.long()].contiguous()
    for cap in SHIFT_CAPS:
        kl = torch.full((7,), float("nan"), device=gpu)
        klr = torch.full((7,), float("nan"), device=gpu)
        ops.head_shift(logits, base, rm, cap, kl, klr)
        assert not _bits(kl).any() and not _bits(klr).any(), (cap, kl, klr)


@pytest.mark.parametrize("V", (9, 4104, 16397, 32795))
def test_row_bits_do_not_depend_on_the_launch(gpu, V):
    """One (edited row, baseline row) pair launched alone, as row 3 of 5 against a larger table, through a permuted
    rowmap, and among more rows than the persistent grid has workgroups: the same bits each time."""
    z, y, _rm, _ = shift_case(V, "gain16", 5)
    z, y = z.to(gpu), y.to(gpu)
    g = torch.Generator().manual_seed(5 * V)
    more = (4 * torch.randn(4, V, generator=g)).to(BF).to(gpu)
    for cap in SHIFT_CAPS:
        alone = ops.head_shift(z[2:3].contiguous(), y[1:2].contiguous(), torch.zeros(1, dtype=torch.int32, device=gpu), cap)
        tab = torch.cat([more[:2], y[1:2], more[2:]]).contiguous()                # the baseline row is row 2 of 5
        lg5 = torch.cat([more[:3], z[2:3], more[3:]]).contiguous()                # the edited row is row 3 of 5
        for rm in ([0, 1, 3, 2, 4], [4, 3, -1, 2, 2]):
            got = ops.head_shift(lg5, tab, torch.tensor(rm, dtype=torch.int32, device=gpu), cap)
            for a, b in zip(alone, got):
                assert torch.equal(_bits(a[0]), _bits(b[3])), (cap, rm)
        if V <= 4104:
            R = 1100                                                              # > 2 workgroups per CU
            big = z[2:3].expand(R, V).contiguous()
            rmb = torch.zeros(R, dtype=torch.int32, device=gpu)
            got = ops.head_shift(big, y[1:2].contiguous(), rmb, cap)
            for a, b in zip(alone, got):
                assert bool((_bits(b) == _bits(a[0])).all()), cap


def test_unsupported_inputs_raise(gpu):
    lg = torch.zeros(2, 64, dtype=BF, device=gpu)
    rm = torch.zeros(2, dtype=torch.int32, device=gpu)
    kl, klr = ops.head_shift(lg, lg, rm, 30.0)
    assert not kl.any() and not klr.any()
    for cap in (0.0, -1.0, 50.0):                                                  # no f kernel for these
        with pytest.raises((RuntimeError, ValueError)):
            ops.head_shift(lg, lg, rm, cap)
    with pytest.raises((RuntimeError, ValueError)):
        ops.head_shift(lg, lg.cpu(), rm, 30.0)
    with pytest.raises((RuntimeError, ValueError)):
        ops.head_shift(lg, lg[:, :32].contiguous(), rm, 30.0)
    with pytest.raises((RuntimeError, ValueError)):
        ops.head_shift(lg, lg, rm.long(), 30.0)
    e = ops.head_shift(lg[:0], lg, rm[:0], 30.0)
    assert e[0].numel() == 0 and e[1].numel() == 0


# -------------------------------------------------------------------------------------------------- sweep
METHODS = ("sae_targeted", "sae_random", "proj_targeted")


@pytest.fixture(scope="module")
def shift_sweeps(gpu):
    """The tiny-model sweep (in-tree GEMMs: batch-invariant) with ``intervention.output_shift`` at every reuse level
    switched one at a time, an all-no-op run forced through the tail, and a run without the switch under a spy on
    ``ops.head_shift``; computed once."""
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from taboo_brittleness_amd.runtime import gemm_dispatch as GD

    old = GD.mode()
    GD.set_mode("tb")
    base = ["experiment.max_new_tokens=12", "intervention.budgets=[1, 4]", "intervention.ranks=[1, 4]",
            "intervention.random_trials=2", "intervention.proj_random_trials=1"]
    sh = ["intervention.output_shift=true"]
    mg = Gemma2Model(random_gemma2(SPEC, dtype=BF, seed=5, norm_std=0.1, device=gpu, post_norm_gain=8.0), gpu)
    tok = SyntheticTokenizer(vocab_size=SPEC.vocab_size)
    key = lambda r: (r["word"], r["prompt_idx"], r["method"], r["budget"], r["trial"])   # noqa: E731
    out, runners, calls = {}, {}, {}
    real = ops.head_shift
    try:
        for name, extra, flags in (("default", sh, {}), ("no_skip", sh, dict(skip_noop_spikes=False)),
                                   ("no_trie", sh, dict(trie_decode=False)), ("no_dedup", sh, dict(_no_dedup=True)),
                                   ("noop", sh + ["intervention.alpha=0.0"], dict(skip_noop_spikes=False)),
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

            ops.head_shift = spy
            methods = ("sae_targeted",) if name == "noop" else METHODS
            pairs = r.build_pairs(["ship"], cfg.prompts[:3], methods)
            r.run_baselines(pairs)
            res = r.run_cells(pairs, r.make_cells(pairs, methods))
            out[name] = {key(x): x for x in res}
            runners[name] = (r, pairs)
            calls[name] = n[0]
    finally:
        ops.head_shift = real
        GD.set_mode(old)
    return out, runners, calls


def test_sweep_fields_are_bit_equal_across_reuse_levels(shift_sweeps):
    """The no-op spike skip, the prefix-trie decode and the lens row dedup change which rows share a launch, never a
    row's bits: the four fields are equal as floats, bit for bit."""
    out, runners, calls = shift_sweeps
    ref_ = out["default"]
    st = runners["default"][0].stats
    assert st["tf_rows"] > 0 and st["diverged"] > 0 and calls["default"] > 0
    assert runners["no_skip"][0].stats["tf_rows"] > st["tf_rows"]              # the skip did skip rows
    for name in ("no_skip", "no_trie", "no_dedup"):
        assert set(out[name]) == set(ref_)
        for k, r in out[name].items():
            assert r["response_ids"] == ref_[k]["response_ids"], (name, k)
            for f in KEYS:
                assert r[f] == ref_[k][f], (name, k, f, r[f], ref_[k][f])
    assert any(r["kl_out_mean"] > 1e-4 for r in ref_.values())
    for r in ref_.values():
        assert r["kl_out_max"] >= r["kl_out_mean"] and r["kl_out_max"] >= 0.0


def test_noop_cells_through_the_tail_are_exactly_zero(shift_sweeps):
    """``alpha = 0`` makes every edit an exact no-op; with the skip off the cells still run their tail from the first
    spike, in a batch of their own shape.  Its rows repeat the baseline pass's bits, so every KL is exactly 0."""
    out, runners, calls = shift_sweeps
    r_, pairs = runners["noop"]
    assert r_.stats["tf_rows"] > 0 and r_.stats["diverged"] == 0 and calls["noop"] > 0 and len(out["noop"]) == 3 * 2
    base = {(p.word, p.pidx): p for p in pairs}
    for k, r in out["noop"].items():
        assert r["response_ids"] == base[k[0], k[1]].resp
        assert all(r[f] == 0.0 for f in KEYS), (k, [r[f] for f in KEYS])


def test_switch_off_launches_nothing_and_keeps_the_records(shift_sweeps, gpu):
    from taboo_brittleness_amd.runtime.generation import Generator
    from test_engine_gpu import FIELDS, _assert_records_equal

    out, runners, calls = shift_sweeps
    r0, pairs = runners["switch_off"]
    assert calls["switch_off"] == 0 and not r0.output_shift and all(p.x_base is None for p in pairs)
    assert "shift_base_rows" not in r0.stats
    for k, r in out["switch_off"].items():
        assert set(out["default"][k]) - set(r) == set(KEYS) and not set(r) - set(out["default"][k]), k
    _assert_records_equal(out["switch_off"], out["default"],
                          fields=FIELDS + ("decoy_probs", "p_secret_final", "p_secret_max", "nll_self"))
    real, n = ops.head_shift, [0]

    def spy(*a, **kw):
        n[0] += 1
        return real(*a, **kw)

    ops.head_shift = spy
    try:
        Generator(r0.m, 2, 32, use_graphs=False, stop_ids=(100_000,)).generate([[2, 5, 9], [2, 7, 8, 3]], 4)
    finally:
        ops.head_shift = real
    assert n[0] == 0
