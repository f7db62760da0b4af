"""Output-side readout on the MI355X: ``ops.decode_head_track`` (csrc/lens.hip decode_head_track_kernel) against its
reference, its bit identities with ``ops.decode_head``, batch invariance, the ``col`` / ``W`` form, the generator's
tracked decode inside a captured graph, and the sweep's reuse levels with ``intervention.output_readout``."""
from dataclasses import replace

import pytest
import torch

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.models.gemma2 import Gemma2Model
from taboo_brittleness_amd.models.spec import GEMMA2_TINY
from taboo_brittleness_amd.models.weights import random_gemma2
from taboo_brittleness_amd.ops import reference as ref
from test_head_track_cpu import NEW_KEYS, planted_case

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CAP = 30.0
SPEC = replace(GEMMA2_TINY, vocab_size=2048, layers=4, sliding_window=8)
# the V % 8 tail and unaligned rows; more rows than the persistent grid; two vocab sizes whose 16-B chunk count ends
# inside a wave on the boundary trip of the 4-deep stream (lanes of one wave then run different trips: the count
# must not depend on which lanes are active) -- 8 * 1636 + 3 with a tail, 128256 without
SHAPES = [(6, 4099 * 8 + 5), (600, 256000), (6, 8 * 1636 + 3), (6, 128256)]


@pytest.fixture(scope="module")
def cases(gpu):
    """Per shape: logits, tracked ids, teacher targets (host and device) and the plain kernel's outputs, once."""
    out = {}
    for R, V in SHAPES:
        lg, track = planted_case(R, V)
        tgt = torch.randint(-1, V, (R,), generator=torch.Generator().manual_seed(R), dtype=torch.int32)
        g = dict(lg=lg.to(gpu), track=track.to(gpu), tgt=tgt.to(gpu))
        plain = ops.decode_head(g["lg"], CAP, g["tgt"])
        lp_ref, rk_ref = ref.head_track(lg, CAP, track, 8)             # n_rank < 8: the same with -1 from n_rank on
        out[(R, V)] = dict(lg=lg, track=track, tgt=tgt, g=g, plain=plain, lp_ref=lp_ref, rk_ref=rk_ref)
    return out


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n_rank", [0, 2, 8])
def test_matches_reference(cases, shape, n_rank):
    """``rank`` is the integer count on the reference's capped values, exactly; ``logp`` within test_decode_head's
    NLL tolerance (the fp32 exp-sum order differs from torch.logsumexp); empty / unranked columns give 0 / -1."""
    c = cases[shape]
    g = c["g"]
    nxt, ns, nt, logp, rank = ops.decode_head_track(g["lg"], CAP, g["track"], n_rank, g["tgt"])
    lp_ref, rk_ref = c["lp_ref"], c["rk_ref"].clone()
    rk_ref[:, n_rank:] = -1
    assert torch.equal(rank.cpu(), rk_ref)
    torch.testing.assert_close(logp.cpu(), lp_ref, atol=2e-3, rtol=1e-4)
    empty = (c["track"] < 0) | (c["track"] >= shape[1])
    assert bool((logp.cpu()[empty] == 0).all()) and bool((rank.cpu()[empty] == -1).all())
    assert bool((rank.cpu()[:, n_rank:] == -1).all())
    if n_rank >= 2:
        # planted: column 0 is the row's argmax, column 1 a saturated logit tied with another (tie not counted)
        assert bool((rank.cpu()[:, 0] == 0).all()) and int(rank[0, 1]) == 0
    if n_rank == 8:
        assert bool((rank.cpu()[~empty] >= 0).all()) and int(rank.max()) > 0
        assert torch.equal(rank[:, 6], rank[:, 7])                # the duplicated id


@pytest.mark.parametrize("shape", SHAPES)
def test_bit_identities_with_decode_head(cases, shape):
    c = cases[shape]
    g = c["g"]
    p_nxt, p_ns, p_nt = c["plain"]
    for n_rank in (0, 2, 8):
        nxt, ns, nt, logp, rank = ops.decode_head_track(g["lg"], CAP, g["track"], n_rank, g["tgt"])
        assert torch.equal(nxt, p_nxt) and torch.equal(ns, p_ns) and torch.equal(nt, p_nt), n_rank
    for k in range(8):
        tk = g["track"][:, k].contiguous()
        want = -ops.decode_head(g["lg"], CAP, tk)[2]
        want = torch.where((tk >= 0) & (tk < shape[1]), want, torch.zeros_like(want))      # -0.0 -> 0.0
        assert torch.equal(logp[:, k], want), k
    # without a teacher
    nxt, ns, nt, lp2, rk2 = ops.decode_head_track(g["lg"], CAP, g["track"], 8)
    assert nt is None and torch.equal(nxt, p_nxt) and torch.equal(ns, p_ns)
    assert torch.equal(lp2, logp) and torch.equal(rk2, rank)


def test_batch_invariance(cases):
    """A row alone and inside the 600-row batch: equal bits for all five outputs."""
    c = cases[SHAPES[1]]
    g = c["g"]
    full = ops.decode_head_track(g["lg"], CAP, g["track"], 8, g["tgt"])
    for r in (0, 3, 511, 512, 599):
        one = ops.decode_head_track(g["lg"][r:r + 1], CAP, g["track"][r:r + 1], 8, g["tgt"][r:r + 1])
        for a, b in zip(one, full):
            assert torch.equal(a[0], b[r]), r


def test_col_form_writes_one_column(cases, gpu):
    c = cases[SHAPES[0]]
    g = c["g"]
    R, W, T = 6, 5, 8
    _, _, _, logp, rank = ops.decode_head_track(g["lg"], CAP, g["track"], 8)
    col = torch.tensor([0, 4, 2, 9, 5, 1], dtype=torch.int64, device=gpu)          # 9, 5 -> W - 1
    lw = torch.full((R, W, T), 7.5, dtype=torch.float32, device=gpu)
    rw = torch.full((R, W, T), -7, dtype=torch.int32, device=gpu)
    out = ops.decode_head_track(g["lg"], CAP, g["track"], 8, logp=lw, rank=rw, col=col)
    assert out[3] is lw and out[4] is rw
    for r in range(R):
        cc = min(int(col[r]), W - 1)
        assert torch.equal(lw[r, cc], logp[r]) and torch.equal(rw[r, cc], rank[r])
        others = [i for i in range(W) if i != cc]
        assert bool((lw[r, others] == 7.5).all()) and bool((rw[r, others] == -7).all())


def test_unsupported_inputs_raise(gpu):
    lg = torch.zeros(2, 64, dtype=BF, device=gpu)
    tk = torch.zeros(2, 8, dtype=torch.int32, device=gpu)
    ops.decode_head_track(lg, CAP, tk, 2)
    with pytest.raises((RuntimeError, ValueError)):
        ops.decode_head_track(lg, 0.0, tk, 2)                                       # no softcap: no f kernel
    with pytest.raises((RuntimeError, ValueError)):
        ops.decode_head_track(lg, 50.0, tk, 2)                                      # cap above the f kernel's range
    with pytest.raises((RuntimeError, ValueError)):
        ops.decode_head_track(lg, CAP, torch.zeros(2, 9, dtype=torch.int32, device=gpu), 2)     # T > 8
    with pytest.raises((RuntimeError, ValueError)):
        ops.decode_head_track(lg, CAP, tk[:, :4].contiguous(), 5)                   # n_rank > T
    with pytest.raises((RuntimeError, ValueError)):
        ops.decode_head_track(torch.zeros(2, 128, dtype=BF, device=gpu)[:, :64], CAP, tk, 2)     # non-contiguous


# ------------------------------------------------------------------------------------------------- engine
def _models(gpu, **kw):
    return Gemma2Model(random_gemma2(SPEC, dtype=BF, seed=5, norm_std=0.1, device=gpu, **kw), gpu)


PROMPTS = [[2, 5, 9, 11, 13], [2, 5, 9, 11, 13], [2, 7, 8], [2, 3, 4, 5, 6, 7, 8]]
TRACK = [[5, 9, 11, 13, 100, 2047, 0, -1], [7, 8], [5, 9, 11, 13, 100, 2047, 0, 1], []]


def test_graph_decode_equals_eager_and_untracked(gpu):
    """``tok_logp`` / ``tok_rank`` of a captured-and-replayed decode equal the eager decode's bits; tokens and NLLs
    equal those of a generator without tracking (whose outputs carry no readout); each column is the readout of the
    distribution that chose that column's token."""
    from taboo_brittleness_amd.runtime.generation import Generator

    mg = _models(gpu)
    kw = dict(use_graphs=False, stop_ids=(100_000,))
    plain = Generator(mg, 4, 32, **kw).generate(PROMPTS, 10)
    assert plain.tok_logp is None and plain.tok_rank is None
    eager = Generator(mg, 4, 32, track_cols=8, **kw).generate(PROMPTS, 10, track=TRACK)
    g = Generator(mg, 4, 32, use_graphs=True, stop_ids=(100_000,), track_cols=8)
    a = g.generate(PROMPTS, 10, graph_key="k", track=TRACK)
    b = g.generate(PROMPTS, 10, graph_key="k", track=TRACK)           # replay path
    assert any(k[-1] == "track" for k in g._graphs)
    for o in (eager, a, b):
        assert torch.equal(o.tokens[:, :10], plain.tokens[:, :10])
        assert torch.equal(o.tok_nll[:, :10], plain.tok_nll[:, :10])
        assert torch.equal(o.tok_logp, eager.tok_logp) and torch.equal(o.tok_rank, eager.tok_rank)
    lp, rk = eager.tok_logp.cpu(), eager.tok_rank.cpu()
    assert lp.shape == (4, 10, 8) and bool((rk[:, :, 2:] == -1).all())
    assert bool((lp[0, :, 7] == 0).all()) and bool((rk[3] == -1).all()) and bool((lp[3] == 0).all())
    assert bool((lp[0, :, :7] < 0).all()) and bool((rk[:3, :, :2] >= 0).all())
    # a tracked id that is the chosen token has rank 0 and logp = -NLL of that token
    toks, nll = eager.tokens.cpu(), eager.tok_nll.cpu()
    row = Generator(mg, 4, 32, track_cols=1, track_rank=1, **kw).generate(
        PROMPTS, 10, track=[[int(toks[i, 4])] for i in range(4)])
    assert bool((row.tok_rank[:, 4, 0] == 0).all())
    assert torch.equal(row.tok_logp[:, 4, 0].cpu(), -nll[:, 4])


def test_tracking_needs_the_logits_head(gpu):
    from taboo_brittleness_amd.runtime.generation import Generator

    mg = _models(gpu)
    mg.fused_head = True
    with pytest.raises(ValueError, match="fused-head"):
        Generator(mg, 4, 32, track_cols=2)
    mg.fused_head = False
    with pytest.raises(ValueError):
        Generator(mg, 4, 32, track_cols=9)
    with pytest.raises(ValueError):
        Generator(mg, 4, 32).generate(PROMPTS, 2, track=TRACK)


# -------------------------------------------------------------------------------------------------- sweep
SWAP = ("sae_swap", "sae_swap_random", "proj_swap", "proj_swap_random")
SWEEP_METHODS = ("sae_targeted", "sae_random", "proj_targeted") + SWAP


@pytest.fixture(scope="module")
def readout_sweeps(gpu):
    """The harness of test_interchange_gpu.py::swap_sweeps with ``intervention.output_readout``: from scratch, with
    every reuse level, and the switch off (in-tree GEMMs: batch-invariant), computed once."""
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from taboo_brittleness_amd.runtime import gemm_dispatch as GD

    old = GD.mode()
    GD.set_mode("tb")
    base = ["experiment.max_new_tokens=12", "intervention.budgets=[1, 4]", "intervention.ranks=[1, 4]",
            "intervention.random_trials=2", "intervention.proj_random_trials=1"]
    ro = ["intervention.output_readout=true"]
    on, off = dict(prefix_share=True, layer_resume=True), dict(prefix_share=False, layer_resume=False)
    mg = _models(gpu, post_norm_gain=8.0)
    tok = SyntheticTokenizer(vocab_size=SPEC.vocab_size)
    key = lambda r: (r["word"], r["prompt_idx"], r["method"], r["budget"], r["trial"])   # noqa: E731
    out, runners = {}, {}
    try:
        for name, extra, kw in (("scratch", ro, off), ("reuse", ro, on), ("switch_off", [], on),
                                ("noop", ro + ["intervention.alpha=0.0"], on)):
            cfg = load_config(None, base + extra)
            sae = JumpReLUSAE.random(SPEC.hidden, 1024, seed=2, device=gpu)
            r = SweepRunner(cfg, mg, tok, sae, batch=96, device=gpu, layer=2, kv_pairs=8, **kw)
            methods = ("sae_targeted",) if name == "noop" else SWEEP_METHODS
            r.skip_noop_spikes = name != "noop"
            pairs = r.build_pairs(["ship", "moon"], cfg.prompts[:3], methods)
            r.run_baselines(pairs)
            res = r.run_cells(pairs, r.make_cells(pairs, methods))
            out[name] = {key(x): x for x in res}
            runners[name] = (r, pairs)
    finally:
        GD.set_mode(old)
    return out, runners


def test_sweep_reuse_is_exact_with_the_readout(readout_sweeps):
    """Every reuse level on (layer resume, trie decode, no-op skip, ride-along baselines) against from scratch: the
    new fields bit-equal, the rest to the criteria of test_sweep_gpu_swap_reuse_is_exact."""
    from test_engine_gpu import FIELDS, _assert_records_equal
    from test_head_track_cpu import DONOR_KEYS

    out, runners = readout_sweeps
    st = runners["reuse"][0].stats
    assert st["tf_rows"] > 0 and st["diverged"] > 0
    assert runners["reuse"][0].gen.track_cols == len(runners["reuse"][1][0].track)
    _assert_records_equal(out["scratch"], out["reuse"], float_rtol=1e-6,
                          fields=FIELDS + ("p_donor_mean", "p_donor_final", "p_donor_max", "delta_p_donor"))
    _assert_records_equal(out["scratch"], out["reuse"], fields=NEW_KEYS + DONOR_KEYS)          # bit-equal
    for k, r in out["reuse"].items():
        assert set(NEW_KEYS) <= set(r) and (set(DONOR_KEYS) <= set(r)) == (k[2] in SWAP), k
        assert r["logp_out_max"] >= r["logp_out_mean"] and r["logp_out_max"] < 0.0 and r["rank_out_min"] >= 0
        assert r["delta_logp_out"] == r["logp_out_mean"] - r["logp_out_mean_base"]
    assert any(r["delta_logp_out"] != 0.0 for r in out["reuse"].values())


def test_noop_cell_carries_its_baseline(readout_sweeps):
    """``alpha = 0`` makes every edit an exact no-op.  With the no-op spike skip off the cells still run their
    teacher-forced tail from the first spike; its rows, like the baseline's decode, give the baseline's bits."""
    out, runners = readout_sweeps
    r_, pairs = runners["noop"]
    assert r_.stats["tf_rows"] > 0 and r_.stats["diverged"] == 0 and len(out["noop"]) == 6 * 2
    base = {(p.word, p.pidx): p for p in pairs}
    for k, r in out["noop"].items():
        p = base[k[0], k[1]]
        want = r_._out_fields(p, p.out_logp[: len(p.resp)], p.out_rank[: len(p.resp)])
        assert r["response_ids"] == p.resp and r["delta_logp_out"] == 0.0
        assert all(r[f] == want[f] or (r[f] != r[f] and want[f] != want[f]) for f in want), (k, r, want)


def test_switch_off_keeps_the_old_keys(readout_sweeps):
    from test_engine_gpu import FIELDS, _assert_records_equal
    from test_head_track_cpu import DONOR_KEYS

    out, runners = readout_sweeps
    r0, pairs = runners["switch_off"]
    assert r0.gen.track_cols == 0 and r0.gen.out_logp is None and all(p.out_logp is None for p in pairs)
    assert not any(k[-1] == "track" for k in r0.gen._graphs)
    for k, r in out["switch_off"].items():
        assert set(out["reuse"][k]) - set(r) == set(NEW_KEYS) | (set(DONOR_KEYS) if k[2] in SWAP else set()), k
        assert not set(r) - set(out["reuse"][k])
    # the readout changes no other number
    _assert_records_equal(out["switch_off"], out["reuse"],
                          fields=FIELDS + ("decoy_probs", "p_secret_final", "p_secret_max", "nll_self", "p_donor_mean"))
