"""Causal latent ranking on CPU: the ``latent_effect`` reference (explicit ablation) against the closed form, its
first-order limit and edge cases, and ``intervention.latent_score = effect_lens | attr_model`` through the sweep."""
import json
import os
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.config import load_config
from taboo_brittleness_amd.ops import reference as ref

BF = torch.bfloat16
EPS = 1e-6
SEG = [0, 1, 4, 4, 5]          # segments of 1 row, 3 rows, 0 rows and 1 row
ROWS = 5                       # row 0 all-silent, row 1 one active latent, row 2 ~40 % active, rows 3, 4 sparse


def effect_case(D, L, seed=0, table=torch.float32):
    """Five spike rows of every activity class over a unit-row decoder (``SEG`` groups them); ``V`` holds one row
    per spike row (``V[:1]`` is the broadcast form).  Sizes chosen so the effects are of order 1e-3 .. 1e-1."""
    g = torch.Generator().manual_seed(1000 * seed + D + L)
    Wd = torch.randn(L, D, generator=g)
    Wd = (Wd / Wd.norm(dim=1, keepdim=True)).to(table)
    X = torch.randn(ROWS, D, generator=g).to(BF)
    V = torch.randn(ROWS, D, generator=g) * 0.05
    a = torch.rand(ROWS, L, generator=g) * 3.0 + 0.25
    keep = torch.zeros(ROWS, L, dtype=torch.bool)
    keep[1, L // 3] = True
    keep[2] = torch.rand(L, generator=g) < 0.4
    keep[3] = torch.rand(L, generator=g) < max(8.0 / L, 0.005)
    keep[4] = torch.rand(L, generator=g) < max(76.0 / L, 0.02)
    acts = torch.where(keep, a, torch.zeros_like(a))
    acts[3, 0] = -1.0                                   # a negative entry is silent too
    return {"acts": acts.contiguous(), "X": X, "V": V.contiguous(), "Wd": Wd.contiguous(),
            "seg": torch.tensor(SEG, dtype=torch.int32)}


def annihilated_case(D, L, table=torch.float32):
    """Row 0 is ``x = c d`` exactly for its one active latent at alpha = 1 (the edited residual is 0); every entry is
    a small multiple of 1/8, so all dot products are exact in fp32 in any order.  Row 1: the same row, other latents."""
    g = torch.Generator().manual_seed(7 + D + L)
    q8 = lambda *s: torch.randint(-8, 9, s, generator=g).float() / 8.0   # noqa: E731
    Wd = q8(L, D)
    X = q8(2, D)
    j = L // 2
    Wd[j] = X[0] / 2.0                                   # a = 2, alpha = 1: c d = x
    V = q8(2, D) / 4.0
    acts = torch.zeros(2, L)
    acts[0, j] = 2.0
    acts[1, : min(L, 6)] = torch.tensor([1.0, 0.5, 0.0, 2.0, 0.0, 1.5])[: min(L, 6)]
    return {"acts": acts, "X": X.to(BF), "V": V, "Wd": Wd.to(table).contiguous(),
            "seg": torch.tensor([0, 1, 2], dtype=torch.int32)}


def closed_form(acts, X, V, Wd, seg, alpha, eps, cap, mode, dots=torch.float64):
    """The closed form of ``latent_effect`` with the D-long dot products taken in ``dots`` and the scalar tail in
    fp64; returns ``(score, eff)`` fp64.  ``dots = float32`` is the kernel's number format in PyTorch."""
    Xf, Vf, Wf = X.to(dots), V.to(dots), Wd.to(dots)
    Vf = Vf.expand(Xf.shape[0], -1)
    D = Xf.shape[1]
    p, q, s = (Xf @ Wf.t()).double(), (Vf @ Wf.t()).double(), (Wf * Wf).sum(1).double()[None, :]
    xu, xx = (Xf * Vf).sum(1).double()[:, None], (Xf * Xf).sum(1).double()[:, None]
    c = float(alpha) * acts.double()
    f = (lambda z: cap * torch.tanh(z / cap)) if cap > 0 else (lambda z: z)
    if mode == 0:
        ss = (xx - 2 * c * p + c * c * s).clamp_min(0)
        e = f(xu / torch.sqrt(xx / D + eps)) - f((xu - c * q) / torch.sqrt(ss / D + eps))
    else:
        e = c * q
    eff = torch.where(acts > 0, e, torch.zeros_like(e))
    segs = seg.tolist()
    score = torch.stack([eff[a:b].sum(0) / max(b - a, 1) for a, b in zip(segs[:-1], segs[1:])])
    return score, eff


def _args(c, per_row=True):
    return c["acts"], c["X"], (c["V"] if per_row else c["V"][:1]), c["Wd"], c["seg"]


# ---------------------------------------------------------------------------------------------- op and reference
@pytest.mark.parametrize("D", [64, 328])
def test_reference_is_the_closed_form(D):
    """Two fp64 derivations of one quantity of size <= 0.1 (explicit ablation vs three dot products): 1e-12."""
    c = effect_case(D, 256)
    worst = 0.0
    for mode in (0, 1):
        for cap in (30.0, 0.0):
            for alpha in (1.0, 0.5, 0.0):
                for per_row in (True, False):
                    sr, er = ref.latent_effect(*_args(c, per_row), alpha, EPS, cap, mode)
                    sc, ec = closed_form(*_args(c, per_row), alpha, EPS, cap, mode)
                    worst = max(worst, float((er - ec).abs().max()), float((sr - sc).abs().max()))
                    assert er.dtype == torch.float64 and float(er.abs().max()) <= 1.0
    print(f"D={D}: max |explicit - closed form| = {worst:.3e}")
    assert worst <= 1e-12


def _lens_model(D, seed=3):
    g = torch.Generator().manual_seed(seed)
    w = SimpleNamespace(lm_head=torch.randn(32, D, generator=g) * 0.05, norm_f=torch.randn(D, generator=g) * 0.1)
    return SimpleNamespace(w=w, spec=SimpleNamespace(eps=EPS, final_softcap=30.0))


@pytest.mark.parametrize("D", [64, 328])
def test_first_order_consistency(D):
    """``effect_lens / alpha`` (cap 0) tends to ``attr`` with the lens gradient rows: the gap is second order in
    alpha, so it shrinks ~10x from alpha = 1e-2 to 1e-3 (at least 5x asserted)."""
    from taboo_brittleness_amd.interp import gradient as GR

    c = effect_case(D, 256)
    m = _lens_model(D)
    u = GR.lens_direction(m, [5]).view(1, -1)
    gl = GR.lens_gradients(m, c["X"], [5])
    _, first = ref.latent_effect(c["acts"], c["X"], gl, c["Wd"], c["seg"], 1.0, EPS, 0.0, 1)
    gap = {}
    for alpha in (1e-2, 1e-3):
        _, e = ref.latent_effect(c["acts"], c["X"], u, c["Wd"], c["seg"], alpha, EPS, 0.0, 0)
        gap[alpha] = float((e / alpha - first).abs().max())
    print(f"D={D}: first-order gap {gap}")
    assert gap[1e-2] > 0 and gap[1e-3] * 5.0 <= gap[1e-2]


def test_lens_direction_is_shared_and_checked():
    from taboo_brittleness_amd.interp import gradient as GR

    m = _lens_model(64)
    u = GR.lens_direction(m, [5, 7])
    assert torch.equal(u, (m.w.lm_head[5] + m.w.lm_head[7]).float() * (1.0 + m.w.norm_f.float()))
    with pytest.raises(ValueError):
        GR.lens_direction(m, [32])
    with pytest.raises(ValueError):
        GR.lens_direction(SimpleNamespace(w=SimpleNamespace()), [1])


def test_edge_cases():
    """Silent latents exactly 0.0, alpha = 0 all zeros, an empty segment scores 0, the annihilated row is finite."""
    c = effect_case(64, 256)
    for mode in (0, 1):
        score, eff = ops.latent_effect(*_args(c), 1.0, EPS, 30.0, mode, want_eff=True)
        assert score.dtype == eff.dtype == torch.float32 and score.shape == (4, 256) and eff.shape == (ROWS, 256)
        assert torch.all(eff[c["acts"] <= 0] == 0.0) and torch.all(eff[0] == 0.0)
        assert float(eff[c["acts"] > 0].abs().min()) > 0.0
        assert torch.all(score[2] == 0.0) and torch.all(score[0] == 0.0)
        assert torch.equal(score[3], eff[4])
        s0, e0 = ops.latent_effect(*_args(c), 0.0, EPS, 30.0, mode, want_eff=True)
        assert torch.all(s0 == 0.0) and torch.all(e0 == 0.0)
    a = annihilated_case(64, 256)
    score, eff = ref.latent_effect(*_args(a), 1.0, EPS, 30.0, 0)
    assert torch.isfinite(eff).all() and torch.isfinite(score).all()
    x, v = a["X"][0].double(), a["V"][0].double()
    want = 30.0 * torch.tanh((x @ v) / torch.sqrt(x.pow(2).mean() + EPS) / 30.0)      # the edited row reads 0
    assert abs(float(eff[0, 128]) - float(want)) <= 1e-12
    assert torch.equal(ops.latent_effect(*_args(c), 1.0, EPS, 30.0, 0), ops.latent_effect(*_args(c), 1.0, EPS, 30.0, 0))


# -------------------------------------------------------------------------------------------------- sweep (CPU)
TINY = ["model.arch=gemma2-tiny", "model.layer_idx=2", "word_plurals={ship: [ship, ships]}",
        "prompts=['Give me a hint!', 'Any hints available?', 'Tell me more.', 'One more clue?']",
        "experiment.max_new_tokens=10", "intervention.budgets=[1, 2, 4, 8]", "intervention.random_trials=1",
        "sae.d_sae=512", "runtime.batch_size=8", "runtime.device=cpu", "runtime.use_graphs=false"]
GAP = 1e-6                     # prefixes are compared where the brute-force scores of ranks m and m + 1 differ by more


def tiny_stack(device="cpu", seed=7, sae_seed=2):
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.gemma2 import Gemma2Model
    from taboo_brittleness_amd.models.spec import GEMMA2_TINY
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.models.weights import random_gemma2

    spec = replace(GEMMA2_TINY, vocab_size=1024, layers=3, hidden=256, ffn=512)
    m = Gemma2Model(random_gemma2(spec, dtype=BF, seed=seed, norm_std=0.1, device=device), device)
    return m, SyntheticTokenizer(vocab_size=spec.vocab_size), JumpReLUSAE.random(spec.hidden, 512, seed=sae_seed,
                                                                                 device=device)


def scored_runner(extra=(), device="cpu", stack=None):
    """A tiny runner with its baselines run and scored (``run_baselines`` scores the pairs it finishes)."""
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    m, tok, sae = stack or tiny_stack(device)
    cfg = load_config(None, TINY + list(extra))
    r = SweepRunner(cfg, m, tok, sae, batch=8, device=device, layer=1, use_graphs=False)
    pairs = r.build_pairs(["ship"], cfg.prompts[:4])
    r.run_baselines(pairs)
    r._score_pairs(pairs)
    return r, pairs


def brute_force_scores(r, p):
    """``[L]`` fp64: mean over the pair's spikes of the drop of the secret's softcapped lens logit when each active
    latent alone is ablated: the edited row is built, final-normed and dotted with the unembedding row."""
    m, sae = r.m, r.sae
    x = p.resid[p.spikes_rel].detach().cpu()
    acts = sae.encode(x.to(sae.device)).cpu().double()
    Wd = sae.W_dec.detach().cpu().double()
    wu = m.w.lm_head[p.track[0]].detach().cpu().double()
    gain = 1.0 + m.w.norm_f.detach().cpu().double()
    cap, eps, alpha = float(m.spec.final_softcap), float(m.spec.eps), float(r.iv.alpha)

    def logit(y):
        z = ((y * torch.rsqrt(y.pow(2).mean(-1, keepdim=True) + eps)) * gain) @ wu
        return cap * torch.tanh(z / cap) if cap > 0 else z

    out = torch.zeros(Wd.shape[0], dtype=torch.float64)
    for t in range(x.shape[0]):
        xt = x[t].double()
        J = torch.nonzero(acts[t] > 0).flatten()
        out[J] += logit(xt[None]) - logit(xt[None] - alpha * acts[t, J, None] * Wd[J])
    return out / max(x.shape[0], 1)


def check_prefixes(pairs, brute, max_skip=0.10):
    """``targeted[:m]`` is the brute-force top-m (as a set, and in order) wherever ranks m and m + 1 are more than
    ``GAP`` apart; at most ``max_skip`` of the prefixes may be too close to call."""
    n = skipped = 0
    for p, b in zip(pairs, brute):
        vals, order = torch.sort(b, descending=True, stable=True)
        for m in range(1, len(p.targeted) + 1):
            n += 1
            if float(vals[m - 1] - vals[m]) <= GAP:
                skipped += 1
                continue
            assert set(p.targeted[:m]) == set(order[:m].tolist()), (p.pidx, m)
    print(f"prefixes: {n}, skipped as ties: {skipped}")
    assert n > 0 and skipped <= max_skip * n, (n, skipped)


@pytest.fixture(scope="module")
def lens_run():
    return scored_runner(["intervention.latent_score=effect_lens"])


@pytest.fixture(scope="module")
def corr_run():
    return scored_runner()


def test_effect_lens_ranking_is_the_brute_force_ranking(lens_run, corr_run):
    r, pairs = lens_run
    brute = [brute_force_scores(r, p) for p in pairs]
    for p, b in zip(pairs, brute):
        got = r.word_scores[p.word][p.pidx].double().cpu()
        assert float((got - b).abs().max()) <= 1e-6                       # fp32 storage of an fp64 reference
        assert len(p.targeted) == 8 and p.targeted_scores == pytest.approx([float(got[j]) for j in p.targeted])
        assert p.targeted_corr is not None and len(p.targeted_corr) == 8
    check_prefixes(pairs, brute)
    _, cpairs = corr_run
    assert [p.spikes_rel for p in pairs] == [p.spikes_rel for p in cpairs]
    assert [p.targeted_corr for p in pairs] == [p.targeted for p in cpairs]
    assert any(p.targeted != q.targeted for p, q in zip(pairs, cpairs))
    assert all(q.targeted_scores is None and q.targeted_corr is None for q in cpairs)


def test_score_over_word_averages_the_new_scores(lens_run):
    from taboo_brittleness_amd.interp import analysis as A
    from taboo_brittleness_amd.pipelines.sweep import word_targeted_latents

    r, pairs = lens_run
    rw, wpairs = scored_runner(["intervention.latent_score=effect_lens", "intervention.score_over=word"])
    per_prompt = torch.stack([r.word_scores["ship"][p.pidx] for p in pairs])
    assert torch.equal(per_prompt, torch.stack([rw.word_scores["ship"][p.pidx] for p in wpairs]))
    mean = per_prompt.mean(0)
    want = A.top_latents_from_scores(mean, 8)
    assert all(p.targeted == want for p in wpairs)
    assert all(p.targeted_scores == pytest.approx([float(mean[j]) for j in want]) for p in wpairs)
    for m in (1, 4, 8):
        assert word_targeted_latents(rw, "ship", m) == want[:m] == word_targeted_latents(r, "ship", m)


def test_attr_model_scores_and_limits():
    from taboo_brittleness_amd.interp import gradient as GR

    r, pairs = scored_runner(["intervention.latent_score=attr_model", "intervention.alpha=0.5"])
    assert r.iv.subspace == "pca"
    calls = []
    orig = GR.model_gradients
    for p in pairs:
        assert getattr(p, "resid_pre", None) is not None and p.resid_pre.shape[0] == p.plen
        seq = torch.cat([p.resid_pre, p.resid], 0)
        g = orig(r.m, seq, r.layer, [p.plen + t for t in p.spikes_rel], p.track[:1]).double()
        acts = r.sae.encode(p.resid[p.spikes_rel]).double()
        want = (0.5 * acts * (g @ r.sae.W_dec.double().t())).mean(0)
        want = torch.where((acts > 0).any(0), want, torch.zeros_like(want))
        got = r.word_scores[p.word][p.pidx].double()
        assert float((got - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))
        assert float(want.abs().max()) > 0
    try:                                   # a re-score of unchanged baselines runs no backward pass
        GR.model_gradients = lambda *a, **k: calls.append(1) or orig(*a, **k)
        r._score_pairs(pairs)
    finally:
        GR.model_gradients = orig
    assert not calls
    for attr in ("tp", "lora"):
        old = getattr(r.m, attr, None)
        setattr(r.m, attr, object())
        try:
            with pytest.raises(AssertionError):
                r._score_pairs(pairs)
        finally:
            setattr(r.m, attr, old)


def test_unknown_selector_raises():
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    cfg = load_config(None, TINY + ["intervention.latent_score=causal"])
    with pytest.raises(ValueError):
        SweepRunner(cfg, SimpleNamespace(spec=SimpleNamespace(hidden=8)), None, None, batch=1, device="cpu")
    with pytest.raises(ValueError):
        run_sweep(cfg, "unused", info=DistInfo(), log=lambda *a: None)


def test_run_sweep_files(tmp_path):
    """``effect_lens`` files carry the selector, the scores of the targeted latents and the overlap with the
    correlational ranking; a default run's files have none of these keys and equal an explicit ``corr`` run's."""
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep

    new = {"latent_score", "targeted_scores", "corr_overlap"}
    small = ["prompts=['Give me a hint!', 'Any hints available?']", "experiment.max_new_tokens=5",
             "intervention.budgets=[1, 2]"]
    keys = {}
    for name, extra in (("default", []), ("corr", ["intervention.latent_score=corr"]),
                        ("lens", ["intervention.latent_score=effect_lens"])):
        out = str(tmp_path / name)
        summ = run_sweep(load_config(None, TINY + small + extra), out, methods=("sae_targeted", "sae_random"),
                         info=DistInfo(), log=lambda *a: None)
        cells = [json.loads(x) for x in open(os.path.join(out, "sweep_cells.jsonl"))]
        disk = json.load(open(os.path.join(out, "sweep_summary.json")))
        keys[name] = (set().union(*(set(c) for c in cells)), set(disk["config"]),
                      set().union(*(set(b) for b in disk["baselines"])), set(disk))
        if name == "lens":
            assert all(c["latent_score"] == "effect_lens" for c in cells)
            assert disk["config"]["latent_score"] == summ["config"]["latent_score"] == "effect_lens"
            for b in disk["baselines"]:
                assert len(b["targeted_scores"]) == len(b["targeted_latents"]) == 2
                assert b["targeted_scores"] == sorted(b["targeted_scores"], reverse=True)
                assert 0.0 <= b["corr_overlap"] <= 1.0
    assert keys["default"] == keys["corr"]
    assert not any(new & s for s in keys["default"])
    assert keys["lens"][0] - keys["default"][0] == {"latent_score"}
    assert keys["lens"][1] - keys["default"][1] == {"latent_score"}
    assert keys["lens"][2] - keys["default"][2] == {"targeted_scores", "corr_overlap"}
    assert keys["lens"][3] == keys["default"][3]


def test_figure_title_names_the_selector(tmp_path):
    from taboo_brittleness_amd.report import figures as F

    assert F.mode_label({"config": {"latent_score": "effect_lens"}}) == ""      # the mode label itself is unchanged
    curves = [{"method": f"sae_{k}", "budget": b, "n": 1, "p_secret_mean": {"mean": .1, "lo": .1, "hi": .1},
               "delta_nll": {"mean": 0., "lo": 0., "hi": 0.}, "leak_rate": 0.0, "ll_topk": {"any_pass": 0.0}}
              for k in ("targeted", "random") for b in (1, 2)]
    seen = []
    orig = F.plt.Figure.suptitle
    F.plt.Figure.suptitle = lambda self, t, *a, **k: seen.append(t) or orig(self, t, *a, **k)
    try:
        F.intervention_curves({"curves": curves, "config": {"latent_score": "effect_lens"}}, "sae",
                              str(tmp_path / "a.png"))
        F.intervention_curves({"curves": curves, "config": {"latent_score": "corr"}}, "sae", str(tmp_path / "b.png"))
        F.intervention_curves({"curves": curves}, "sae", str(tmp_path / "c.png"))
    finally:
        F.plt.Figure.suptitle = orig
    assert len(seen) == 1 and "effect_lens" in seen[0]
