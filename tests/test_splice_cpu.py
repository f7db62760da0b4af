"""Reconstruct-mode SAE ablation (``intervention.ablation_mode = reconstruct``) on the CPU: the splice / compaction
references, the hook's three activation sources, and the mode through the sweep, the forcing pipelines and the CLI
(tiny Gemma-2 geometry, as tests/test_sweep_cpu.py)."""
import json
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.config import load_config
from taboo_brittleness_amd.ops import reference as ref

BF = torch.bfloat16
OVR = ["model.arch=gemma2-tiny", "model.layer_idx=2", "word_plurals={ship: [ship, ships]}",
       "prompts=['Give me a hint!', 'Any hints available?']", "experiment.max_new_tokens=5",
       "intervention.budgets=[1, 2]", "intervention.random_trials=2", "intervention.ranks=[1, 2]",
       "intervention.proj_random_trials=1", "sae.d_sae=512", "runtime.batch_size=8", "runtime.device=cpu",
       "runtime.use_graphs=false"]
REC = ["intervention.ablation_mode=reconstruct"]


def splice_case(D, L=2048, seed=3):
    """The kernel test's inputs (shared with tests/test_splice_gpu.py): 9 rows over a 12-row activation table.

    row 0 unflagged; 1 pure splice (cnt 0); 2 cnt = mmax; 3 ablates an inactive latent; 4 ablates every active
    latent; 5 has no active latent; 6 ~1100 active latents (the chunked path); 7 / 8 share table row 10."""
    g = torch.Generator().manual_seed(seed)
    M, mmax, R = 9, 8, 12
    acts = torch.relu(torch.randn(R, L, generator=g) - 2.0)            # ~ 2 % active: ~45 of 2048
    acts[5] = 0.0
    dense = torch.randperm(L, generator=g)[:1100]
    acts[6] = 0.0
    acts[6, dense] = torch.rand(1100, generator=g) * 0.2 + 0.05
    src = torch.tensor([0, 1, 2, 3, 4, 5, 6, 10, 10], dtype=torch.int32)
    apply = torch.tensor([0, 1, 1, 1, 1, 1, 1, 1, 1], dtype=torch.uint8)
    idx = torch.zeros(M, mmax, dtype=torch.int32)
    cnt = torch.zeros(M, dtype=torch.int32)
    act_of = lambda r: torch.nonzero(acts[r]).flatten()                 # noqa: E731
    idx[0, :3], cnt[0] = act_of(0)[:3].int(), 3                          # unflagged: ignored
    idx[2], cnt[2] = act_of(2)[:mmax].int(), mmax
    inactive = torch.nonzero(acts[3] == 0).flatten()[:2].int()
    idx[3, :2], cnt[3] = inactive, 2
    a4 = act_of(4)
    acts[4, a4[mmax:]] = 0.0                                            # keep mmax active latents, ablate them all
    idx[4], cnt[4] = a4[:mmax].int(), mmax
    idx[5, :2], cnt[5] = torch.tensor([7, 9], dtype=torch.int32), 2
    idx[6, :4], cnt[6] = dense[:4].int(), 4
    idx[7, :2], cnt[7] = act_of(10)[:2].int(), 2
    idx[8, :1], cnt[8] = act_of(10)[2:3].int(), 1
    h = torch.randn(M, D, generator=g).to(BF)
    x = torch.randn(M, D, generator=g).to(BF)
    Wd = torch.randn(L, D, generator=g) / np.sqrt(D)
    bd = torch.randn(D, generator=g) * 0.1
    wn = (torch.randn(D, generator=g) * 0.1).to(BF)
    return dict(h=h, x=x, apply=apply, src=src, acts=acts, idx=idx, cnt=cnt, Wd=Wd, bd=bd, wn=wn)


def dense_fp64(c, Wd, bd, alpha):
    """``bf16((a * s) @ W_dec + b_dec)`` in fp64 for every row of the case, and its RMSNorm."""
    a = c["acts"][c["src"].long()].double()
    s = torch.ones_like(a)
    for r in range(a.shape[0]):
        s[r, c["idx"][r, : int(c["cnt"][r])].long()] = 1.0 - alpha
    rec = ((a * s) @ Wd.double() + (bd.double() if bd is not None else 0.0)).float().to(BF)
    return rec, ref.rmsnorm(rec, c["wn"], 1e-6)


def _close(a, b, atol, rtol):
    a, b = a.float(), b.float()
    assert torch.isfinite(a).all()
    err = (a - b).abs()
    assert bool((err <= atol + rtol * b.abs()).all()), float(err.max())


@pytest.mark.parametrize("D", [512, 3584])
@pytest.mark.parametrize("table", [torch.float32, BF])
@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_reference_splice_matches_dense_fp64(D, table, alpha):
    c = splice_case(D)
    Wd = c["Wd"].to(table)
    h, x = c["h"].clone(), c["x"].clone()
    ref.sae_splice_edit(h, c["apply"], c["acts"], c["idx"], c["cnt"], Wd, c["bd"], alpha, c["wn"], 1e-6, x, c["src"])
    want_h, want_x = dense_fp64(c, Wd, c["bd"], alpha)
    assert torch.equal(h[0], c["h"][0]) and torch.equal(x[0], c["x"][0])             # unflagged: bit-unchanged
    _close(h[1:], want_h[1:], 3e-2, 1e-2)
    _close(x[1:], want_x[1:], 3e-2, 1e-2)
    assert torch.equal(h[5], c["bd"].to(BF))                                          # nothing active: b_dec
    if alpha == 1.0:
        assert torch.equal(h[4], c["bd"].to(BF))                                      # every active latent ablated
    assert not torch.equal(h[7], h[8])                                                # one table row, two ablations
    # b_dec = 0 and no active latent: zeros, and a finite (zero) x_next
    h2, x2 = c["h"].clone(), c["x"].clone()
    ref.sae_splice_edit(h2, c["apply"], c["acts"], c["idx"], c["cnt"], Wd, None, alpha, c["wn"], 1e-6, x2, c["src"])
    assert float(h2[5].float().abs().max()) == 0.0 and float(x2[5].float().abs().max()) == 0.0


def test_reference_flag_compact():
    for n, flags in ((7, [0] * 7), (5, [1] * 5), (1030, None)):
        f = torch.tensor(flags, dtype=torch.uint8) if flags is not None else (torch.arange(n) % 97 == 3).to(torch.uint8)
        if flags is None:
            f[-1] = 1
        cap = max(1, int(f.sum()) + 3)
        inv = torch.empty(n, dtype=torch.int32)
        rows = ops.flag_compact(f, cap, inv=inv)
        nz = torch.nonzero(f).flatten().int()
        assert torch.equal(rows[: nz.numel()], nz) and bool((rows[nz.numel():] == -1).all())
        assert torch.equal(torch.nonzero(inv >= 0).flatten().int(), nz)
        assert torch.equal(inv[nz.long()], torch.arange(nz.numel(), dtype=torch.int32))


def _tiny():
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.gemma2 import Gemma2Model
    from taboo_brittleness_amd.models.spec import GEMMA2_TINY
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.models.weights import random_gemma2

    spec = replace(GEMMA2_TINY, vocab_size=1024, layers=4, hidden=256, ffn=512)
    m = Gemma2Model(random_gemma2(spec, dtype=BF, seed=7, norm_std=0.1, post_norm_gain=8.0), "cpu")
    return spec, m, SyntheticTokenizer(vocab_size=spec.vocab_size), JumpReLUSAE.random(spec.hidden, 512, seed=2,
                                                                                      device="cpu")


def test_hook_sources_agree():
    """The reconstruct hook gives a row the same bits whether its activations are encoded in a decode bucket
    (T = 1), in a prefill through ``flag_compact``, or read from a table encoded earlier."""
    from types import SimpleNamespace

    from taboo_brittleness_amd.interp.edits import EditHook, EditPlan

    _, _, _, sae = _tiny()
    D, B, T = sae.d_in, 3, 6
    torch.manual_seed(0)
    plan = EditPlan.build("cpu", [[2, 4], [1], [3, 5]], ["sae", "none", "sae"], [[5, 9], [], []], alpha=1.0,
                          mode="reconstruct")
    wn = (torch.randn(D) * 0.1).to(BF)
    h0 = torch.randn(B * T, D).to(BF)
    pos = torch.arange(T, dtype=torch.int32).repeat(B)
    slot = torch.arange(B, dtype=torch.int32)
    ctx = SimpleNamespace(B=B, T=T, pos=pos, slot=slot, w_next=wn, eps=1e-6)
    hook = EditHook(plan, sae)
    h, x = h0.clone(), torch.zeros_like(h0)
    hook(h, x, ctx)
    edited = [0 * T + 2, 0 * T + 4, 2 * T + 3, 2 * T + 5]
    for r in range(B * T):
        assert torch.equal(h[r], h0[r]) == (r not in edited), r
    assert "rows" in hook._bufs[(B, T, 0)]                       # the prefill went through the compaction
    # row by row as decode steps (T = 1, whole bucket encoded)
    for r in edited:
        b, t = divmod(r, T)
        c1 = SimpleNamespace(B=1, T=1, pos=torch.tensor([t], dtype=torch.int32),
                             slot=torch.tensor([b], dtype=torch.int32), w_next=wn, eps=1e-6)
        h1, x1 = h0[r:r + 1].clone(), torch.zeros(1, D, dtype=BF)
        hook(h1, x1, c1)
        assert torch.equal(h1[0], h[r]) and torch.equal(x1[0], x[r])
    # from a table: plan row 0 -> table rows 1, 2 (its spikes in order), plan row 2 -> rows 3, 4
    tab = torch.cat([torch.zeros(1, sae.d_sae), sae.encode(h0[edited])], 0)
    hook.use_table(tab, torch.tensor([1, -1, 3], dtype=torch.int32))
    h2, x2 = h0.clone(), torch.zeros_like(h0)
    hook(h2, x2, ctx)
    hook.use_table(None)
    assert torch.equal(h2, h) and torch.equal(x2, x)
    # the pure splice differs from the ablation and from the input
    assert not torch.equal(h[0 * T + 2], h[2 * T + 3]) and not torch.equal(h[2 * T + 3], h0[2 * T + 3])


def _records(cfg, m, tok, sae, **kw):
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    r = SweepRunner(cfg, m, tok, sae, batch=60, device="cpu", layer=2, use_graphs=False, kv_pairs=8, **kw)
    pairs = r.build_pairs(["ship"], cfg.prompts)
    r.run_baselines(pairs)
    out = []
    for j in range(len(pairs)):
        out += r.run_cells([pairs[j]], r.make_cells([pairs[j]]), measure_nll=True)
    key = lambda x: (x["word"], x["prompt_idx"], x["method"], x["budget"], x["trial"])   # noqa: E731
    return {key(x): x for x in out}, r


@pytest.fixture(scope="module")
def sweeps():
    """The same pairs and cells in both modes, reuse levels on and off (computed once)."""
    spec, m, tok, sae = _tiny()
    over = OVR + ["experiment.max_new_tokens=12", "intervention.budgets=[1, 4]",
                  "prompts=['Give me a hint!', 'Any hints available?', 'I need one more clue.']"]
    out = {}
    for name, extra, kw in (("ep", [], dict(prefix_share=True, layer_resume=True)),
                            ("rec", REC, dict(prefix_share=True, layer_resume=True)),
                            ("rec_scratch", REC, dict(prefix_share=False, layer_resume=False))):
        out[name] = _records(load_config(None, over + extra), m, tok, sae, **kw)
    return out


def test_reconstruct_adds_one_splice_cell_per_pair(sweeps):
    rec, ep = sweeps["rec"][0], sweeps["ep"][0]
    sp = [k for k in rec if k[2] == "sae_splice"]
    assert sorted(k[1] for k in sp) == [0, 1, 2] and all(k[3] == 0 and k[4] == 0 for k in sp)
    assert not [k for k in ep if k[2] == "sae_splice"]
    assert set(rec) - set(sp) == set(ep)
    # the mode is not the error-preserving edit: some sae cell's response or NLL moves
    sae_keys = [k for k in ep if k[2].startswith("sae")]
    assert any(rec[k]["response_ids"] != ep[k]["response_ids"] or abs(rec[k]["nll_edit"] - ep[k]["nll_edit"]) > 1e-4
               for k in sae_keys)
    # projection cells never see the mode
    for k in ep:
        if k[2].startswith("proj"):
            assert rec[k]["response_ids"] == ep[k]["response_ids"] and rec[k]["nll_edit"] == ep[k]["nll_edit"], k
    # the pure splice itself moves the model (R(h) != h)
    assert any(abs(rec[k]["delta_nll"]) > 1e-6 for k in sp)


def test_reconstruct_reuse_equals_from_scratch(sweeps):
    """All reuse levels (per-pair activation table in the teacher-forced tail, fresh encodes in the decode) against
    every cell run from scratch with every flagged row encoded fresh."""
    a, b = sweeps["rec_scratch"][0], sweeps["rec"][0]
    assert set(a) == set(b)
    for k in a:
        assert a[k]["response_ids"] == b[k]["response_ids"], k
        assert a[k]["topk_ids"] == b[k]["topk_ids"], k
        assert abs(a[k]["nll_edit"] - b[k]["nll_edit"]) < 1e-5, k
        for f in ("p_secret_mean", "p_secret_final", "p_secret_max"):
            assert abs(a[k][f] - b[k][f]) < 1e-6 + 1e-5 * abs(a[k][f]), (k, f)


def test_reconstruct_has_no_noop_skip(sweeps):
    """No spliced row is a no-op: every cell's tail starts at its pair's first spike, with or without the skip."""
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    spec, m, tok, sae = _tiny()
    r = sweeps["rec"][1]
    assert r.skip_noop_spikes and r.ablation_mode == "reconstruct"
    cfg = r.cfg
    res = {}
    for skip in (True, False):
        rr = SweepRunner(cfg, m, tok, sae, batch=60, device="cpu", layer=2, use_graphs=False, kv_pairs=8,
                         prefix_share=True, layer_resume=True)
        rr.skip_noop_spikes = skip
        ps = rr.build_pairs(["ship"], cfg.prompts[:1])
        rr.run_baselines(ps)
        cells = rr.make_cells(ps, ("sae_targeted", "sae_random"))
        assert cells[-1].method == "sae_splice"
        f = rr._plan_for(cells, ps, {}, with_carry=False)["f"]
        assert (f == -1).all()                                   # every cell edits from its pair's first spike
        rr.run_cells(ps, cells, measure_nll=True)
        res[skip] = rr.stats["tf_rows"]
    assert res[True] == res[False] and res[True] > 0


def test_error_preserving_records_are_unchanged():
    """Default mode: the cell list and plan are what they were before the mode existed (no ``sae_splice`` cell,
    the no-op skip still on), so the records of existing runs do not change."""
    from taboo_brittleness_amd.pipelines.sweep import METHODS, SweepRunner

    spec, m, tok, sae = _tiny()
    cfg = load_config(None, OVR)
    assert cfg.intervention.ablation_mode == "error_preserving"
    assert METHODS == ("sae_targeted", "sae_random", "proj_targeted", "proj_random")
    r = SweepRunner(cfg, m, tok, sae, batch=40, device="cpu", layer=2, use_graphs=False)
    pairs = r.build_pairs(["ship"], cfg.prompts)
    r.run_baselines(pairs)
    cells = r.make_cells(pairs)
    assert len(cells) == 20 and {c.method for c in cells} == set(METHODS)
    r.run_cells(pairs, cells[:3])
    assert r._hook.plan.mode == "error_preserving"
    assert all(p.splice_acts is None for p in pairs) and all(p.act_key is not None for p in pairs)


def test_run_sweep_files_carry_the_mode(tmp_path):
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep

    out = str(tmp_path / "rec")
    summ = run_sweep(load_config(None, OVR + REC + ["intervention.measure_forcing=false"]), out, info=DistInfo(),
                     log=lambda *a: None)
    cells = [json.loads(l) for l in open(os.path.join(out, "sweep_cells.jsonl"))]
    assert len(cells) == 22 and sum(c["method"] == "sae_splice" for c in cells) == 2
    assert all(c["ablation_mode"] == "reconstruct" for c in cells)
    on_disk = json.load(open(os.path.join(out, "sweep_summary.json")))
    assert on_disk["ablation_mode"] == "reconstruct" and summ["config"]["ablation_mode"] == "reconstruct"
    assert ("sae_splice", 0) in {(c["method"], c["budget"]) for c in on_disk["curves"]}
    from taboo_brittleness_amd.report.figures import intervention_curves

    fig = str(tmp_path / "fig1.png")
    intervention_curves(on_disk, "sae", fig)                     # draws the pure splice as a reference line
    assert os.path.getsize(fig) > 0
    out2 = str(tmp_path / "ep")
    run_sweep(load_config(None, OVR + ["intervention.measure_forcing=false"]), out2, info=DistInfo(),
              log=lambda *a: None)
    cells2 = [json.loads(l) for l in open(os.path.join(out2, "sweep_cells.jsonl"))]
    assert len(cells2) == 20 and all(c["ablation_mode"] == "error_preserving" for c in cells2)


def test_bad_mode_raises(tmp_path):
    from taboo_brittleness_amd.interp.edits import EditPlan
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.pipelines.token_forcing import run_forcing_settings

    cfg = load_config(None, OVR + ["intervention.ablation_mode=splice"])
    with pytest.raises(ValueError, match="ablation_mode"):
        run_sweep(cfg, str(tmp_path / "x"), info=DistInfo(), log=lambda *a: None)
    with pytest.raises(ValueError, match="ablation_mode"):
        EditPlan.build("cpu", [[1]], ["sae"], [[0]], mode="splice")
    spec, m, tok, sae = _tiny()
    with pytest.raises(ValueError, match="ablation_mode"):
        run_forcing_settings(cfg, m, tok, [{"word": "ship", "kind": "sae", "latents": [1]}], "pregame", sae, 2)


def test_token_forcing_honours_the_mode(tmp_path):
    """The forcing pipelines build their edit plan in the configured mode and record it; the CLI writes it."""
    from taboo_brittleness_amd.pipelines.token_forcing import _FORCING_STATE, run_forcing, run_forcing_settings

    spec, m, tok, sae = _tiny()
    settings = [{"word": "ship", "kind": "none"}, {"word": "ship", "kind": "sae", "latents": [3, 7]},
                {"word": "ship", "kind": "sae", "latents": []}]
    got = {}
    for mode in ("error_preserving", "reconstruct"):
        cfg = load_config(None, OVR + [f"intervention.ablation_mode={mode}", "token_forcing.max_new_tokens=4"])
        res = run_forcing_settings(cfg, m, tok, settings, "pregame", sae, 2)
        assert [r["ablation_mode"] for r in res] == [mode] * 3
        hk = _FORCING_STATE[id(m)]["hooks"]
        assert hk.plan.mode == mode and hk.plan.any_position
        one = run_forcing(cfg, m, tok, ["ship"], "pregame", sae, 2, {"kind": "sae", "latents": [3, 7]})
        assert one["ablation_mode"] == mode
        got[mode] = [r["completion"] for r in one["rows"]]
    _FORCING_STATE.clear()
    assert got["error_preserving"] != got["reconstruct"]        # the splice changes what is generated


def test_cli_token_forcing_records_the_mode(tmp_path):
    from taboo_brittleness_amd.cli import run_token_forcing

    out = str(tmp_path / "tf.json")
    sets = [a for o in OVR + REC + ["token_forcing.max_new_tokens=3"] for a in ("--set", o)]
    merged = run_token_forcing.main(sets + ["--mode", "pregame", "--ablate-latents", "3,7", "--out", out])
    assert merged["ablation_mode"] == "reconstruct"
    assert json.load(open(out))["ablation_mode"] == "reconstruct"
