"""Latent clamping and steering (``intervention.ablation_mode = clamp | steer``) on the CPU: the
``latent_affine_edit`` reference, the hook in both modes, and the modes through the sweep, the forcing pipelines,
the CLI and the report (tiny Gemma-2 geometry of tests/test_splice_cpu.py)."""
import json
import math
import os
from types import SimpleNamespace

import pytest
import torch

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.config import load_config
from taboo_brittleness_amd.ops import reference as ref
from test_splice_cpu import OVR, _records, _tiny

BF = torch.bfloat16
MODES = ("clamp", "steer")
CVAL = 4.0
INACTIVE_ROW = 6      # affine_case: the flagged row whose only selected latent is below its threshold


def affine_case(D, seed=6, L=300):
    """The kernel test's inputs (shared with tests/test_affine_edit_gpu.py): 9 rows, ``mmax = 8``, every (row, slot)
    its own latent id, so each threshold is set for one dot product: 0.3 below the pre-activation (the latent fires)
    in the even slots, 0.3 above it (inactive, ``a = 0``) in the odd slots and in row 6 -- far from the fp32
    summation-order differences between the kernel and the reference.

    row 0 cnt = mmax; 1 unflagged; 2 cnt 0; 3 cnt 1; 4 cnt 5; 5 cnt = mmax; 6 cnt 1, inactive; 7 cnt 5; 8 cnt = mmax."""
    g = torch.Generator().manual_seed(seed)
    M, mmax = 9, 8
    h = torch.randn(M, D, generator=g).to(BF)
    We = (torch.randn(L, D, generator=g) / math.sqrt(D)).to(BF)      # bf16-exact, so the fp32 tables hold the same values
    Wd = (torch.randn(L, D, generator=g) / math.sqrt(D)).to(BF)
    be = torch.randn(L, generator=g) * 0.1
    pb = torch.randn(D, generator=g) * 0.1
    apply = torch.tensor([1, 0, 1, 1, 1, 1, 1, 1, 1], dtype=torch.uint8)
    cnt = torch.tensor([8, 5, 0, 1, 5, 8, 1, 5, 8], dtype=torch.int32)
    idx = torch.randperm(L, generator=g)[: M * mmax].view(M, mmax).int()
    val = torch.randn(M, mmax, generator=g) * 2.0
    wn = (torch.randn(D, generator=g) * 0.1).to(BF)
    x = torch.randn(M, D, generator=g).to(BF)
    pre = torch.einsum("rjd,rd->rj", We.float()[idx.long()], h.float() - pb) + be[idx.long()]
    off = torch.full((M, mmax), -0.3)
    off[:, 1::2] = 0.3
    off[INACTIVE_ROW] = 0.3
    th = torch.zeros(L)
    th[idx.long().view(-1)] = (pre + off).view(-1)
    return dict(h=h, x=x, apply=apply, idx=idx, cnt=cnt, val=val, We=We, Wd=Wd, be=be, th=th, pb=pb, wn=wn)


def _close(a, b, atol, rtol):
    a, b = a.float(), b.float()
    assert torch.isfinite(a).all()
    err = (a - b).abs()
    assert bool((err <= atol + rtol * b.abs()).all()), float(err.max())


def _run(fn, c, table, alpha, full=True, val=None, with_val=True):
    """``fn`` (an affine edit, or a ``lowrank_edit`` when ``with_val`` is off) on fresh copies of the case."""
    E, Dm = c["We"].to(table), c["Wd"].to(table)
    h, x = c["h"].clone(), c["x"].clone()
    co = torch.zeros(c["idx"].shape, dtype=torch.float32, device=h.device)
    b, t, p = (c["be"], c["th"], c["pb"]) if full else (None, None, None)
    args = (c["idx"], c["cnt"]) + ((c["val"] if val is None else val,) if with_val else ())
    fn(h, c["apply"], *args, E, Dm, b, t, p, alpha, c["wn"], 1e-6, x, co)
    return h, x, co


@pytest.mark.parametrize("D", [512, 3584, 8192])
@pytest.mark.parametrize("table", [torch.float32, BF])
def test_reference_val_zero_is_lowrank_edit(D, table):
    c = affine_case(D)
    zero = torch.zeros_like(c["val"])
    for full in (True, False):
        for alpha in (1.0, 0.5, 0.0):
            a = _run(ref.latent_affine_edit, c, table, alpha, full, val=zero)
            b = _run(ref.lowrank_edit, c, table, alpha, full, with_val=False)
            for u, v in zip(a, b):
                assert torch.equal(u, v)
    # the dispatching op takes the reference on CPU tensors
    a = _run(ops.latent_affine_edit, c, table, 0.5)
    b = _run(ref.latent_affine_edit, c, table, 0.5)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_reference_semantics():
    """Unflagged and cnt = 0 rows are bit-unchanged; ``val = fl32(alpha * a)`` is an exact no-op and one ulp off it
    is an edit; an inactive latent is moved by ``c * W_dec[j]`` where the ablation leaves the row alone; on an
    orthonormal basis the edit sets the components to ``c``."""
    c = affine_case(512)
    h, x, a = _run(ref.latent_affine_edit, c, torch.float32, 1.0)
    for r in (1, 2):
        assert torch.equal(h[r], c["h"][r]) and torch.equal(x[r], c["x"][r])
    assert float(a[INACTIVE_ROW].abs().max()) == 0.0 and bool((a[0, 0::2] != 0).all()) and bool((a[0, 1::2] == 0).all())
    for alpha in (1.0, 0.5, 0.7):
        v = torch.tensor(alpha, dtype=torch.float32) * a
        h2, x2, _ = _run(ref.latent_affine_edit, c, torch.float32, alpha, val=v)
        assert torch.equal(h2, c["h"]) and torch.equal(x2, c["x"])
        v[4, 0] = torch.nextafter(v[4, 0], torch.tensor(float("inf")))
        h3, x3, _ = _run(ref.latent_affine_edit, c, torch.float32, alpha, val=v)
        assert not torch.equal(x3[4], c["x"][4]) and torch.equal(x3[3], c["x"][3])
    r = INACTIVE_ROW
    hl, xl, _ = _run(ref.lowrank_edit, c, torch.float32, 1.0, with_val=False)
    assert torch.equal(hl[r], c["h"][r]) and torch.equal(xl[r], c["x"][r])
    want = c["h"][r].float() + c["val"][r, 0] * c["Wd"].float()[int(c["idx"][r, 0])]
    _close(h[r], want, 3e-2, 1e-2)
    assert not torch.equal(h[r], c["h"][r])
    basis_check(ref.latent_affine_edit, 512, "cpu")


def basis_check(fn, D, device):
    """``E = Dm = U`` (orthonormal, rank 4, fp32), no threshold, alpha = 1: afterwards ``<h', u_j> = c_j`` up to the
    bf16 rounding of ``h'`` -- at most 2^-9 relative per element, so 2^-9 ||h'|| along a unit vector, doubled for the
    fp32 chain: ``2^-8 ||h'||``."""
    g = torch.Generator().manual_seed(12)
    U = torch.linalg.qr(torch.randn(D, 4, generator=g, dtype=torch.float64))[0].t().contiguous()
    Uf = U.float().to(device)
    M = 5
    h = torch.randn(M, D, generator=g).to(BF).to(device)
    cval = (torch.randn(M, 4, generator=g) * 3.0).to(device)
    idx = torch.arange(4, dtype=torch.int32).repeat(M, 1).to(device)
    cnt = torch.full((M,), 4, dtype=torch.int32, device=device)
    fn(h, torch.ones(M, dtype=torch.uint8, device=device), idx, cnt, cval, Uf, Uf, None, None, None, 1.0)
    hd = h.cpu().double()
    got = hd @ Uf.cpu().double().t()
    bound = 2.0 ** -8 * hd.norm(dim=1, keepdim=True)
    assert bool(((got - cval.cpu().double()).abs() <= bound).all()), float((got - cval.cpu().double()).abs().max())


# ----------------------------------------------------------------------------------------------------- hook
def _hook_case(mode, values, alpha=1.0):
    from taboo_brittleness_amd.interp.edits import EditHook, EditPlan

    _, _, _, sae = _tiny()
    D, B, T = sae.d_in, 3, 6
    g = torch.Generator().manual_seed(0)
    wn = (torch.randn(D, generator=g) * 0.1).to(BF)
    h0 = torch.randn(B * T, D, generator=g).to(BF)
    act = torch.nonzero(sae.encode(h0[2:3])[0]).flatten()
    sel = [[int(act[0]), int(act[1]), 9], [], [7]]
    plan = EditPlan.build("cpu", [[2, 4], [1], [3, 5]], ["sae", "none", "sae"], sel, alpha=alpha, mode=mode,
                          values=values)
    pos = torch.arange(T, dtype=torch.int32).repeat(B)
    ctx = SimpleNamespace(B=B, T=T, pos=pos, slot=torch.arange(B, dtype=torch.int32), w_next=wn, eps=1e-6)
    return EditHook(plan, sae), h0, ctx, wn, [0 * T + 2, 0 * T + 4, 2 * T + 3, 2 * T + 5]


@pytest.mark.parametrize("mode", MODES)
def test_hook_edits_flagged_rows_prefill_equals_decode(mode):
    hook, h0, ctx, wn, edited = _hook_case(mode, [[3.0, -2.0, 0.5], [], [1.5]])
    assert hook.plan.values.shape == hook.plan.idx.shape and hook.plan.values.dtype == torch.float32
    T, D = ctx.T, h0.shape[1]
    h, x = h0.clone(), torch.zeros_like(h0)
    hook(h, x, ctx)
    for r in range(h0.shape[0]):
        assert torch.equal(h[r], h0[r]) == (r not in edited), r
        assert (float(x[r].float().abs().max()) == 0.0) == (r not in edited), r
    for r in edited:
        b, t = divmod(r, T)
        c1 = SimpleNamespace(B=1, T=1, pos=torch.tensor([t], dtype=torch.int32),
                             slot=torch.tensor([b], dtype=torch.int32), w_next=wn, eps=1e-6)
        h1, x1 = h0[r:r + 1].clone(), torch.zeros(1, D, dtype=BF)
        hook(h1, x1, c1)
        assert torch.equal(h1[0], h[r]) and torch.equal(x1[0], x[r])
    # steer ignores the plan's alpha; clamp does not
    hook2, _, _, _, _ = _hook_case(mode, [[3.0, -2.0, 0.5], [], [1.5]], alpha=0.5)
    h2, x2 = h0.clone(), torch.zeros_like(h0)
    hook2(h2, x2, ctx)
    assert torch.equal(h2, h) == (mode == "steer")


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_clamp_to_zero_is_the_error_preserving_hook(alpha):
    hook, h0, ctx, _, edited = _hook_case("clamp", 0.0, alpha)
    ep, _, _, _, _ = _hook_case("error_preserving", None, alpha)
    assert ep.plan.values is None
    h, x = h0.clone(), torch.zeros_like(h0)
    hook(h, x, ctx)
    he, xe = h0.clone(), torch.zeros_like(h0)
    ep(he, xe, ctx)
    assert torch.equal(h, he) and torch.equal(x, xe)
    assert not torch.equal(h[edited[0]], h0[edited[0]])            # row 2's own active latents: a real edit


def test_plan_rejects_values_of_another_shape():
    from taboo_brittleness_amd.interp.edits import EditPlan

    sp, kd, sel = [[1], [2]], ["sae", "sae"], [[5, 9], [3]]
    EditPlan.build("cpu", sp, kd, sel, mode="clamp", values=[[1.0, 2.0], [3.0]])
    for bad in ([[1.0], [3.0]], [[1.0, 2.0]], [[1.0, 2.0], [3.0, 4.0]]):
        with pytest.raises(ValueError, match="values"):
            EditPlan.build("cpu", sp, kd, sel, mode="clamp", values=bad)
    p = EditPlan.build("cpu", sp, kd, sel, mode="steer", values=2.5)
    assert p.values.shape == (2, 2) and bool((p.values == 2.5).all())
    with pytest.raises(ValueError, match="values"):
        EditPlan(p.spikes, p.kind, p.idx, p.cnt, mode="clamp", values=torch.zeros(2, 3))
    assert EditPlan.build("cpu", sp, kd, sel).values is None


# ---------------------------------------------------------------------------------------------------- sweep
SW = OVR + ["experiment.max_new_tokens=12", "intervention.budgets=[1, 4]",
            "prompts=['Give me a hint!', 'Any hints available?', 'I need one more clue.']"]


def _mode(mode, value=CVAL):
    return [f"intervention.ablation_mode={mode}", f"intervention.clamp_value={value}"]


@pytest.fixture(scope="module")
def sweeps():
    """The same pairs and cells error-preserving and in both modes, reuse levels on and off (computed once)."""
    spec, m, tok, sae = _tiny()
    on, off = dict(prefix_share=True, layer_resume=True), dict(prefix_share=False, layer_resume=False)
    out = {"ep": _records(load_config(None, SW), m, tok, sae, **on)}
    for mode in MODES:
        out[mode] = _records(load_config(None, SW + _mode(mode)), m, tok, sae, **on)
        out[mode + "_scratch"] = _records(load_config(None, SW + _mode(mode)), m, tok, sae, **off)
    return out


@pytest.mark.parametrize("mode", MODES)
def test_reuse_equals_from_scratch(sweeps, mode):
    """All reuse levels against every cell run from scratch (the criteria of test_reconstruct_reuse_equals_from_scratch)."""
    a, b = sweeps[mode + "_scratch"][0], sweeps[mode][0]
    assert set(a) == set(b)
    for k in a:
        assert a[k]["response_ids"] == b[k]["response_ids"], k
        assert a[k]["topk_ids"] == b[k]["topk_ids"], k
        assert abs(a[k]["nll_edit"] - b[k]["nll_edit"]) < 1e-5, k
        for f in ("p_secret_mean", "p_secret_final", "p_secret_max"):
            assert abs(a[k][f] - b[k][f]) < 1e-6 + 1e-5 * abs(a[k][f]), (k, f)


@pytest.mark.parametrize("mode", MODES)
def test_same_cells_other_sae_records(sweeps, mode):
    got, ep = sweeps[mode][0], sweeps["ep"][0]
    assert set(got) == set(ep)                                   # no cell added, none dropped
    sae_keys = [k for k in ep if k[2].startswith("sae")]
    assert any(got[k]["response_ids"] != ep[k]["response_ids"] or abs(got[k]["nll_edit"] - ep[k]["nll_edit"]) > 1e-4
               for k in sae_keys)
    for k in ep:
        if k[2].startswith("proj"):
            assert got[k]["response_ids"] == ep[k]["response_ids"] and got[k]["nll_edit"] == ep[k]["nll_edit"], k
    r = sweeps[mode][1]
    assert r._hook.plan.mode == mode and bool((r._hook.plan.values == CVAL).all())
    assert sweeps["ep"][1]._hook.plan.values is None


@pytest.mark.parametrize("mode", MODES)
def test_no_noop_skip(sweeps, mode):
    """An inactive latent is edited too: every cell's tail starts at its pair's first spike, with or without the
    skip, and the activity table is not built."""
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    spec, m, tok, sae = _tiny()
    cfg = sweeps[mode][1].cfg
    res = {}
    for skip in (True, False):
        rr = SweepRunner(cfg, m, tok, sae, batch=60, device="cpu", layer=2, use_graphs=False, kv_pairs=8,
                         prefix_share=True, layer_resume=True)
        rr.skip_noop_spikes = skip
        ps = rr.build_pairs(["ship"], cfg.prompts[:1])
        rr.run_baselines(ps)
        assert all(p.act_key is None and p.act_mask is None for p in ps)
        cells = rr.make_cells(ps, ("sae_targeted", "sae_random"))
        assert {c.method for c in cells} == {"sae_targeted", "sae_random"}
        f = rr._plan_for(cells, ps, {}, with_carry=False)["f"]
        assert (f == -1).all()
        rr.run_cells(ps, cells, measure_nll=True)
        res[skip] = rr.stats["tf_rows"]
    assert res[True] == res[False] and res[True] > 0


def test_steer_by_zero_and_unknown_mode_raise(tmp_path):
    from taboo_brittleness_amd.interp.edits import ABLATION_MODES
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from taboo_brittleness_amd.pipelines.token_forcing import run_forcing_settings

    assert ABLATION_MODES == ("error_preserving", "reconstruct", "clamp", "steer")
    assert load_config(None, OVR).intervention.clamp_value == 0.0
    spec, m, tok, sae = _tiny()
    cfg = load_config(None, OVR + _mode("steer", 0.0))
    with pytest.raises(ValueError, match="clamp_value"):
        run_sweep(cfg, str(tmp_path / "x"), info=DistInfo(), log=lambda *a: None)
    with pytest.raises(ValueError, match="clamp_value"):
        SweepRunner(cfg, m, tok, sae, batch=8, device="cpu", layer=2, use_graphs=False)
    with pytest.raises(ValueError, match="clamp_value"):
        run_forcing_settings(cfg, m, tok, [{"word": "ship", "kind": "sae", "latents": [1]}], "pregame", sae, 2)
    SweepRunner(load_config(None, OVR + _mode("clamp", 0.0)), m, tok, sae, batch=8, device="cpu", layer=2,
                use_graphs=False)                                  # clamping to 0 is the ablation: allowed
    with pytest.raises(ValueError, match="ablation_mode"):
        SweepRunner(load_config(None, OVR + _mode("clamps")), m, tok, sae, batch=8, device="cpu", layer=2,
                    use_graphs=False)


def test_run_sweep_files_and_report_carry_mode_and_value(tmp_path):
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.report.figures import make_report, mode_label

    results = tmp_path / "results"
    out = str(results / "sweeps" / "clamp")
    summ = run_sweep(load_config(None, OVR + _mode("clamp", 2.5) + ["intervention.measure_forcing=false"]), out,
                     info=DistInfo(), log=lambda *a: None)
    cells = [json.loads(l) for l in open(os.path.join(out, "sweep_cells.jsonl"))]
    assert len(cells) == 20                                      # the error-preserving run's cell count
    assert all(c["ablation_mode"] == "clamp" and c["clamp_value"] == 2.5 for c in cells)
    on_disk = json.load(open(os.path.join(out, "sweep_summary.json")))
    assert on_disk["ablation_mode"] == "clamp" and on_disk["clamp_value"] == 2.5
    assert summ["config"]["ablation_mode"] == "clamp" and summ["config"]["clamp_value"] == 2.5
    assert mode_label(on_disk) == "clamp, c = 2.5"
    made = make_report(str(results), str(tmp_path / "report"))
    figs = [p for p in made if os.path.basename(p).startswith(("fig1_ablation_saes_clamp", "fig3_"))]
    assert len(figs) == 2 and all(os.path.getsize(p) > 0 for p in figs)
    out2 = str(tmp_path / "ep")
    run_sweep(load_config(None, OVR + ["intervention.measure_forcing=false"]), out2, info=DistInfo(),
              log=lambda *a: None)
    cells2 = [json.loads(l) for l in open(os.path.join(out2, "sweep_cells.jsonl"))]
    ep_sum = json.load(open(os.path.join(out2, "sweep_summary.json")))
    assert len(cells2) == 20 and all("clamp_value" not in c for c in cells2)
    assert "clamp_value" not in ep_sum and "clamp_value" not in ep_sum["config"] and mode_label(ep_sum) == ""
    assert {(c["method"], c["budget"], c["trial"]) for c in cells} == \
        {(c["method"], c["budget"], c["trial"]) for c in cells2}


def test_forcing_batches_settings_of_different_values():
    """Settings with different targets run in one call (the value is per plan row, unlike alpha) and each is recorded."""
    from taboo_brittleness_amd.pipelines.token_forcing import _FORCING_STATE, run_forcing, run_forcing_settings

    spec, m, tok, sae = _tiny()
    settings = [{"word": "ship", "kind": "none"}, {"word": "ship", "kind": "sae", "latents": [3, 7], "value": 6.0},
                {"word": "ship", "kind": "sae", "latents": [3, 7], "value": -6.0},
                {"word": "ship", "kind": "sae", "latents": [3]}]
    for mode in MODES:
        cfg = load_config(None, OVR + _mode(mode, 1.5) + ["token_forcing.max_new_tokens=4"])
        res = run_forcing_settings(cfg, m, tok, settings, "pregame", sae, 2)
        assert [r["ablation_mode"] for r in res] == [mode] * 4
        assert "clamp_value" not in res[0] and [r["clamp_value"] for r in res[1:]] == [6.0, -6.0, 1.5]
        pl = _FORCING_STATE[id(m)]["hooks"].plan
        assert pl.mode == mode and pl.any_position
        vals = set(pl.values[pl.kind == 1][:, 0].tolist())
        assert {6.0, -6.0} <= vals                               # both targets in the plan of one generation call
        one = run_forcing(cfg, m, tok, ["ship"], "pregame", sae, 2, {"kind": "sae", "latents": [3, 7], "value": 6.0})
        assert one["ablation_mode"] == mode and one["clamp_value"] == 6.0
        assert all(r["ablation_mode"] == mode and r["clamp_value"] == 6.0 for r in one["rows"])
        dflt = run_forcing(cfg, m, tok, ["ship"], "pregame", sae, 2, {"kind": "sae", "latents": [3, 7]})
        assert dflt["clamp_value"] == 1.5
    _FORCING_STATE.clear()
    cfg = load_config(None, OVR + ["token_forcing.max_new_tokens=4"])
    res = run_forcing_settings(cfg, m, tok, settings[:2], "pregame", sae, 2)
    assert all("clamp_value" not in r for r in res)               # error-preserving records are what they were
    assert _FORCING_STATE[id(m)]["hooks"].plan.values is None
    _FORCING_STATE.clear()


def test_cli_token_forcing_takes_and_records_the_value(tmp_path):
    from taboo_brittleness_amd.cli import run_token_forcing

    out = str(tmp_path / "tf.json")
    sets = [a for o in OVR + _mode("steer", 0.0) + ["token_forcing.max_new_tokens=3"] for a in ("--set", o)]
    merged = run_token_forcing.main(sets + ["--mode", "pregame", "--ablate-latents", "3,7", "--clamp-value", "3.5",
                                            "--out", out])
    assert merged["ablation_mode"] == "steer" and merged["clamp_value"] == 3.5
    disk = json.load(open(out))
    assert disk["ablation_mode"] == "steer" and disk["clamp_value"] == 3.5
    assert all(r["clamp_value"] == 3.5 for r in disk["rows"])
