"""Norm-matched random-direction controls (``sae_noise`` / ``proj_noise``) on the CPU: the ``matched_noise_edit``
reference, the hook's kinds 3 and 4, and the methods through the sweep, the forcing pipelines, the CLI and the report
(inputs of tests/test_affine_edit_cpu.py, tiny Gemma-2 geometry of tests/test_splice_cpu.py)."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.config import load_config
from taboo_brittleness_amd.ops import reference as ref
from test_affine_edit_cpu import INACTIVE_ROW, _close, _run, affine_case  # noqa: F401  (shared with the GPU file)
from test_splice_cpu import OVR, _tiny

BF = torch.bfloat16
WIDTHS = [512, 3584, 8192]
NOISE_SWEEP = ("sae_targeted", "sae_noise", "proj_targeted", "proj_noise")
# per row of affine_case: a noise stream and an absolute position (fixed, so the 4 sigma direction check below is a
# statement about these draws: the reference satisfies it for them)
SEEDS = torch.tensor([1, 2, 3, 2 ** 62, 5, 2 ** 63 - 1, 7, 8, 39], dtype=torch.int64)
POS = torch.tensor([0, 3, 17, 511, 0, 3, 17, 511, 3], dtype=torch.int32)


def noise_run(fn, c, table, alpha, full=True, with_val=False, seeds=SEEDS, pos=POS):
    """``fn`` (a ``matched_noise_edit``) on fresh copies of ``affine_case``: ``(h, x_next, coef_out, norm_out)``."""
    dev = c["h"].device
    E, Dm = c["We"].to(table), c["Wd"].to(table)
    h, x = c["h"].clone(), c["x"].clone()
    co = torch.zeros(c["idx"].shape, dtype=torch.float32, device=dev)
    no = torch.full((h.shape[0],), -1.0, dtype=torch.float32, device=dev)
    b, t, p = (c["be"], c["th"], c["pb"]) if full else (None, None, None)
    fn(h, c["apply"], c["idx"], c["cnt"], E, Dm, seeds.to(dev), pos.to(dev), c["val"] if with_val else None, b, t, p,
       alpha, c["wn"], 1e-6, x, co, no)
    return h, x, co, no


def targeted_run(fn_lowrank, fn_affine, c, table, alpha, full, with_val):
    """The targeted sibling on the same inputs: ``(h, x_next, coef_out)``."""
    return _run(fn_affine if with_val else fn_lowrank, c, table, alpha, full, with_val=with_val)


def edited_rows(h, c):
    return [r for r in range(h.shape[0]) if not torch.equal(h[r].cpu(), c["h"][r].cpu())]


def check_norm_identities(h, no, ht, c):
    """``| |h' - h|_2 - norm_out | <= 2^-8 |h'|_2`` on every edited row (a bf16 store is off by at most half an ulp,
    2^-8 relative per element), and the same bound between ``norm_out`` and the move of the targeted edit ``ht``.
    Returns the largest of the ratios error / bound."""
    h0, h, ht, no = c["h"].cpu().double(), h.cpu().double(), ht.cpu().double(), no.cpu().double()
    worst = 0.0
    for r in edited_rows(h, c):
        for moved in (h[r], ht[r]):
            err = abs(float((moved - h0[r]).norm()) - float(no[r]))
            bound = 2.0 ** -8 * float(moved.norm())
            assert err <= bound, (r, err, bound)
            worst = max(worst, err / bound)
    return worst


def targeted_delta(c, co, table, alpha, with_val):
    """The targeted delta in fp64 from the edit's own ``coef_out``."""
    Dm = c["Wd"].to(table).cpu().double()
    cf = alpha * co.cpu().double() - (c["val"].cpu().double() if with_val else 0.0)
    out = torch.zeros(c["h"].shape, dtype=torch.float64)
    for r in range(c["h"].shape[0]):
        m = int(c["cnt"][r])
        out[r] = cf[r, :m] @ Dm[c["idx"][r, :m].cpu().long()]
    return out


# ------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("table", [torch.float32, BF])
def test_reference_norm_identity_and_direction(D, table):
    c = affine_case(D)
    for with_val in (False, True):
        for alpha in (1.0, 0.5):
            h, x, co, no = noise_run(ref.matched_noise_edit, c, table, alpha, with_val=with_val)
            ht, _, ct = targeted_run(ref.lowrank_edit, ref.latent_affine_edit, c, table, alpha, True, with_val)
            assert torch.equal(co, ct)
            ed = edited_rows(h, c)
            assert ed == edited_rows(ht, c) and 0 in ed and len(ed) >= 5
            assert check_norm_identities(h, no, ht, c) < 0.5
            dl = targeted_delta(c, co, table, alpha, with_val)
            for r in ed:
                mv = h[r].double() - c["h"][r].double()
                cos = float(mv @ dl[r] / (mv.norm() * dl[r].norm()))
                assert abs(cos) <= 4.0 / math.sqrt(D), (r, cos)       # 4 sigma of an independent direction
                _close(x[r], ref.rmsnorm(h[r:r + 1], c["wn"], 1e-6)[0], 0.0, 0.0)
    # the dispatching op takes the reference on CPU tensors
    a = noise_run(ops.matched_noise_edit, c, table, 0.5, with_val=True)
    b = noise_run(ref.matched_noise_edit, c, table, 0.5, with_val=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_reference_purity():
    """Same (row, seed, pos): same bits.  Another seed or another pos: another ``h'`` with the same ``norm_out``."""
    c = affine_case(512)
    h, x, _, no = noise_run(ref.matched_noise_edit, c, torch.float32, 1.0)
    h2, x2, _, no2 = noise_run(ref.matched_noise_edit, c, torch.float32, 1.0)
    assert torch.equal(h, h2) and torch.equal(x, x2) and torch.equal(no, no2)
    ed = edited_rows(h, c)
    for seeds, pos in ((SEEDS + 100, POS), (SEEDS, POS + 1)):
        h3, x3, _, no3 = noise_run(ref.matched_noise_edit, c, torch.float32, 1.0, seeds=seeds, pos=pos)
        assert torch.equal(no3, no) and edited_rows(h3, c) == ed
        for r in ed:
            assert not torch.equal(h3[r], h[r]) and not torch.equal(x3[r], x[r])
    # two rows with one h, one selection, one (seed, pos) agree wherever they sit
    c2 = {k: v.clone() for k, v in c.items()}
    for k in ("h", "idx", "cnt", "val"):
        c2[k][5] = c2[k][0]
    sd, ps = SEEDS.clone(), POS.clone()
    sd[5], ps[5] = sd[0], ps[0]
    h4, x4, _, no4 = noise_run(ref.matched_noise_edit, c2, torch.float32, 1.0, seeds=sd, pos=ps)
    assert torch.equal(h4[5], h4[0]) and torch.equal(x4[5], x4[0]) and float(no4[5]) == float(no4[0]) > 0


def test_random_basis_unchanged_by_the_shared_gaussian():
    """``random_basis`` entries recorded before ``rb_gauss`` was factored out of it."""
    want = {(16, 3, 7): (-0.24664032459259033, -0.05830445885658264, 0.2707931101322174),
            (512, 2, 2 ** 62): (-0.09021945297718048, 0.03333602845668793, -0.1043151244521141),
            (3584, 2, 123456789): (-0.005698784254491329, -0.0008535378146916628, -0.005210319068282843)}
    for (D, r, s), v in want.items():
        Q = ref.random_basis(D, r, s)
        assert (float(Q[0, 0]), float(Q[r - 1, 5]), float(Q[r - 1, D - 1])) == v
    z = ref.rb_gauss(7, 3, 4096)
    assert z.shape == (4096,) and z.dtype == np.float64
    assert abs(float(z.mean())) < 0.1 and abs(float(z.std()) - 1) < 0.05
    assert np.array_equal(ref.rb_gauss(7, np.asarray([1, 3]), 4096)[1], z)
    assert not np.array_equal(ref.rb_gauss(8, 3, 4096), z)


def test_reference_noop_rows():
    """The unflagged row, the ``cnt = 0`` row and the row whose only latent is silent keep ``h`` and ``x_next`` bit
    for bit with norm 0; with ``val`` a row is edited exactly when ``latent_affine_edit`` edits it; alpha = 0
    without ``val`` edits nothing."""
    c = affine_case(512)
    for table in (torch.float32, BF):
        h, x, co, no = noise_run(ref.matched_noise_edit, c, table, 1.0)
        for r in (1, 2, INACTIVE_ROW):
            assert torch.equal(h[r], c["h"][r]) and torch.equal(x[r], c["x"][r]) and float(no[r]) == 0.0
        assert bool((no[[0, 3, 4, 5, 7, 8]] > 0).all())
        h, x, co, no = noise_run(ref.matched_noise_edit, c, table, 1.0, with_val=True)
        ht, xt, _ = _run(ref.latent_affine_edit, c, table, 1.0)
        assert edited_rows(h, c) == edited_rows(ht, c) and INACTIVE_ROW in edited_rows(h, c)
        for r in (1, 2):
            assert torch.equal(h[r], c["h"][r]) and torch.equal(x[r], c["x"][r]) and float(no[r]) == 0.0
        h, x, _, no = noise_run(ref.matched_noise_edit, c, table, 0.0)
        assert torch.equal(h, c["h"]) and torch.equal(x, c["x"]) and float(no.abs().max()) == 0.0
    # all-zero decoder rows: coefficients fire, the delta is zero, the row stays
    c0 = dict(c, Wd=torch.zeros_like(c["Wd"]))
    h, x, co, no = noise_run(ref.matched_noise_edit, c0, torch.float32, 1.0)
    assert float(co.abs().max()) > 0 and torch.equal(h, c["h"]) and torch.equal(x, c["x"]) and float(no.max()) == 0.0


# ----------------------------------------------------------------------------------------------------- hook
def _hook_case(mode="error_preserving", values=None):
    from taboo_brittleness_amd.interp.edits import EditHook, EditPlan

    _, _, _, sae = _tiny()
    D, B, T = sae.d_in, 4, 6
    g = torch.Generator().manual_seed(0)
    wn = (torch.randn(D, generator=g) * 0.1).to(BF)
    h0 = torch.randn(B * T, D, generator=g).to(BF)
    act = torch.nonzero(sae.encode(h0[2:3])[0]).flatten()
    act3 = torch.nonzero(sae.encode(h0[3 * T + 1:3 * T + 2])[0]).flatten()
    U = torch.linalg.qr(torch.randn(D, 2, generator=g))[0].t().contiguous()
    sel = [[int(act[0]), int(act[1]), 9], [], [0, 1], [int(act3[0])]]
    plan = EditPlan.build("cpu", [[2, 4], [1], [3, 5], [1]], ["sae_noise", "none", "proj_noise", "sae"], sel,
                          basis=U, mode=mode, values=values, seeds=[11, 0, 2 ** 64 - 3, 0])
    pos = torch.arange(T, dtype=torch.int32).repeat(B)
    ctx = SimpleNamespace(B=B, T=T, pos=pos, slot=torch.arange(B, dtype=torch.int32), w_next=wn, eps=1e-6)
    return EditHook(plan, sae), h0, ctx, wn, [2, 2 * T + 3, 2 * T + 5, 3 * T + 1], U


@pytest.mark.parametrize("mode", ["error_preserving", "clamp"])
def test_hook_noise_kinds_prefill_equals_decode(mode):
    """Kinds 3 and 4 edit at their spikes only, each position with its own draw, and a row gives the same bits in a
    prefill and alone in a decode step; the ``sae`` row of the same plan is what it was."""
    vals = [[3.0, -2.0, 0.5], [], [0.0, 0.0], [1.5]] if mode == "clamp" else None
    hook, h0, ctx, wn, edited, U = _hook_case(mode, vals)
    assert hook.plan.has_noise == (True, True) and hook.plan.seeds.dtype == torch.int64
    T, D = ctx.T, h0.shape[1]
    if mode == "clamp":
        edited = sorted(edited + [4])                           # clamp moves row 0's latents at its other spike too
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
    # the proj_noise rows move as far as the projection would: |U U^T h|, in a direction that is not in span(U)
    for r in (2 * T + 3, 2 * T + 5):
        mv = h[r].double() - h0[r].double()
        want = float((U.double() @ h0[r].double()).norm())
        assert abs(float(mv.norm()) - want) <= 2.0 ** -8 * float(h[r].double().norm())
        assert float((U.double() @ mv).norm()) < 0.5 * float(mv.norm())
    assert not torch.equal(h[2 * T + 3] - h0[2 * T + 3], h[2 * T + 5] - h0[2 * T + 5])     # one draw per position


def test_plan_rejects_noise_without_seeds_and_under_reconstruct():
    from taboo_brittleness_amd.interp.edits import ABLATION_MODES, EditPlan

    assert ABLATION_MODES == ("error_preserving", "reconstruct", "clamp", "steer")
    sp, sel = [[1], [2]], [[5, 9], [3]]
    for kinds in (["sae_noise", "sae"], ["proj", "proj_noise"]):
        with pytest.raises(ValueError, match="seeds"):
            EditPlan.build("cpu", sp, kinds, sel)
        with pytest.raises(ValueError, match="seeds"):
            EditPlan.build("cpu", sp, kinds, sel, seeds=[1])
    p = EditPlan.build("cpu", sp, ["sae_noise", "proj_noise"], sel, seeds=[2 ** 64 - 1, 5])
    assert p.kind.tolist() == [3, 4] and p.seeds.tolist() == [-1, 5]
    with pytest.raises(ValueError, match="reconstruct"):
        EditPlan.build("cpu", sp, ["sae_noise", "sae"], sel, seeds=[1, 2], mode="reconstruct")
    EditPlan.build("cpu", sp, ["proj_noise", "sae"], sel, seeds=[1, 2], mode="reconstruct")   # proj rows are unchanged
    assert EditPlan.build("cpu", sp, ["sae", "proj"], sel).seeds is None


# ---------------------------------------------------------------------------------------------------- sweep
SW = OVR + ["experiment.max_new_tokens=12", "intervention.budgets=[1, 4]", "intervention.noise_trials=2",
            "prompts=['Give me a hint!', 'Any hints available?', 'I need one more clue.']"]


def _records(cfg, m, tok, sae, methods, **kw):
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    r = SweepRunner(cfg, m, tok, sae, batch=60, device="cpu", layer=2, use_graphs=False, kv_pairs=8, **kw)
    pairs = r.build_pairs(["ship"], cfg.prompts)
    r.run_baselines(pairs)
    out = []
    for j in range(len(pairs)):
        out += r.run_cells([pairs[j]], r.make_cells([pairs[j]], methods), measure_nll=True)
    key = lambda x: (x["word"], x["prompt_idx"], x["method"], x["budget"], x["trial"])   # noqa: E731
    return {key(x): x for x in out}, r


@pytest.fixture(scope="module")
def sweeps():
    spec, m, tok, sae = _tiny()
    cfg = load_config(None, SW)
    on, off = dict(prefix_share=True, layer_resume=True), dict(prefix_share=False, layer_resume=False)
    return {"reuse": _records(cfg, m, tok, sae, NOISE_SWEEP, **on),
            "scratch": _records(cfg, m, tok, sae, NOISE_SWEEP, **off),
            "default": _records(cfg, m, tok, sae, ("sae_targeted", "sae_random", "proj_targeted", "proj_random"), **on)}


def test_sweep_reuse_equals_from_scratch(sweeps):
    a, b = sweeps["scratch"][0], sweeps["reuse"][0]
    assert set(a) == set(b) and {k[2] for k in a} == set(NOISE_SWEEP)
    assert sweeps["reuse"][1].stats["tf_rows"] > 0
    for k in a:
        assert a[k]["response_ids"] == b[k]["response_ids"], k
        assert a[k]["topk_ids"] == b[k]["topk_ids"], k
        assert abs(a[k]["nll_edit"] - b[k]["nll_edit"]) < 1e-5, k
        for f in ("p_secret_mean", "p_secret_final", "p_secret_max"):
            assert abs(a[k][f] - b[k][f]) < 1e-6 + 1e-5 * abs(a[k][f]), (k, f)
        assert a[k].get("edit_norm") == b[k].get("edit_norm")


def test_sweep_trials_differ_and_records_carry_the_edit_size(sweeps):
    got, runner = sweeps["reuse"]
    same = lambda a, b: a["response_ids"] == b["response_ids"] and a["nll_edit"] == b["nll_edit"]   # noqa: E731
    n_real = 0
    for (w, pi, meth, bud, t), r in got.items():
        if meth not in ("sae_noise", "proj_noise") or t != 0:
            continue
        tgt, other = got[(w, pi, meth.split("_")[0] + "_targeted", bud, 0)], got[(w, pi, meth, bud, 1)]
        assert r["seed"] != other["seed"]
        if tgt["nll_edit"] == tgt["nll_base"] and tgt["response_ids"] == runner_resp(runner, pi):
            assert same(r, tgt) and same(other, tgt)              # the targeted cell is its baseline: so are they
        else:
            n_real += 1
            assert not same(r, other) and not same(r, tgt) and not same(other, tgt), (w, pi, meth, bud)
    assert n_real >= 4
    for k, r in got.items():
        if k[2] in ("sae_noise", "proj_noise"):
            assert 0.0 < r["edit_norm"] < 10.0, (k, r["edit_norm"])
        else:
            assert "edit_norm" not in r
    from taboo_brittleness_amd.pipelines.sweep import summarize_cells

    curves = summarize_cells(list(got.values()), ["ship"], {"ship": ["ship", "ships"]})["curves"]
    for c in curves:
        assert ("edit_norm" in c) == (c["method"] in ("sae_noise", "proj_noise"))
        assert c["n"] == (6 if c["method"].endswith("noise") else 3)


def runner_resp(runner, pidx):
    return next(p.resp for p in runner._kv_pair.values() if p.pidx == pidx)


def test_default_methods_are_untouched(sweeps):
    """The default method set makes the cells it made, its records keep their keys, and the targeted records of a
    sweep with the controls equal those of a sweep without them."""
    from taboo_brittleness_amd.pipelines.sweep import METHODS, NOISE_METHODS

    assert METHODS == ("sae_targeted", "sae_random", "proj_targeted", "proj_random")
    assert NOISE_METHODS == ("sae_noise", "proj_noise")
    got, runner = sweeps["default"]
    assert runner._plan.seeds is None and runner._plan.has_noise == (False, False)
    pairs = list(runner._kv_pair.values())
    cells = runner.make_cells(pairs)
    assert [c.method for c in cells if c.pair == 0] == \
        ["sae_targeted"] * 2 + ["sae_random"] * 4 + ["proj_targeted"] * 2 + ["proj_random"] * 2
    assert {c.method for c in cells} == set(METHODS)
    assert all("edit_norm" not in r for r in got.values())
    noise = sweeps["reuse"][0]
    for k, r in got.items():
        if k[2].endswith("targeted"):
            assert r == noise[k], k
    assert load_config(None, OVR).intervention.noise_trials == 5
    n = sweeps["reuse"][1].make_cells(pairs, NOISE_SWEEP)
    assert sum(c.method == "sae_noise" for c in n) == len(pairs) * 2 * 2
    assert len({c.seed for c in n if c.method.endswith("noise")}) == len(pairs) * 2 * 2 * 2


def test_reconstruct_mode_rejects_sae_noise():
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    spec, m, tok, sae = _tiny()
    cfg = load_config(None, SW + ["intervention.ablation_mode=reconstruct"])
    r = SweepRunner(cfg, m, tok, sae, batch=8, device="cpu", layer=2, use_graphs=False)
    pairs = r.build_pairs(["ship"], cfg.prompts[:1])
    with pytest.raises(ValueError, match="reconstruct"):
        r.make_cells(pairs, ("sae_targeted", "sae_noise"))
    assert {c.method for c in r.make_cells(pairs, ("proj_targeted", "proj_noise"))} == {"proj_targeted", "proj_noise"}


# ------------------------------------------------------------------------------------- files and entry points
def test_run_sweep_all_noise_files_report_and_forcing(tmp_path):
    from taboo_brittleness_amd.cli.run_sweep import METHOD_SETS
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.pipelines.token_forcing import _FORCING_STATE
    from taboo_brittleness_amd.report.figures import make_report

    assert METHOD_SETS["all"] == ("sae_targeted", "sae_random", "proj_targeted", "proj_random")
    assert METHOD_SETS["all_noise"] == METHOD_SETS["all"] + ("sae_noise", "proj_noise")
    assert METHOD_SETS["sae_noise"] == METHOD_SETS["sae"] + ("sae_noise",)
    assert METHOD_SETS["proj_noise"] == METHOD_SETS["proj"] + ("proj_noise",)
    results = tmp_path / "results"
    out = str(results / "sweeps" / "noise")
    cfg = load_config(None, OVR + ["intervention.noise_trials=2", "intervention.measure_forcing=true",
                                   "intervention.forcing_trials=1", "token_forcing.max_new_tokens=3",
                                   "token_forcing.warmup_max_new_tokens=3"])
    summ = run_sweep(cfg, out, METHOD_SETS["all_noise"], info=DistInfo(), log=lambda *a: None)
    _FORCING_STATE.clear()
    disk = json.load(open(os.path.join(out, "sweep_summary.json")))
    assert disk["config"]["noise_trials"] == 2 and summ["config"]["noise_trials"] == 2
    by = {(c["method"], c["budget"]): c for c in disk["curves"]}
    for meth, xs in (("sae_noise", (1, 2)), ("proj_noise", (1, 2))):
        for b in xs:
            assert by[(meth, b)]["n"] == 4 and by[(meth, b)]["edit_norm"] > 0          # 2 prompts x 2 trials
    assert all("edit_norm" not in c for k, c in by.items() if not k[0].endswith("noise"))
    cells = [json.loads(l) for l in open(os.path.join(out, "sweep_cells.jsonl"))]
    assert len(cells) == 20 + 16
    assert all(("edit_norm" in c) == c["method"].endswith("noise") for c in cells)
    fc = {(c["method"], c["budget"]) for c in disk["forcing"]["curves"]}
    assert {("sae_noise", 1), ("sae_noise", 2), ("proj_noise", 1), ("proj_noise", 2)} <= fc
    made = make_report(str(results), str(tmp_path / "report"))
    figs = [p for p in made if os.path.basename(p).startswith(("fig1_ablation_saes_noise", "fig2_"))]
    assert len(figs) == 2 and all(os.path.getsize(p) > 0 for p in figs)
    # a sweep without the controls writes no noise_trials
    out2 = str(tmp_path / "plain")
    run_sweep(load_config(None, OVR + ["intervention.measure_forcing=false"]), out2, info=DistInfo(),
              log=lambda *a: None)
    assert "noise_trials" not in json.load(open(os.path.join(out2, "sweep_summary.json")))["config"]


def test_forcing_settings_take_the_noise_kinds():
    from taboo_brittleness_amd.pipelines.token_forcing import _FORCING_STATE, run_forcing, run_forcing_settings

    spec, m, tok, sae = _tiny()
    U = torch.linalg.qr(torch.randn(spec.hidden, 2, generator=torch.Generator().manual_seed(1)))[0].t().contiguous()
    settings = [{"word": "ship", "kind": "none"},
                {"word": "ship", "kind": "sae_noise", "latents": [3, 7], "alpha": 1.0, "seed": 5},
                {"word": "ship", "kind": "proj_noise", "basis": U, "seed": 2 ** 63 + 9},
                {"word": "ship", "kind": "sae", "latents": [3, 7], "alpha": 1.0}]
    cfg = load_config(None, OVR + ["token_forcing.max_new_tokens=4"])
    res = run_forcing_settings(cfg, m, tok, settings, "pregame", sae, 2)
    assert len(res) == 4 and all(r["n"] > 0 for r in res)
    pl = _FORCING_STATE[id(m)]["hooks"].plan
    assert pl.has_noise == (True, True) and pl.any_position and {3, 4} <= set(pl.kind.tolist())
    assert 5 in pl.seeds.tolist()
    _FORCING_STATE.clear()
    one = run_forcing(cfg, m, tok, ["ship"], "pregame", sae, 2, {"kind": "proj_noise", "basis": U, "seed": 3})
    assert one["rows"] and "clamp_value" not in one
    with pytest.raises(ValueError, match="reconstruct"):
        run_forcing_settings(load_config(None, OVR + ["intervention.ablation_mode=reconstruct"]), m, tok, settings[:2],
                             "pregame", sae, 2)
    _FORCING_STATE.clear()
    res = run_forcing_settings(cfg, m, tok, settings[:1] + settings[3:], "pregame", sae, 2)
    assert _FORCING_STATE[id(m)]["hooks"].plan.seeds is None       # plans without the controls are what they were
    _FORCING_STATE.clear()


def test_cli_accepts_the_noise_method_sets(tmp_path):
    from taboo_brittleness_amd.cli import run_sweep as cli

    out = str(tmp_path / "cli")
    sets = [a for o in OVR + ["intervention.noise_trials=1", "intervention.budgets=[1]"] for a in ("--set", o)]
    summ = cli.main(sets + ["--methods", "sae_noise", "--out", out])
    assert {c["method"] for c in summ["curves"]} == {"sae_targeted", "sae_random", "sae_noise"}
    assert summ["config"]["noise_trials"] == 1
    with pytest.raises(SystemExit):
        cli.main(sets + ["--methods", "noise", "--out", out])
