"""Layer trace off the GPU: the criterion of tests/layer_trace_cases.py cannot pass vacuously, ops/reference.py meets it
and planted bugs do not, ``ops.lens_track`` validates its arguments, the kernel compiles without scratch, ``TraceHook``
fills its slabs, and the CPU sweep with ``intervention.layer_trace``: every cell's ``trace_*`` fields against plain
full-sequence forwards of the edited and the unedited model, the last block against the model's own logits, exact
zeros where nothing fires, unchanged records without the switch, the combinations that raise, the files and fig6."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from layer_trace_cases import (EPS, TRACE_CAPS, TRACE_D, TRACE_M, TRACE_T, TRACE_U, U32, check_trace, lens_z, run_trace,
                               trace_case, trace_mutant, trace_truth, trace_vrow)
from taboo_brittleness_amd import ops
from taboo_brittleness_amd.config import load_config
from taboo_brittleness_amd.ops import reference as ref
from test_head_shift_cpu import OVR, run_tiny, tiny

BF = torch.bfloat16
CPU = torch.device("cpu")
TRACE = ["intervention.layer_trace=true"]
LISTS = ("trace_dz_spike", "trace_dz_mean", "trace_z_base_spike", "trace_decoy_dz_spike")
KEYS = LISTS + ("trace_recovery",)


# ---------------------------------------------------------------------------------------------- criterion and op
@pytest.mark.parametrize("D", TRACE_D)
def test_cases_hold_what_they_must_and_the_bound_can_fail(D):
    """The row maps are unsorted, repeated and hold both out-of-range values; the truth is far above its bound on
    most elements (a result of 0, or one not tied to the inputs, fails); skipped rows and the absent id are marked."""
    for M in TRACE_M[1:]:
        v = trace_vrow(M).tolist()
        assert -1 in v and TRACE_U in v and len(set(v)) < len(v) and v != sorted(v)
    for T in TRACE_T:
        h, V, vrow = trace_case(D, T, 257)
        for cap in TRACE_CAPS:
            t = trace_truth(h, V, vrow, EPS, cap)
            live = t["ok"][:, None] & ~t["zero"]
            assert int(live.sum()) > 100 * T and bool((t["bound"][live] > 0).all())
            # |z| / bound is about 1 / (D^1.5 u) for random rows: 80 at the widest D, tens of thousands at the narrowest
            assert float((t["f"].abs() > 10 * t["bound"])[live].double().mean()) > 0.8, (T, cap)
            assert bool(t["zero"][~t["ok"]].all()) and bool((t["f"][t["zero"]] == 0).all())
            assert bool(t["zero"][(vrow == 1)][:, T - 1].all())
            assert check_trace(torch.zeros(257, T), t)                 # all zeros is rejected


@pytest.mark.parametrize("D", TRACE_D)
@pytest.mark.parametrize("T", TRACE_T)
def test_reference_meets_the_criterion(D, T):
    assert not run_trace(ops.lens_track, CPU, D, T)
    assert not run_trace(lambda h, V, vr, eps, cap, out=None: ref.lens_track(h, V, vr, eps, cap).float(), CPU, D, T)


@pytest.mark.parametrize("D", TRACE_D)
@pytest.mark.parametrize("T", TRACE_T)
def test_planted_bugs_are_rejected(D, T):
    """Each stand-in fails wherever its bug can show: the dropped tail, the wrong mean square and the missing ``eps``
    (the rows with ``|h|^2 / D`` near ``eps``) everywhere, the wrong table stride from two columns on."""
    assert not run_trace(trace_mutant(), CPU, D, T)                    # the stand-in itself is sound
    for bug in ("drop_tail", "rms_is_d", "no_eps"):
        bad = run_trace(trace_mutant(**{bug: True}), CPU, D, T, Ms=(5, 257))
        assert bad and all("want exactly" not in b for b in bad), (bug, bad[:2])
    bad = run_trace(trace_mutant(t_stride=True), CPU, D, T, Ms=(5, 257))
    assert bool(bad) == (T > 1), bad[:2]


def test_op_validates_and_maps():
    h, V, vrow = trace_case(64, 3, 5)
    out = ops.lens_track(h, V, vrow, EPS, 30.0)
    assert out.dtype == torch.float32 and out.shape == (5, 3)
    assert torch.equal(out, ref.lens_track(h, V, vrow, EPS, 30.0).float())
    assert not out[2].any() and not out[3].any() and out[0].all() and out[1].all()
    o = torch.full((5, 3), 7.0)
    assert ops.lens_track(h, V, vrow, EPS, 30.0, out=o) is o and torch.equal(o, out)
    assert ops.lens_track(h[:0], V, vrow[:0], EPS, 30.0).shape == (0, 3)
    none = ops.lens_track(h, V[:0], vrow, EPS, 30.0)                   # no table block: every row is skipped
    assert none.shape == (5, 3) and not none.any()
    hb = torch.zeros(5, 4104, dtype=BF)
    for bad in (dict(h=h.float()), dict(h=h[0]), dict(V=V.double()), dict(V=V[0]), dict(V=V[:, :, :32]),
                dict(V=torch.zeros(3, 9, 64)), dict(V=torch.zeros(3, 0, 64)), dict(vrow=vrow.long()),
                dict(vrow=vrow[:4]), dict(vrow=vrow.view(5, 1)), dict(out=torch.zeros(5, 2)),
                dict(out=torch.zeros(5, 3, dtype=torch.float64)), dict(h=hb, V=torch.zeros(3, 3, 4104)),
                dict(h=hb[:, :60], V=torch.zeros(3, 3, 60))):
        with pytest.raises(ValueError):
            ops.lens_track(bad.get("h", h), bad.get("V", V), bad.get("vrow", vrow), EPS, 30.0, out=bad.get("out"))


def test_trace_kernel_uses_no_scratch(tmp_path):
    """lens_track.hip compiled for gfx950 with the extension's flags: the compiler's resource-usage remarks list one
    kernel per T = 1..8, each with 0 bytes of scratch and a register count that lets its 256 threads (one wave per
    SIMD: up to 512 registers) launch -- held to 256, two workgroups per CU at least."""
    from taboo_brittleness_amd import build as b

    hipcc = os.path.join(b.ROCM, "bin", "hipcc")
    cmd = [hipcc, f"--offload-arch={b.ARCH}", "-c", os.path.join(b.CSRC, "lens_track.hip"), "-o",
           str(tmp_path / "lens_track.o"), "--cuda-device-only", "-munsafe-fp-atomics", "-fPIC", "-O3", "-std=c++17",
           "-I", b.CSRC, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    mine = [x for x in blocks if "lens_track_kernel" in x.split()[0]]
    assert len(mine) == 8, [x.split()[0] for x in blocks]
    for x in mine:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", x).group(1)) == 0, x
        assert int(re.search(r"VGPRs: (\d+)", x).group(1)) <= 256, x
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", x).group(1)) <= 8 * 2048, x


def test_trace_hook_fills_its_slabs():
    """Two chunks of a 7-row launch, each padded to 8 rows, at blocks 1 and 2: every slab row equals the op on that
    row alone, padding rows are skipped, a block outside the hook's range and a forward of another size raise."""
    from types import SimpleNamespace

    from taboo_brittleness_amd.interp.edits import TraceHook

    h, V, vrow = trace_case(64, 3, 5)
    g = torch.Generator().manual_seed(3)
    H = {l: torch.randn(2, 8, 64, generator=g).to(BF) for l in (1, 2)}
    rows = torch.tensor([2, 0, -1, 1, 1, 0, 2], dtype=torch.int32)
    out = torch.full((2, 7, 3), float("nan"))
    hk = TraceHook(V, rows, out, 1, EPS, 30.0)
    assert list(hk.layers) == [1, 2]
    for ci, (r0, r1) in enumerate(((0, 4), (4, 7))):
        hk.use_rows(r0, r1, 8)
        for l in (1, 2):
            hk(H[l][ci], None, SimpleNamespace(layer=l))
    for l in (1, 2):
        for i in range(7):
            ci, k = (0, i) if i < 4 else (1, i - 4)
            want = ops.lens_track(H[l][ci][k:k + 1], V, rows[i:i + 1], EPS, 30.0)
            assert torch.equal(out[l - 1, i], want[0]), (l, i)
    assert not out[:, 2].any() and hk.calls == 4
    with pytest.raises(ValueError):
        hk(H[1][0], None, SimpleNamespace(layer=3))
    with pytest.raises(ValueError):
        hk(H[1][0][:5], None, SimpleNamespace(layer=1))
    with pytest.raises(ValueError):
        TraceHook(V, rows.long(), out, 1, EPS, 30.0)


# ------------------------------------------------------------------------------------------------------ sweep
@pytest.fixture(scope="module")
def sweeps():
    on = run_tiny(TRACE)
    return {"on": on, "off": run_tiny([], model=on[4])}


class _Grab:
    def __init__(self):
        self.h = {}

    def __call__(self, h, x, ctx):
        self.h[ctx.layer] = h.detach().reshape(-1, h.shape[-1]).clone()


def _full_forward(m, r, p, b, hook=None):
    """Blocks 1 and 2 residual rows (after the edit at block 1) and final-normed rows over the response of pair ``p``,
    from a plain forward of prompt + baseline response in slot ``b``."""
    full = p.ids + p.resp
    ids = torch.tensor([full], dtype=torch.int32)
    pos = torch.arange(len(full), dtype=torch.int32)[None]
    g = _Grab()
    hooks = {r.layer: ([hook] if hook is not None else []) + [g], r.layer + 1: [g]}
    x = m.forward(ids, pos, m.new_cache(r.B, len(full) + 1), torch.tensor([b], dtype=torch.int32), hooks)
    return [g.h[l][p.plen:] for l in (r.layer, r.layer + 1)], x.reshape(-1, x.shape[-1])[p.plen:]


def test_sweep_fields_match_full_forwards(sweeps):
    """Per cell: a plain forward of prompt + baseline response through the edited model (the cell's plan row) and one
    through the unedited model, capture hooks at blocks 1 and 2, the float64 ``z`` of every row, then the record's own
    reductions.  A row's tolerance is its bound (layer_trace_cases.py), a difference's the sum of the two rows'
    bounds, a field's the same reduction of those."""
    _got, r, pairs, cells, (spec, m, _tok, _sae) = sweeps["on"]
    hook = r._hook                                              # plan row b = cell b (one batch)
    assert spec.layers - r.layer == 2
    moved = 0
    for b, (c, rec) in enumerate(cells):
        p = pairs[c.pair]
        n = len(p.resp)
        he, _ = _full_forward(m, r, p, b, hook)
        hb, _ = _full_forward(m, r, p, b)
        sp = [s for s in p.spikes_rel if s < n]
        dec = list(range(2, 2 + p.n_decoys))
        for k in range(2):
            te, tb = lens_z(m, he[k], p.track), lens_z(m, hb[k], p.track)
            dz = te["f"] - tb["f"]                              # [n, T]
            tol = te["bound"] + tb["bound"]
            same = (he[k] == hb[k]).all(-1)                     # rows no edit reached: exactly the baseline's
            assert bool((dz[same] == 0).all())
            tol = torch.where(same[:, None], torch.zeros_like(tol), tol)
            want = {"trace_dz_spike": float(dz[sp, 0].sum()) / len(sp) if sp else 0.0,
                    "trace_dz_mean": float(dz[: n - 1, 0].sum()) / n if n else 0.0,
                    "trace_z_base_spike": float(tb["f"][sp, 0].sum()) / len(sp) if sp else 0.0,
                    "trace_decoy_dz_spike": float(dz[sp][:, dec].sum()) / (len(sp) * len(dec)) if sp and dec else 0.0}
            tols = {"trace_dz_spike": float(tol[sp, 0].sum()) / len(sp) if sp else 0.0,
                    "trace_dz_mean": float(tol[: n - 1, 0].sum()) / n if n else 0.0,
                    "trace_z_base_spike": float(tb["bound"][sp, 0].sum()) / len(sp) if sp else 0.0,
                    "trace_decoy_dz_spike": float(tol[sp][:, dec].sum()) / (len(sp) * len(dec)) if sp and dec else 0.0}
            for f in LISTS:
                assert len(rec[f]) == 2
                assert abs(rec[f][k] - want[f]) <= tols[f] + 1e-300, (b, c.method, c.budget, k, f, rec[f][k], want[f],
                                                                     tols[f])
            if k == 0:
                moved += abs(want["trace_dz_spike"]) > 10 * tols["trace_dz_spike"] > 0
        d0, d1 = rec["trace_dz_spike"]
        assert (rec["trace_recovery"] != rec["trace_recovery"]) if d0 == 0.0 else rec["trace_recovery"] == 1.0 - d1 / d0
    assert moved >= len(cells) // 2                             # the comparison is not one of zeros


def test_last_block_matches_the_models_own_logits(sweeps):
    """The trace of the last block reads the row the model's head reads, so the baseline's trace there must agree with
    the capped bf16 ``m.logits`` entry of the same row and token, up to what the model's bf16 chain loses.

    Derivation, for one row and token, ``w = 2^-9`` the bf16 unit roundoff: the final norm rounds each normed entry
    ``h_d (1 + g_d) / r`` once to bf16 (its fp32 steps are of order ``u``): ``w S / r`` on the logit.  The unembedding
    accumulates bf16 products in fp32 (``gamma S / r``) and rounds the logit ``x`` to bf16: ``w |x|``.  The softcap
    chain ``rbf(rbf(tanh(rbf(x / cap))) cap)`` rounds three times; ``tanh`` is 1-Lipschitz and ``|cap tanh| <= |x|``,
    so each rounding moves the result by at most ``w |x|``: ``3 w |x|``.  With ``|x| <= |z| + (w + gamma) S / r``:
    ``tol = (w + gamma) S / r (1 + 4 w) + 4 w |z|`` plus the trace's own bound.  On rows with ``S / r >= 2 |z|`` this
    is below the ``2^-8 (S / r + |z|)`` of the feature's specification; the test checks that too."""
    _got, r, pairs, _cells, (spec, m, _tok, _sae) = sweeps["on"]
    w = 2.0 ** -9
    D = spec.hidden
    gam = D * U32 / (1 - D * U32)
    seen = 0
    for b, p in enumerate(pairs):
        n = len(p.resp)
        hb, x = _full_forward(m, r, p, b)
        lg = m.logits(x)[:, [int(t) for t in p.track]]
        got = ref.softcap_bf16(lg, spec.final_softcap).double()              # [n, T] capped bf16 logits
        t = lens_z(m, hb[1], p.track)
        zb = p.z_base[1].double()[:, -1, : len(p.track)]                    # the sweep's own baseline trace
        assert bool(((zb - t["f"]).abs() <= t["bound"]).all())
        tol = (w + gam) * t["S_over_r"] * (1 + 4 * w) + 4 * w * t["z"].abs() + t["bound"]
        loose = 2.0 ** -8 * (t["S_over_r"] + t["z"].abs()) + t["bound"] + gam * t["S_over_r"]
        assert bool((tol <= loose)[t["S_over_r"] >= 2 * t["z"].abs()].all())
        err = (zb - got).abs()
        assert bool((err <= tol).all()), (b, float((err - tol).max()))
        seen += int((got.abs() > 10 * tol).sum())
    assert seen > 0


def test_sweep_zero_cells_and_unchanged_records(sweeps):
    """A cell none of whose latents fire at any spike is its baseline: every trace field exactly 0 (its recovery is
    undefined).  Without the switch the records have no such keys and are otherwise what the run with it gives, and
    neither a ``lens_track`` launch nor the baseline pass shows in the stats."""
    on, r, pairs, cells, _ = sweeps["on"]
    off, r_off = sweeps["off"][0], sweeps["off"][1]
    assert set(on) == set(off) and not r_off.layer_trace and r.layer_trace
    for k in on:
        assert set(on[k]) - set(off[k]) == set(KEYS) and not set(off[k]) - set(on[k]), k
        for f in off[k]:
            assert on[k][f] == off[k][f] or (on[k][f] != on[k][f] and off[k][f] != off[k][f]), (k, f)
        assert not any(f.startswith("trace_") for f in off[k])
    sae_cells = [(c, rec) for c, rec in cells if c.kind == "sae"]
    f = r._plan_for([c for c, _ in sae_cells], pairs, {}, with_carry=False)["f"][: len(sae_cells)]
    noop = [(c, rec) for (c, rec), fc in zip(sae_cells, f) if fc >= len(pairs[c.pair].resp)]
    for c, rec in noop:
        assert all(v == 0.0 for k in LISTS if k != "trace_z_base_spike" for v in rec[k]), (c, rec)
        assert rec["trace_recovery"] != rec["trace_recovery"] and rec["response_ids"] == pairs[c.pair].resp
    for c, rec in cells:
        assert all(math.isfinite(v) for k in LISTS for v in rec[k])
        assert rec["trace_z_base_spike"] == cells[[cc.pair for cc, _ in cells].index(c.pair)][1]["trace_z_base_spike"]
    for key in ("trace_rows", "trace_base_rows", "shift_base_pass_rows", "shift_base_rows"):
        assert key not in r_off.stats
    assert r.stats["trace_rows"] == 2 * r.stats["tf_rows"] and r.stats["trace_base_rows"] > 0
    assert "shift_base_pass_rows" not in r.stats and all(p.x_base is None and p.z_base is not None for p in pairs)
    assert all(p.z_base is None for p in sweeps["off"][2])


def test_sweep_noop_cell_is_exactly_zero():
    """Cells whose latents never fire, made so by hand (pair 0's targeted latents replaced by latents that are
    inactive at every one of its spikes), next to pair 1's cells, which do edit: exact zeros in every difference,
    while the batch's other cells move."""
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    spec, m, tok, sae = tiny()
    cfg = load_config(None, OVR + TRACE)
    r = SweepRunner(cfg, m, tok, sae, batch=40, device="cpu", layer=1, use_graphs=False, kv_pairs=8)
    pairs = r.build_pairs(["ship"], cfg.prompts[:2], ("sae_targeted",))
    r.run_baselines(pairs)
    p = pairs[0]
    enc = sae.encode(p.resid[[t for t in p.spikes_rel if t < len(p.resp)]])
    dead = [int(i) for i in (enc.float().abs().sum(0) == 0).nonzero().reshape(-1)[:8]]
    assert len(dead) == 8 and p.spikes_rel
    p.targeted = dead
    cells = r.make_cells(pairs, ("sae_targeted",))
    res = r.run_cells(pairs, cells, measure_nll=True)
    mine = [x for c, x in zip(cells, res) if c.pair == 0]
    assert mine and len(mine) < len(res)
    for x in mine:
        assert all(v == 0.0 for k in LISTS if k != "trace_z_base_spike" for v in x[k]), x
        assert any(v != 0.0 for v in x["trace_z_base_spike"]) and x["response_ids"] == p.resp
    assert any(abs(x["trace_dz_spike"][0]) > 1e-4 for c, x in zip(cells, res) if c.pair == 1)


def test_swap_cells_report_the_donor_column():
    """Swap runs track the other words' secrets; their cells carry ``trace_dz_donor_spike``, the others do not."""
    ovr = [o for o in OVR if not o.startswith("word_plurals")] + ["word_plurals={ship: [ship, ships], moon: [moon]}"]
    methods = ("sae_targeted", "sae_swap")
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    spec, m, tok, sae = tiny()
    cfg = load_config(None, ovr + TRACE)
    r = SweepRunner(cfg, m, tok, sae, batch=40, device="cpu", layer=1, use_graphs=False, kv_pairs=8)
    pairs = r.build_pairs(["ship", "moon"], cfg.prompts[:2], methods)
    r.run_baselines(pairs)
    cells = r.make_cells(pairs, methods)
    res = r.run_cells(pairs, cells, measure_nll=True)
    sw = [x for c, x in zip(cells, res) if c.method == "sae_swap"]
    assert sw and all(len(x["trace_dz_donor_spike"]) == 2 for x in sw)
    assert all("trace_dz_donor_spike" not in x for c, x in zip(cells, res) if c.method != "sae_swap")


def test_unsupported_combinations_raise(tmp_path):
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    with pytest.raises(ValueError, match="tensor-parallel"):
        run_sweep(load_config(None, OVR + TRACE + ["parallel.tp=2"]), str(tmp_path / "tp"), log=lambda *a: None)
    spec, m, tok, sae = tiny()
    cfg = load_config(None, OVR + TRACE)
    mk = lambda **kw: SweepRunner(cfg, m, tok, sae, batch=8, device="cpu", layer=1, use_graphs=False, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="layer resume"):
        mk(layer_resume=False)
    with pytest.raises(ValueError, match="layer resume"):
        mk(prefix_share=False)
    with pytest.raises(ValueError, match="layer resume"):
        SweepRunner(load_config(None, OVR + TRACE + ["runtime.layer_resume=false"]), m, tok, sae, batch=8, device="cpu",
                    layer=1, use_graphs=False)
    m.tp = object()
    try:
        with pytest.raises(ValueError, match="tensor-parallel"):
            mk()
    finally:
        m.tp = None
    m.fused_head = True                                          # the trace does not touch the head: no objection
    try:
        assert mk().layer_trace
    finally:
        m.fused_head = False
    r = mk(kv_pairs=8)
    pairs = r.build_pairs(["ship"], cfg.prompts[:2])
    r.run_baselines(pairs)
    r.carry_rows = 4
    with pytest.raises(ValueError, match="carry-over"):
        r.run_cells(pairs, r.make_cells(pairs)[:4])
    r.carry_rows = 0
    r.layer_resume = False                                       # switched off behind the constructor's back
    with pytest.raises(ValueError, match="layer-resume"):
        r.run_cells(pairs, r.make_cells(pairs)[:4])
    r9 = mk()
    r9.iv.decoys = {"ship": [f"w{i}" for i in range(7)]}
    try:
        with pytest.raises(ValueError, match="at most 8"):
            r9.build_pairs(["ship"], cfg.prompts[:1])
    finally:
        r9.iv.decoys = {}


def test_run_sweep_files_and_report(tmp_path):
    """``sweep_trace.csv``, the summary's per-block curves, the cell records and fig6 carry the trace only when
    enabled; the other files of the run are what they are without it."""
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.report.figures import make_report

    results = tmp_path / "results"
    ovr = [o for o in OVR if not o.startswith("experiment.max_new_tokens")] + ["experiment.max_new_tokens=5"]
    texts, curves = {}, {}
    for tag, extra in (("on", TRACE), ("off", [])):
        out = str(results / "sweeps" / tag)
        summ = run_sweep(load_config(None, ovr + extra), out, info=DistInfo(), log=lambda *a: None)
        texts[tag] = open(os.path.join(out, "sweep_cells.jsonl")).read()
        curves[tag] = open(os.path.join(out, "sweep_curves.csv")).read()
        cells = [json.loads(l) for l in texts[tag].splitlines()]
        if tag == "off":
            assert "layer_trace" not in summ["config"] and "trace_blocks" not in summ["config"]
            assert not os.path.exists(os.path.join(out, "sweep_trace.csv"))
            assert not any(k.startswith("trace_") for c in summ["curves"] for k in c)
            assert not any(k.startswith("trace_") for c in cells for k in c)
            continue
        blocks = summ["config"]["trace_blocks"]                 # the tiny preset's blocks from the hooked one on
        assert summ["config"]["layer_trace"] is True and blocks == list(range(1, 1 + len(blocks))) and len(blocks) >= 2
        assert all(set(KEYS) <= set(c) for c in cells)
        lines = open(os.path.join(out, "sweep_trace.csv")).read().splitlines()
        assert lines[0].startswith("method,budget,n,block,trace_dz_spike,") and \
            len(lines) == 1 + len(blocks) * len(summ["curves"])
        assert {l.split(",")[3] for l in lines[1:]} == {str(b) for b in blocks}
        for c in summ["curves"]:
            assert len(c["trace_dz_spike"]) == len(blocks)
            for ci in c["trace_dz_spike"]:
                assert ci["lo"] <= ci["mean"] <= ci["hi"], c["method"]
            rc = c["trace_recovery"]
            assert rc["n"] == 0 or rc["lo"] <= rc["mean"] <= rc["hi"]
    strip = lambda t: [{k: v for k, v in json.loads(l).items() if k not in KEYS} for l in t.splitlines()]   # noqa: E731
    assert json.dumps(strip(texts["on"])) == json.dumps([json.loads(l) for l in texts["off"].splitlines()])
    assert curves["on"] == curves["off"]
    made = [os.path.basename(p) for p in make_report(str(results), str(tmp_path / "report"))]
    assert [p for p in made if p.startswith("fig6_layer_trace")] == ["fig6_layer_trace_on.png"]
    assert os.path.getsize(tmp_path / "report" / "fig6_layer_trace_on.png") > 0


def test_cli_flag_sets_the_switch():
    import inspect

    from taboo_brittleness_amd.cli import run_sweep as cli

    src = inspect.getsource(cli.main)
    assert "--layer-trace" in src and "layer_trace = True" in src
    assert load_config(None, []).intervention.layer_trace is False and np.isfinite(EPS)
