"""Output shift off the GPU: the criteria of tests/shift_cases.py cannot pass vacuously, ops/reference.py meets them and
planted bugs do not, ``ops.head_shift`` validates its arguments, and the CPU sweep with ``intervention.output_shift``:
every cell's ``kl_out_*`` fields against plain full-sequence forwards of the edited and the unedited model, exact zeros
where nothing fires, unchanged records without the switch, the combinations that raise, the files and fig5."""
import json
import math
import os
import re
import subprocess
from dataclasses import replace

import pytest
import torch

from readout_cases import STREAM_WIDTHS
from shift_cases import (KINDS, ROWMAPS, SHIFT_CAPS, SHIFT_RB, case_truth, run_shift, shift_case, shift_mutant,
                         shift_truth)
from taboo_brittleness_amd import ops
from taboo_brittleness_amd.config import load_config
from taboo_brittleness_amd.ops import reference as ref

BF = torch.bfloat16
CPU = torch.device("cpu")
KEYS = ("kl_out_mean", "kl_out_max", "kl_out_spike_mean", "kl_rev_out_mean")
SHIFT = ["intervention.output_shift=true"]


# ---------------------------------------------------------------------------------------------- criteria and op
@pytest.mark.parametrize("V", STREAM_WIDTHS)
def test_truth_is_nonnegative_and_the_bound_can_fail(V):
    """The float64 truth is a KL (>= 0 up to float64 rounding); the rowmaps hold what they must; in the one-entry
    case the bound lies below the smallest truth, so a result of 0 -- or any value not tied to the inputs -- fails."""
    assert -1 in ROWMAPS[5] and SHIFT_RB in ROWMAPS[5] and len(set(ROWMAPS[5])) < 5 and ROWMAPS[5][0] > ROWMAPS[5][2]
    for cap in SHIFT_CAPS:
        for kind in KINDS:
            for R in (1, 3, 5):
                t = case_truth(V, kind, R, cap)
                assert float(t["kl"].min()) >= -1e-12 and float(t["kl_rev"].min()) >= -1e-12, (kind, R)
                assert bool((t["kl"][t["same"]].abs() < 1e-12).all())
                if kind == "identical":
                    assert bool(t["same"][t["ok"]].all())
                if kind == "one_entry" and V > 1:
                    live = t["ok"]
                    assert int(live.sum()) > 0 and not bool(t["same"][live].any())
                    for k, b in (("kl", "bound"), ("kl_rev", "bound_rev")):
                        assert float(t[b][live].max()) < float(t[k][live].min()), (k, R, cap)


@pytest.mark.parametrize("V", STREAM_WIDTHS)
def test_reference_meets_the_criteria(V):
    run_shift(ops.head_shift, CPU, V).assert_ok(f"reference head_shift V {V}")
    run_shift(lambda lg, b, rm, cap, **kw: ref.head_shift(lg, b, rm, cap), CPU, V, fill=False).assert_ok(
        f"ref.head_shift V {V}")


@pytest.mark.parametrize("V", STREAM_WIDTHS)
def test_planted_bugs_are_rejected(V):
    """Each stand-in fails at every width where its bug can show: the dropped tail wherever ``V % 8 != 0`` (the
    one-entry rows plant their logit in the last column), the wrong sum everywhere, the ignored rowmap from two
    columns on."""
    assert not run_shift(shift_mutant(), CPU, V).failures                      # the stand-in itself is sound
    rep = run_shift(shift_mutant(drop_tail=True), CPU, V)
    assert rep.failed("one_entry") == (V % 8 != 0 and V > 1), rep.failures[:3]    # V = 1: every KL is 0
    rep = run_shift(shift_mutant(swap_sum=True), CPU, V)
    assert rep.failed("kl ", "gain16") and rep.failed("kl ", "negation") and (V == 1 or rep.failed("kl ", "one_entry"))
    assert not rep.failed("identical")
    rep = run_shift(shift_mutant(ignore_map=True), CPU, V)
    if V > 1:                                    # one column: every distribution is the same, nothing can show
        assert rep.failed("identical", "want exactly 0") and rep.failed("unmapped") and rep.failed("gain1")


def test_op_validates_and_maps():
    z, y, rm, _ = shift_case(4104, "gain1", 5)
    kl, klr = ops.head_shift(z, y, rm, 30.0)
    a, b = ref.head_shift(z, y, rm, 30.0)
    assert torch.equal(kl, a) and torch.equal(klr, b) and kl.dtype == torch.float32 and kl.shape == (5,)
    assert kl[1] == 0 and kl[3] == 0 and klr[1] == 0 and klr[3] == 0 and kl[0] > 0 and kl[4] > 0
    o1, o2 = torch.full((5,), 7.0), torch.full((5,), 7.0)
    r1, r2 = ops.head_shift(z, y, rm, 30.0, o1, o2)
    assert r1 is o1 and r2 is o2 and torch.equal(o1, kl) and torch.equal(o2, klr)
    e = ops.head_shift(z[:0], y, rm[:0], 30.0)
    assert e[0].shape == (0,) and e[1].shape == (0,)
    nob = ops.head_shift(z, y[:0], torch.zeros(5, dtype=torch.int32), 30.0)       # no baseline rows: all unmapped
    assert not nob[0].any() and not nob[1].any()
    for bad in (dict(base=y[:, :-1]), dict(base=y.float()), dict(logits=z.float()), dict(logits=z[0]),
                dict(rowmap=rm.long()), dict(rowmap=rm[:4]), dict(rowmap=rm.view(5, 1)), dict(kl=torch.zeros(4)),
                dict(kl_rev=torch.zeros(5, dtype=torch.float64)), dict(logits=z[:, :0], base=y[:, :0])):
        with pytest.raises(ValueError):
            ops.head_shift(bad.get("logits", z), bad.get("base", y), bad.get("rowmap", rm), 30.0, bad.get("kl"),
                           bad.get("kl_rev"))


def test_shift_kernel_uses_no_scratch(tmp_path):
    """lens.hip compiled for gfx950 with the extension's flags: the compiler's resource-usage remarks list the shift
    kernel with 0 bytes of scratch and a register count that lets its 512 threads (8 waves on 4 SIMDs) launch."""
    from taboo_brittleness_amd import build as b

    hipcc = os.path.join(b.ROCM, "bin", "hipcc")
    cmd = [hipcc, f"--offload-arch={b.ARCH}", "-c", os.path.join(b.CSRC, "lens.hip"), "-o", str(tmp_path / "lens.o"),
           "--cuda-device-only", "-munsafe-fp-atomics", "-fPIC", "-O3", "-std=c++17", "-I", b.CSRC,
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    mine = [x for x in blocks if "head_shift_kernel" in x.split()[0]]
    assert len(mine) == 1, [x.split()[0] for x in blocks]
    assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0]).group(1)) == 0, mine[0]
    assert int(re.search(r"VGPRs: (\d+)", mine[0]).group(1)) <= 128, mine[0]


# ------------------------------------------------------------------------------------------------------ sweep
OVR = ["model.arch=gemma2-tiny", "model.layer_idx=1", "word_plurals={ship: [ship, ships]}",
       "prompts=['Give me a hint!', 'Any hints available?']", "experiment.max_new_tokens=10",
       "intervention.budgets=[1, 4]", "intervention.random_trials=2", "intervention.ranks=[1, 2]",
       "intervention.proj_random_trials=1", "intervention.noise_trials=1", "sae.d_sae=512", "runtime.batch_size=8",
       "runtime.device=cpu", "runtime.use_graphs=false"]
METHODS = ("sae_targeted", "sae_random", "sae_noise", "proj_targeted", "proj_random")


def tiny():
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.gemma2 import Gemma2Model
    from taboo_brittleness_amd.models.spec import GEMMA2_TINY
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.models.weights import random_gemma2

    spec = replace(GEMMA2_TINY, vocab_size=1024, layers=3, hidden=256, ffn=512)
    m = Gemma2Model(random_gemma2(spec, dtype=BF, seed=7, norm_std=0.1), "cpu")
    return spec, m, SyntheticTokenizer(vocab_size=spec.vocab_size), JumpReLUSAE.random(spec.hidden, 512, seed=2,
                                                                                      device="cpu")


def run_tiny(extra, methods=METHODS, device="cpu", model=None, **kw):
    """One batch of every cell of two pairs: ``(records by key, runner, pairs, cells, model)``."""
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    spec, m, tok, sae = model or tiny()
    cfg = load_config(None, OVR + list(extra))
    r = SweepRunner(cfg, m, tok, sae, batch=40, device=device, layer=1, use_graphs=False, kv_pairs=8)
    for k, v in kw.items():
        setattr(r, k, v)
    pairs = r.build_pairs(["ship"], cfg.prompts[:2], methods)
    r.run_baselines(pairs)
    cells = r.make_cells(pairs, methods)
    assert len(cells) <= r.B
    res = r.run_cells(pairs, cells, measure_nll=True)
    key = lambda x: (x["word"], x["prompt_idx"], x["method"], x["budget"], x["trial"])   # noqa: E731
    return {key(x): x for x in res}, r, pairs, list(zip(cells, res)), (spec, m, tok, sae)


@pytest.fixture(scope="module")
def sweeps():
    on = run_tiny(SHIFT)
    return {"on": on, "off": run_tiny([], model=on[4])}


def test_sweep_fields_match_full_forwards(sweeps):
    """Per cell: a plain forward of prompt + baseline response through the edited model (the cell's plan row) and one
    through the unedited model, float64 KL of their capped logits row by row, then the record's own reductions.  A
    row's tolerance is its ``shift_bound``; the fields' are the same reductions of the rows' bounds."""
    _got, r, pairs, cells, (spec, m, _tok, _sae) = sweeps["on"]
    hook = r._hook                                              # plan row b = cell b (one batch)
    cap = spec.final_softcap
    moved = 0
    for b, (c, rec) in enumerate(cells):
        p = pairs[c.pair]
        n = len(p.resp)
        full = p.ids + p.resp
        ids = torch.tensor([full], dtype=torch.int32)
        pos = torch.arange(len(full), dtype=torch.int32)[None]
        slot = torch.tensor([b], dtype=torch.int32)
        le = m.logits(m.forward(ids, pos, m.new_cache(r.B, len(full) + 1), slot, {r.layer: [hook]})[p.plen:])
        lb = m.logits(m.forward(ids, pos, m.new_cache(r.B, len(full) + 1), slot)[p.plen:])
        t = shift_truth(le, lb, cap)                            # row t: the distribution over response token t + 1
        kl, klr, bd, bdr = (t[k][: n - 1] for k in ("kl", "kl_rev", "bound", "bound_rev"))
        sp = [s for s in p.spikes_rel if s < n]
        want = {"kl_out_mean": float(kl.sum()) / n, "kl_rev_out_mean": float(klr.sum()) / n,
                "kl_out_max": max([0.0] + kl.tolist()),
                "kl_out_spike_mean": float(sum(t["kl"][s] for s in sp)) / len(sp) if sp else 0.0}
        tol = {"kl_out_mean": float(bd.sum()) / n, "kl_rev_out_mean": float(bdr.sum()) / n,
               "kl_out_max": float(bd.max()) if n > 1 else 0.0,
               "kl_out_spike_mean": float(sum(t["bound"][s] for s in sp)) / len(sp) if sp else 0.0}
        for k in KEYS:
            assert abs(rec[k] - want[k]) <= tol[k], (b, c.method, c.budget, k, rec[k], want[k], tol[k])
        moved += want["kl_out_mean"] > 10 * tol["kl_out_mean"]
    assert moved >= len(cells) // 2                             # the comparison is not one of zeros


def test_sweep_zero_cells_and_unchanged_records(sweeps):
    """A cell none of whose latents fire at any spike is its baseline: all four fields exactly 0.  Without the
    switch the records have no such keys and are otherwise what the run with it gives."""
    on, r, pairs, cells, _ = sweeps["on"]
    off = sweeps["off"][0]
    assert set(on) == set(off) and not sweeps["off"][1].output_shift
    for k in on:
        assert set(on[k]) - set(off[k]) == set(KEYS) and not set(off[k]) - set(on[k]), k
        for f in off[k]:
            assert on[k][f] == off[k][f] or (on[k][f] != on[k][f] and off[k][f] != off[k][f]), (k, f)
        assert not any(f.startswith("kl_") for f in off[k])
    sae_cells = [(c, rec) for c, rec in cells if c.kind == "sae"]
    f = r._plan_for([c for c, _ in sae_cells], pairs, {}, with_carry=False)["f"][: len(sae_cells)]
    noop = [(c, rec) for (c, rec), fc in zip(sae_cells, f) if fc >= len(pairs[c.pair].resp)]
    for c, rec in noop:
        assert all(rec[k] == 0.0 for k in KEYS), (c, [rec[k] for k in KEYS])
        assert rec["response_ids"] == pairs[c.pair].resp and abs(rec["delta_nll"]) < 1e-5
    for c, rec in cells:
        assert rec["kl_out_max"] >= rec["kl_out_mean"] >= -1e-6 and rec["kl_out_max"] >= 0.0
        assert all(math.isfinite(rec[k]) for k in KEYS)
    assert "shift_base_rows" not in sweeps["off"][1].stats and r.stats["shift_base_rows"] > 0


def test_sweep_noop_cell_is_exactly_zero():
    """Cells whose latents never fire, made so by hand (pair 0's targeted latents replaced by latents that are
    inactive at every one of its spikes), next to pair 1's cells, which do edit: exact zeros in all four fields,
    while the batch's other cells move."""
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    spec, m, tok, sae = tiny()
    cfg = load_config(None, OVR + SHIFT)
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
        assert all(x[k] == 0.0 for k in KEYS), [x[k] for k in KEYS]
        assert x["response_ids"] == p.resp and abs(x["delta_nll"]) < 1e-5
    assert any(x["kl_out_mean"] > 1e-5 for c, x in zip(cells, res) if c.pair == 1)


def test_unsupported_combinations_raise(tmp_path):
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    with pytest.raises(ValueError, match="tensor-parallel"):
        run_sweep(load_config(None, OVR + SHIFT + ["parallel.tp=2"]), str(tmp_path / "tp"), log=lambda *a: None)
    spec, m, tok, sae = tiny()
    cfg = load_config(None, OVR + SHIFT)
    mk = lambda **kw: SweepRunner(cfg, m, tok, sae, batch=8, device="cpu", layer=1, use_graphs=False, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="layer resume"):
        mk(layer_resume=False)
    with pytest.raises(ValueError, match="layer resume"):
        SweepRunner(load_config(None, OVR + SHIFT + ["runtime.layer_resume=false"]), m, tok, sae, batch=8, device="cpu",
                    layer=1, use_graphs=False)
    m.fused_head = True
    with pytest.raises(ValueError, match="fused-head"):
        mk()
    m.fused_head = False
    for cap in (0.0, 50.0):
        m2 = type("M", (), {"spec": replace(spec, final_softcap=cap), "tp": None, "head_path": False})()
        with pytest.raises(ValueError, match="final softcap"):
            SweepRunner(cfg, m2, tok, sae, batch=8, device="cpu", layer=1, use_graphs=False)
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


def test_run_sweep_files_and_report(tmp_path):
    """``sweep_curves.csv``, the summary's curves, the cell records and fig5 carry the shift only when enabled; with
    the output readout as well the figure gains the specificity plane."""
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.report.figures import make_report

    results = tmp_path / "results"
    head = "method,budget,n,p_secret_mean,p_lo,p_hi,delta_p,delta_nll,leak_rate,ll_accuracy,ll_pass10,ll_majority"
    cols = ("kl_out_mean", "kl_out_spike_mean")
    ovr = [o for o in OVR if not o.startswith("experiment.max_new_tokens")] + ["experiment.max_new_tokens=5"]
    rec = ["intervention.ablation_mode=reconstruct"]
    texts = {}
    for tag, extra in (("on", SHIFT + rec), ("both", SHIFT + ["intervention.output_readout=true"]), ("off", rec)):
        out = str(results / "sweeps" / tag)
        summ = run_sweep(load_config(None, ovr + extra), out, info=DistInfo(), log=lambda *a: None)
        lines = open(os.path.join(out, "sweep_curves.csv")).read().splitlines()
        cells = [json.loads(l) for l in open(os.path.join(out, "sweep_cells.jsonl"))]
        texts[tag] = open(os.path.join(out, "sweep_cells.jsonl")).read()
        if tag == "off":
            assert lines[0] == head and "output_shift" not in summ["config"]
            assert not any(f in c for c in summ["curves"] for f in cols)
            assert not any(k.startswith("kl_") for c in cells for k in c)
            continue
        assert lines[0].endswith("".join(f",{c},{c}_lo,{c}_hi" for c in cols)) and lines[0].startswith(head)
        assert summ["config"]["output_shift"] is True and all(set(KEYS) <= set(c) for c in cells)
        for c in summ["curves"]:
            for f in cols:
                assert c[f]["lo"] <= c[f]["mean"] <= c[f]["hi"], (c["method"], f)
        if tag == "on":                                          # the pure-splice control cell gets the fields too
            assert any(c["method"] == "sae_splice" and c["kl_out_mean"] > 0 for c in cells)
            assert all(len(l.split(",")) == 12 + 6 for l in lines[1:])
    # the run with the switch differs from the run without it by the four keys alone
    strip = lambda t: [{k: v for k, v in json.loads(l).items() if k not in KEYS} for l in t.splitlines()]   # noqa: E731
    assert strip(texts["on"]) == [json.loads(l) for l in texts["off"].splitlines()]
    made = [os.path.basename(p) for p in make_report(str(results), str(tmp_path / "report"))]
    assert sorted(p for p in made if p.startswith("fig5_collateral")) == ["fig5_collateral_both.png",
                                                                         "fig5_collateral_on.png"]
    for t in ("on", "both"):
        assert os.path.getsize(tmp_path / "report" / f"fig5_collateral_{t}.png") > 0
