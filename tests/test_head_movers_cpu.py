"""Output movers off the GPU: the criteria of tests/movers_cases.py cannot pass vacuously, ops/reference.py meets them
and every planted bug is caught by name, the ``planted`` exact-match condition holds with room, ``ops.head_movers``
validates its arguments, the kernel compiles for gfx950 without scratch, and the CPU sweep with
``intervention.output_movers``: every cell's lists and total variation against plain full-sequence forwards of the
edited and the unedited model, consistent record fields, unchanged records without the switch, the combinations that
raise, the files, ``movers_top.csv`` and fig7."""
import os
import re
import subprocess

import pytest
import torch

from movers_cases import (KINDS, KS, MOVERS_CAPS, ROWMAP, ROWS, T_IDS, case_truth, movers_case, movers_mutant,
                          planted_gap, run_movers, tie_columns)
from readout_cases import STREAM_WIDTHS
from taboo_brittleness_amd import ops
from taboo_brittleness_amd.ops import reference as ref

BF = torch.bfloat16
CPU = torch.device("cpu")


@pytest.mark.parametrize("V", STREAM_WIDTHS)
def test_truth_is_a_difference_of_distributions_and_the_bound_can_fail(V):
    """``D`` sums to 0 and ``tv`` lies in [0, 1]; the row selections hold what they must; in the one-entry case the
    raised column's gain is far above its bound, so a result of 0 -- or any value not tied to the inputs -- fails."""
    assert -1 in ROWMAP and max(ROWMAP) >= 2 and 5 in ROWS[5] and -1 in ROWS[3] and len(set(ROWS[5])) < 5
    assert ROWMAP[ROWS[5][3]] == -1 and ROWMAP[ROWS[3][0]] == 2
    for cap in MOVERS_CAPS:
        for kind in KINDS:
            for Rs in (1, 3, 5):
                t = case_truth(V, kind, Rs, 3, cap)
                assert float(t["D"].sum(-1).abs().max()) < 1e-12 and float(t["tv"].max()) <= 1.0 + 1e-12
                assert bool((t["tv"][t["same"]] == 0).all())
                if kind == "identical":
                    assert bool(t["same"][t["ok"]].all())
                if kind == "one_entry" and V > 1:
                    live = t["ok"]
                    assert int(live.sum()) > 0 and not bool(t["same"][live].any())
                    for i in live.nonzero().reshape(-1).tolist():
                        h = int(t["up"][i][0])
                        assert float(t["D"][i, h]) > 1e3 * float(t["eps"][i, h])
                        assert float(t["tv"][i]) > 1e3 * float(t["tv_bound"][i])


@pytest.mark.parametrize("V", STREAM_WIDTHS)
def test_reference_meets_the_criteria(V):
    rep = run_movers(ops.head_movers, CPU, V)
    rep.assert_ok(f"reference head_movers V {V}")
    assert V == 1 or rep.used.get("tracked ids found listed") == 1.0
    run_movers(lambda lg, b, rm, rows, cap, k, ids=None, **kw: ref.head_movers(lg, b, rm, rows, cap, k, ids), CPU, V,
               fill=False, ks=(3,)).assert_ok(f"ref.head_movers V {V}")


@pytest.mark.parametrize("V", STREAM_WIDTHS)
def test_planted_condition_holds_with_room(V):
    """The exact-match rule of the ``planted`` kind is a condition on the inputs: neighbouring truth values among the
    compared entries lie at least 1000 (eps_i + eps_u) apart at every width, ``k``, row selection and cap, and the
    reference reproduces every list."""
    for cap in MOVERS_CAPS:
        for Rs in (1, 3, 5):
            for k in KS:
                room = planted_gap(V, Rs, k, cap)
                print(f"planted V {V} Rs {Rs} k {k} cap {cap:g}: smallest gap {room:.3g} (eps_i + eps_u)")
                assert room >= 1e3, (V, Rs, k, cap, room)
    rep = run_movers(ops.head_movers, CPU, V, kinds=("planted",))
    assert not rep.failures, rep.failures[:3]


@pytest.mark.parametrize("V", STREAM_WIDTHS)
def test_planted_bugs_are_rejected(V):
    """Each stand-in fails, by name, at every width where its bug can show (at ``k = 3``)."""
    assert not run_movers(movers_mutant(), CPU, V, ks=(3,)).failures                      # the stand-in itself is sound
    rep = run_movers(movers_mutant(drop_tail=True), CPU, V, ks=(3,))
    assert rep.failed("one_entry") == (V % 8 != 0 and V > 1), rep.failures[:3]    # V = 1: every difference is 0
    body, tail = tie_columns(V)
    rep = run_movers(movers_mutant(tie_high=True), CPU, V, kinds=("tie",), ks=(3,))
    assert rep.failed("tie ids") == (body is not None or tail is not None), rep.failures[:3]
    if body is not None or tail is not None:
        assert rep.failed("same (p, q) bits")
    rep = run_movers(movers_mutant(no_sums=True), CPU, V, ks=(3,))
    assert rep.failed("tv ", "gain16") and rep.failed("gain1 ") and (V == 1 or rep.failed("up ", "one_entry"))
    assert not rep.failed("identical")
    if V > 1:                                    # one column: every distribution is the same, nothing can show
        rep = run_movers(movers_mutant(ignore_map=True), CPU, V, ks=(3,))
        assert rep.failed("unmapped", "want tv +0.0") and rep.failed("gain1")
        rep = run_movers(movers_mutant(ignore_rows=True), CPU, V, ks=(3,))
        assert rep.failed("no row", "want tv +0.0") and rep.failed("gain16") and rep.failed("Rs 1 ")
        rep = run_movers(movers_mutant(swap_lists=True), CPU, V, ks=(3,))
        assert rep.failed("has not the list's sign") and rep.failed("up ", "one_entry")
    rep = run_movers(movers_mutant(list_zeros=True), CPU, V, ks=(3,))
    assert rep.failed("identical", "empty lists")             # zeros exist only where the rows are equal


def test_op_validates_and_maps():
    V, k = 4104, 3
    z, y, rm, rows, _ = movers_case(V, "gain1", 5, k)
    ids = case_truth(V, "gain1", 5, k, 30.0)["ids"]
    got = ops.head_movers(z, y, rm, rows, 30.0, k, ids)
    want = ref.head_movers(z, y, rm, rows, 30.0, k, ids)
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
    tv, ui, ud, di, dd, dpt = got
    assert [tuple(o.shape) for o in got] == [(5,), (5, k), (5, k), (5, k), (5, k), (5, T_IDS)]
    assert tv.dtype == torch.float32 and ui.dtype == torch.int32 and dpt.dtype == torch.float32
    assert tv[2] == 0 and tv[3] == 0 and tv[0] > 0 and tv[4] > 0
    assert torch.equal(ui[0], ui[4]) and bool((ui[2] == -1).all())
    assert bool((ud[0] > 0).all()) and bool((dd[0] < 0).all())
    outs = {"tv": torch.full((5,), 7.0), "up_id": torch.full((5, k), 7, dtype=torch.int32),
            "up_dp": torch.full((5, k), 7.0), "dn_id": torch.full((5, k), 7, dtype=torch.int32),
            "dn_dp": torch.full((5, k), 7.0), "dp_track": torch.full((5, T_IDS), 7.0)}
    r2 = ops.head_movers(z, y, rm, rows, 30.0, k, ids, **outs)
    assert all(a is outs[n] and torch.equal(a, b) for a, n, b in zip(r2, outs, got))
    none = ops.head_movers(z, y, rm, rows, 30.0, k)                               # no ids: [Rs, 0]
    assert none[5].shape == (5, 0) and torch.equal(none[1], ui)
    e = ops.head_movers(z, y, rm, rows[:0], 30.0, k, ids[:0])
    assert [tuple(o.shape) for o in e] == [(0,), (0, k), (0, k), (0, k), (0, k), (0, T_IDS)]
    nob = ops.head_movers(z, y[:0], rm, rows, 30.0, k)                            # no baseline rows: all unmapped
    assert not nob[0].any() and bool((nob[1] == -1).all()) and bool((nob[3] == -1).all())
    wide = ops.head_movers(z[:, :2].contiguous(), y[:, :2].contiguous(), rm, rows, 30.0, 8)   # k > V: empty slots
    assert bool((wide[1][:, 2:] == -1).all()) and bool((wide[3][:, 2:] == -1).all())
    for bad in (dict(base=y[:, :-1]), dict(base=y.float()), dict(logits=z.float()), dict(logits=z[0]),
                dict(rowmap=rm.long()), dict(rowmap=rm[:4]), dict(rows=rows.long()), dict(rows=rows.view(5, 1)),
                dict(k=0), dict(k=9), dict(ids=ids.long()), dict(ids=ids[:4]),
                dict(ids=torch.zeros(5, 9, dtype=torch.int32)),
                dict(tv=torch.zeros(4)), dict(up_id=torch.zeros(5, k)), dict(dp_track=torch.zeros(5, T_IDS + 1)),
                dict(logits=z[:, :0], base=y[:, :0])):
        with pytest.raises(ValueError):
            ops.head_movers(bad.get("logits", z), bad.get("base", y), bad.get("rowmap", rm), bad.get("rows", rows),
                            30.0, bad.get("k", k), bad.get("ids", ids), tv=bad.get("tv"), up_id=bad.get("up_id"),
                            dp_track=bad.get("dp_track"))


def test_movers_kernel_uses_no_scratch(tmp_path):
    """lens.hip compiled for gfx950 with the extension's flags: the compiler's resource-usage remarks list the movers
    kernel with 0 bytes of scratch and a register count that lets its 512 threads (8 waves on 4 SIMDs) launch."""
    from taboo_brittleness_amd import build as b

    hipcc = os.path.join(b.ROCM, "bin", "hipcc")
    cmd = [hipcc, f"--offload-arch={b.ARCH}", "-c", os.path.join(b.CSRC, "lens.hip"), "-o", str(tmp_path / "lens.o"),
           "--cuda-device-only", "-munsafe-fp-atomics", "-fPIC", "-O3", "-std=c++17", "-I", b.CSRC,
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    mine = [x for x in blocks if "head_movers_kernel" in x.split()[0]]
    assert len(mine) == 1, [x.split()[0] for x in blocks]
    assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0]).group(1)) == 0, mine[0]
    assert int(re.search(r"VGPRs Spill: (\d+)", mine[0]).group(1)) == 0, mine[0]
    assert int(re.search(r"VGPRs: (\d+)", mine[0]).group(1)) <= 128, mine[0]


# ------------------------------------------------------------------------------------------------------ sweep
MOVERS = ["intervention.output_movers=true", "intervention.movers_k=4"]
NEW_KEYS = ("movers_up", "movers_dn", "tv_out_spike_mean", "movers_up_share", "movers_dn_share", "secret_loss_share",
            "secret_in_losers", "decoy_in_gainers", "top_gainer")


@pytest.fixture(scope="module")
def sweeps():
    from test_head_shift_cpu import run_tiny

    on = run_tiny(MOVERS)
    return {"on": on, "off": run_tiny([], model=on[4])}


def test_sweep_fields_match_full_forwards(sweeps):
    """Per cell: a plain forward of prompt + baseline response through the edited model (the cell's plan row) and one
    through the unedited model; at every spike the float64 difference of the two next-token distributions holds the
    record's lists to the list criterion and its total variation to the tv bound."""
    from movers_cases import check_list, movers_truth
    from readout_cases import Report

    _got, r, pairs, cells, (spec, m, _tok, _sae) = sweeps["on"]
    hook = r._hook                                              # plan row b = cell b (one batch)
    cap, k = spec.final_softcap, 4
    assert r.output_movers and r.movers_k == k and r.stats["movers_rows"] > 0
    rep = Report()
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
        sp = [s for s in p.spikes_rel if s < n]
        assert len(rec["movers_up"]) == len(sp) == len(rec["movers_dn"])
        if not sp:
            continue
        t = movers_truth(le[sp], lb[sp], cap)
        want = float(t["tv"].sum()) / len(sp)
        tol = float(t["tv_bound"].sum()) / len(sp)
        assert abs(rec["tv_out_spike_mean"] - want) <= tol, (b, c.method, c.budget, rec["tv_out_spike_mean"], want, tol)
        moved += want > 100 * tol
        pb, qb = lb[sp].view(torch.int16).int(), le[sp].view(torch.int16).int()
        for j in range(len(sp)):
            for name, sign in (("movers_up", 1.0), ("movers_dn", -1.0)):
                lst = rec[name][j]
                li = torch.full((k,), -1, dtype=torch.int32)
                lv = torch.zeros(k)
                li[: len(lst)] = torch.tensor([x[0] for x in lst], dtype=torch.int32)
                lv[: len(lst)] = torch.tensor([x[1] for x in lst])
                check_list(rep, f"{name} cell {b} {c.method} {c.budget} spike {sp[j]}", li, lv, t["D"][j], t["eps"][j],
                           sign, pb[j], qb[j])
    assert not rep.failures, rep.failures[:5]
    assert moved >= len(cells) // 2                             # the comparison is not one of zeros


def test_sweep_records_are_consistent_and_switch_off_is_unchanged(sweeps):
    """Shares lie in [0, 1 + rounding]; the total variation is at least either list's sum, minus the bound;
    ``secret_in_losers`` / ``decoy_in_gainers`` / ``top_gainer`` agree with the lists; a cell none of whose latents
    fire is exactly zero with empty lists and NaN shares; without the switch the records lack exactly the new keys."""
    import math

    from shift_cases import depth

    on, r, pairs, cells, (spec, _m, _tok, _sae) = sweeps["on"]
    off = sweeps["off"][0]
    assert set(on) == set(off) and not sweeps["off"][1].output_movers
    assert "movers_rows" not in sweeps["off"][1].stats and all(p.x_base is None for p in sweeps["off"][2])
    for key in on:
        assert set(on[key]) - set(off[key]) == set(NEW_KEYS) and not set(off[key]) - set(on[key]), key
        for f in off[key]:
            assert on[key][f] == off[key][f] or (on[key][f] != on[key][f] and off[key][f] != off[key][f]), (key, f)
    # a value is within delta (P + Q) of the truth; a list's sum and tv each err by at most delta * 2
    bound = 4 * 2.0 ** -22 * (spec.final_softcap + depth(spec.vocab_size) + 4)
    live = 0
    for c, rec in cells:
        p = pairs[c.pair]
        sp = [s for s in p.spikes_rel if s < len(p.resp)]
        secret, decoys = set(p.track[:2]), set(p.track[2: 2 + p.n_decoys])
        tvs = []
        gains = {}
        for up, dn in zip(rec["movers_up"], rec["movers_dn"]):
            assert len(up) <= 4 and len(dn) <= 4
            assert all(v > 0 for _, v in up) and all(v < 0 for _, v in dn)
            assert [v for _, v in up] == sorted((v for _, v in up), reverse=True)
            assert [v for _, v in dn] == sorted(v for _, v in dn)
            for i, v in up:
                gains[i] = gains.get(i, 0.0) + v
        n_sp = len(sp)
        if n_sp:
            assert rec["secret_in_losers"] == sum(any(i in secret for i, _ in dn) for dn in rec["movers_dn"]) / n_sp
            assert rec["decoy_in_gainers"] == sum(any(i in decoys for i, _ in up) for up in rec["movers_up"]) / n_sp
        assert (rec["top_gainer"] == -1) == (not gains)
        if gains:
            best = max(gains.values())
            assert gains[rec["top_gainer"]] >= best - 1e-6
        assert 0.0 <= rec["tv_out_spike_mean"] <= 1.0 + bound
        any_list = any(rec["movers_up"]) or any(rec["movers_dn"])
        for key in ("movers_up_share", "movers_dn_share", "secret_loss_share"):
            if math.isnan(rec[key]):
                assert not any_list and rec["tv_out_spike_mean"] == 0.0
            else:
                assert -0.0 <= rec[key] <= 1.0 + 1e-4, (key, rec[key])
                live += 1
        # tv >= both list sums minus the bound: summed over the cell's spikes
        if n_sp:
            tot = rec["tv_out_spike_mean"] * n_sp
            assert tot >= sum(v for up in rec["movers_up"] for _, v in up) - n_sp * bound
            assert tot >= -sum(v for dn in rec["movers_dn"] for _, v in dn) - n_sp * bound
    assert live > 0
    sae_cells = [(c, rec) for c, rec in cells if c.kind == "sae"]
    f = r._plan_for([c for c, _ in sae_cells], pairs, {}, with_carry=False)["f"][: len(sae_cells)]
    for (c, rec), fc in zip(sae_cells, f):
        if fc >= len(pairs[c.pair].resp):                        # none of its latents fires at any spike
            assert rec["tv_out_spike_mean"] == 0.0 and not any(rec["movers_up"]) and not any(rec["movers_dn"])
            assert math.isnan(rec["movers_up_share"]) and rec["top_gainer"] == -1


def test_unsupported_combinations_raise(tmp_path):
    from dataclasses import replace

    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from test_head_shift_cpu import OVR, tiny

    with pytest.raises(ValueError, match="tensor-parallel"):
        run_sweep(load_config(None, OVR + MOVERS + ["parallel.tp=2"]), str(tmp_path / "tp"), log=lambda *a: None)
    spec, m, tok, sae = tiny()
    cfg = load_config(None, OVR + MOVERS)
    def mk(**kw):
        return SweepRunner(cfg, m, tok, sae, batch=8, device="cpu", layer=1, use_graphs=False, **kw)

    with pytest.raises(ValueError, match="layer resume"):
        mk(layer_resume=False)
    for k in (0, 9):
        with pytest.raises(ValueError, match="movers_k"):
            SweepRunner(load_config(None, OVR + ["intervention.output_movers=true", f"intervention.movers_k={k}"]), m,
                        tok, sae, batch=8, device="cpu", layer=1, use_graphs=False)
    m.fused_head = True
    try:
        with pytest.raises(ValueError, match="fused-head"):
            mk()
    finally:
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
    """``sweep_curves.csv``, the summary, ``movers_top.csv`` and fig7 carry the movers only when enabled; the run with
    the switch (and the output shift beside it) differs from the run without by the new keys alone."""
    import csv
    import json

    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.report.figures import make_report
    from test_head_shift_cpu import KEYS, OVR

    results = tmp_path / "results"
    head = "method,budget,n,p_secret_mean,p_lo,p_hi,delta_p,delta_nll,leak_rate,ll_accuracy,ll_pass10,ll_majority"
    cols = ("tv_out_spike_mean", "movers_up_share", "secret_loss_share")
    ovr = [o for o in OVR if not o.startswith("experiment.max_new_tokens")] + ["experiment.max_new_tokens=5"]
    texts = {}
    for tag, extra in (("on", MOVERS), ("both", MOVERS + ["intervention.output_shift=true"]), ("off", [])):
        out = str(results / "sweeps" / tag)
        summ = run_sweep(load_config(None, ovr + extra), out, info=DistInfo(), log=lambda *a: None)
        lines = open(os.path.join(out, "sweep_curves.csv")).read().splitlines()
        cells = [json.loads(l) for l in open(os.path.join(out, "sweep_cells.jsonl"))]
        texts[tag] = open(os.path.join(out, "sweep_cells.jsonl")).read()
        if tag == "off":
            assert lines[0] == head and "output_movers" not in summ["config"] and "movers_k" not in summ["config"]
            assert not any(f in c for c in summ["curves"] for f in cols + ("secret_in_losers",))
            assert not any(k in c for c in cells for k in NEW_KEYS)
            assert not os.path.exists(os.path.join(out, "movers_top.csv"))
            continue
        assert lines[0].endswith("".join(f",{c},{c}_lo,{c}_hi" for c in cols)) and lines[0].startswith(head)
        assert summ["config"]["output_movers"] is True and summ["config"]["movers_k"] == 4
        assert all(set(NEW_KEYS) <= set(c) for c in cells)
        assert all(("kl_out_mean" in c) == (tag == "both") for c in cells)
        for c in summ["curves"]:
            assert 0.0 <= c["secret_in_losers"] <= 1.0 and 0.0 <= c["decoy_in_gainers"] <= 1.0
            for f in cols:
                assert c[f]["mean"] != c[f]["mean"] or c[f]["lo"] <= c[f]["mean"] <= c[f]["hi"], (c["method"], f)
        rows = list(csv.reader(open(os.path.join(out, "movers_top.csv"), newline="")))
        assert rows[0] == ["method", "budget", "rank", "token_id", "token", "count"] and len(rows) > 1
        per = {}
        for meth, bud, rank, tid, _tok, n in rows[1:]:
            per.setdefault((meth, int(bud)), []).append((int(rank), int(tid), int(n)))
        want = {}
        for c in cells:
            if c["top_gainer"] >= 0:
                want.setdefault((c["method"], c["budget"]), []).append(c["top_gainer"])
        assert set(per) == set(want)
        for key, ent in per.items():
            assert [e[0] for e in ent] == list(range(len(ent))) and len(ent) <= 10
            assert [e[2] for e in ent] == sorted((e[2] for e in ent), reverse=True)
            assert all(want[key].count(tid) == n for _, tid, n in ent)
    def strip(t, ks):
        return [{k: v for k, v in json.loads(l).items() if k not in ks} for l in t.splitlines()]

    def same(a, b):
        return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)

    assert same(strip(texts["on"], NEW_KEYS), [json.loads(l) for l in texts["off"].splitlines()])
    assert same(strip(texts["both"], NEW_KEYS + tuple(KEYS)), [json.loads(l) for l in texts["off"].splitlines()])
    assert same(strip(texts["both"], KEYS), strip(texts["on"], ()))     # the shift beside it changes no movers field
    made = [os.path.basename(p) for p in make_report(str(results), str(tmp_path / "report"))]
    assert sorted(p for p in made if p.startswith("fig7_movers")) == ["fig7_movers_both.png", "fig7_movers_on.png"]
    for t in ("on", "both"):
        assert os.path.getsize(tmp_path / "report" / f"fig7_movers_{t}.png") > 0
