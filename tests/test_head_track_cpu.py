"""Output-side readout off the GPU: ``ref.head_track`` against a plain fp64 computation, the CPU sweep's reuse levels
with ``intervention.output_readout``, the record / summary / CSV keys it adds, the forcing fields, the combinations
that raise, and the tracking kernel's compiled resource usage."""
import json
import os
import re
import subprocess

import pytest
import torch

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.ops import reference as ref

BF = torch.bfloat16
CAP = 30.0
NEW_KEYS = ("logp_out_mean", "logp_out_max", "logp_out_final", "logp_out_spike_mean", "rank_out_min",
            "rank_out_median", "delta_logp_out", "logp_out_mean_base", "decoy_logp_out")
DONOR_KEYS = ("logp_out_donor_mean", "rank_out_donor_min", "delta_logp_out_donor")


def planted_case(R, V, seed=13):
    """bf16 logits ``[R, V]`` and tracked ids ``[R, 8]``.  Columns: 0 the row's argmax (rank 0), 1 / 2 free (planted
    in rows 0-2), 3-5 the ids ``0``, ``V - 1``, ``-1``, 6-7 one id twice.  Row 0: logits 80 and 200 (bf16 softcap at
    cap 30: 29.75 and the saturated 30), the 200 tracked in column 1 (rank 0), the 80 in column 2 (rank 1).  Row 1:
    150 and 200, both saturated, the later one tracked (rank 0: the tie does not count).  Row 2: one value at columns
    16, 17 (one 8-logit chunk) and 33 (another chunk), 17 tracked."""
    g = torch.Generator().manual_seed(seed)
    lg = (torch.randn(R, V, generator=g) * 4).to(BF)
    track = torch.randint(0, V, (R, 8), generator=g, dtype=torch.int32)
    lg[0, 10], lg[0, 4000] = 80.0, 200.0
    far = min(20000, V - 2)
    lg[1, 7], lg[1, far] = 150.0, 200.0
    lg[2, 16] = lg[2, 17] = lg[2, 33] = 9.5
    track[0, 1], track[0, 2], track[1, 1], track[2, 1] = 4000, 10, far, 17
    track[:, 0] = ref.argmax_rows(lg, CAP).view(-1)
    track[:, 3], track[:, 4], track[:, 5] = 0, V - 1, -1
    track[:, 7] = track[:, 6]
    return lg, track


@pytest.mark.parametrize("n_rank", [0, 2, 8])
def test_reference_matches_fp64(n_rank):
    """log_softmax of the capped values in fp64 and a sort-based rank (position of the first equal value in the
    descending order = the number of strictly greater entries)."""
    R, V = 6, 4099 * 8 + 5
    lg, track = planted_case(R, V)
    logp, rank = ref.head_track(lg, CAP, track, n_rank)
    z = ref.softcap_bf16(lg.float(), CAP).double()
    lsm = torch.log_softmax(z, -1)
    srt = torch.sort(z, -1, descending=True).values
    for r in range(R):
        for k in range(8):
            i = int(track[r, k])
            if i < 0:
                assert float(logp[r, k]) == 0.0 and int(rank[r, k]) == -1
                continue
            assert abs(float(logp[r, k]) - float(lsm[r, i])) <= 1e-4 + 1e-5 * abs(float(lsm[r, i]))
            want = int(torch.searchsorted(-srt[r], -z[r, i], right=False)) if k < n_rank else -1
            assert int(rank[r, k]) == want, (r, k)
    if n_rank >= 2:
        assert rank[:, 0].tolist() == [0] * R and int(rank[0, 1]) == 0 and int(rank[1, 1]) == 0
        assert float(z[1, 7]) == float(z[1, 20000]) == 30.0
    if n_rank == 8:
        assert int(rank[0, 2]) == 1                                   # the 80 sits under the 200 only
        assert float(z[2, 16]) == float(z[2, 17]) == float(z[2, 33])
        assert int(rank[2, 1]) == int((z[2] > z[2, 17]).sum()) > 0
        assert torch.equal(rank[:, 6], rank[:, 7])


def test_op_cpu_path_and_col_form():
    lg, track = planted_case(6, 4099 * 8 + 5)
    tgt = torch.tensor([5, -1, 11, 7, 0, 77], dtype=torch.int32)
    nxt, ns, nt, logp, rank = ops.decode_head_track(lg, CAP, track, 2, tgt)
    n0, s0, t0 = ops.decode_head(lg, CAP, tgt)
    assert torch.equal(nxt, n0) and torch.equal(ns, s0) and torch.equal(nt, t0)
    lp, rk = ref.head_track(lg, CAP, track, 2)
    assert torch.equal(logp, lp) and torch.equal(rank, rk)
    lw, rw = torch.full((6, 4, 8), 7.5), torch.full((6, 4, 8), -7, dtype=torch.int32)
    col = torch.tensor([0, 3, 2, 9, 1, 1])
    ops.decode_head_track(lg, CAP, track, 2, logp=lw, rank=rw, col=col)
    for r in range(6):
        c = min(int(col[r]), 3)
        assert torch.equal(lw[r, c], lp[r]) and torch.equal(rw[r, c], rk[r])
        assert int((lw[r] == 7.5).sum()) == 3 * 8
    for bad in (dict(track=track[:, :0]), dict(track=torch.zeros(6, 9, dtype=torch.int32)), dict(n_rank=9)):
        with pytest.raises(ValueError):
            ops.decode_head_track(lg, CAP, bad.get("track", track), bad.get("n_rank", 2))


def test_tracking_kernel_uses_no_scratch(tmp_path):
    """lens.hip compiled for gfx950 with the extension's flags: the compiler's resource-usage remarks list every
    instantiation of the tracking kernel with 0 bytes of scratch (and the __launch_bounds__(512) they keep)."""
    from taboo_brittleness_amd import build as b

    hipcc = os.path.join(b.ROCM, "bin", "hipcc")
    cmd = [hipcc, f"--offload-arch={b.ARCH}", "-c", os.path.join(b.CSRC, "lens.hip"), "-o", str(tmp_path / "lens.o"),
           "--cuda-device-only", "-munsafe-fp-atomics", "-fPIC", "-O3", "-std=c++17", "-I", b.CSRC,
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    track = [x for x in blocks if "decode_head_track_kernel" in x.split()[0]]
    assert len(track) == 4, [x.split()[0] for x in blocks]
    for x in track:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", x).group(1)) == 0, x
        assert int(re.search(r"VGPRs: (\d+)", x).group(1)) <= 128, x          # 512 threads: 8 waves on 4 SIMDs


# ------------------------------------------------------------------------------------------------------ sweep
READOUT = ["intervention.output_readout=true"]


def _records(extra, methods, **kw):
    from test_interchange_cpu import _runner

    cfg, r = _runner(extra, **kw)
    pairs = r.build_pairs(cfg.words, cfg.prompts, methods)
    r.run_baselines(pairs)
    cells = r.make_cells(pairs, methods)
    out = []
    for c0 in range(0, len(cells), 50):                        # several batches
        out += r.run_cells(pairs, cells[c0:c0 + 50], measure_nll=True)
    key = lambda x: (x["word"], x["prompt_idx"], x["method"], x["budget"], x["trial"])   # noqa: E731
    return {key(x): x for x in out}, r, pairs


@pytest.fixture(scope="module")
def sweeps():
    from test_interchange_cpu import DEFAULT, SWAP

    on, off = dict(prefix_share=True, layer_resume=True), dict(prefix_share=False, layer_resume=False)
    return {"reuse": _records(READOUT, DEFAULT + SWAP, **on), "scratch": _records(READOUT, DEFAULT + SWAP, **off),
            "share": _records(READOUT, DEFAULT + SWAP, prefix_share=True, layer_resume=False),
            "off": _records([], DEFAULT + SWAP, **on)}


def _same(u, v):
    if isinstance(u, list):
        return len(u) == len(v) and all(_same(a, b) for a, b in zip(u, v))
    if isinstance(u, float):
        return (u != u and v != v) or abs(u - v) <= 1e-6 + 1e-5 * abs(u)
    return u == v


def test_sweep_reuse_equals_from_scratch(sweeps):
    """Every reuse level on, and prefix sharing alone, against ``prefix_share = layer_resume = False``: the integer
    fields equal, the float fields to the tolerance of tests/test_interchange_cpu.py's reuse test."""
    from test_interchange_cpu import SWAP

    a = sweeps["scratch"][0]
    assert sweeps["reuse"][1].stats["tf_rows"] > 0 and sweeps["reuse"][1].stats["diverged"] > 0
    for name in ("reuse", "share"):
        b = sweeps[name][0]
        assert set(a) == set(b)
        for k in a:
            assert set(a[k]) == set(b[k]), k
            assert a[k]["response_ids"] == b[k]["response_ids"], k
            for f in NEW_KEYS + (DONOR_KEYS if k[2] in SWAP else ()):
                assert _same(a[k][f], b[k][f]), (name, k, f, a[k][f], b[k][f])
    assert any(r["delta_logp_out"] != 0.0 for r in a.values())


def test_record_fields(sweeps):
    """The new keys appear only with the switch, the donor fields on swap cells only; the fields are consistent with
    each other and with the pair's baseline table."""
    from test_interchange_cpu import SWAP

    got, runner, pairs = sweeps["reuse"]
    off = sweeps["off"][0]
    base = {(p.word, p.pidx): p for p in pairs}
    assert all(p.out_logp is None and p.out_rank is None for p in sweeps["off"][2]) and sweeps["off"][1].gen.track_cols == 0
    for k, r in got.items():
        assert set(r) - set(off[k]) == set(NEW_KEYS) | (set(DONOR_KEYS) if k[2] in SWAP else set()), k
        assert not set(off[k]) - set(r)
        assert all(r[f] == off[k][f] for f in ("response_ids", "topk_ids", "p_secret_mean", "nll_edit")), k
        p = base[k[0], k[1]]
        assert p.out_logp.shape == (len(p.gen_toks), len(p.track)) == p.out_rank.shape
        ranked = [0, 1] + sorted(p.extra.values())               # the secret forms and the other words' secrets
        assert (p.out_rank[:, ranked] >= 0).all() and (p.out_logp < 0).all()
        assert (p.out_rank[:, [j for j in range(len(p.track)) if j not in ranked]] == -1).all()
        want = runner._out_fields(p, p.out_logp[: len(p.resp)], p.out_rank[: len(p.resp)])
        assert r["logp_out_mean_base"] == want["logp_out_mean"]
        assert r["delta_logp_out"] == r["logp_out_mean"] - r["logp_out_mean_base"]
        assert r["logp_out_max"] >= r["logp_out_mean"] and r["logp_out_max"] >= r["logp_out_final"]
        assert 0 <= r["rank_out_min"] <= r["rank_out_median"] and len(r["decoy_logp_out"]) == p.n_decoys == 3
        if k[2] in SWAP:
            assert r["rank_out_donor_min"] >= 0 and r["logp_out_donor_mean"] < 0
    # a run with swap methods also ranks the other words' secrets: they lie after the decoys in Pair.track and are
    # moved in front of them in the head's id table
    assert pairs[0].ro_order() == [0, 1, 5, 2, 3, 4] and runner._n_track == len(pairs[0].track) == 6
    assert runner._n_rank == 3 == runner.gen.track_rank


def test_generator_is_rebuilt_when_the_ranked_columns_grow():
    """``build_pairs`` without and then with swap methods: the ranked block grows and the generator follows."""
    from test_interchange_cpu import DEFAULT, SWAP, _runner

    cfg, r = _runner(READOUT)
    pairs = r.build_pairs(cfg.words, cfg.prompts, DEFAULT)
    r.run_baselines(pairs[:1])
    g0 = r.gen
    assert (r._n_rank, g0.track_rank, g0.track_cols) == (2, 2, 5)
    pairs = r.build_pairs(cfg.words, cfg.prompts, DEFAULT + SWAP)
    r.run_baselines(pairs[:1])
    assert r.gen is not g0 and (r.gen.track_rank, r.gen.track_cols) == (3, 6)
    assert (pairs[0].out_rank[:, 5] >= 0).all()


def test_run_sweep_files_report_and_forcing(tmp_path):
    """``sweep_curves.csv``, the summary's curves, fig3b and the forcing records carry the readout only when enabled."""
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.pipelines.token_forcing import _FORCING_STATE, run_forcing, run_forcing_settings
    from taboo_brittleness_amd.report.figures import make_report
    from test_splice_cpu import OVR, _tiny

    results = tmp_path / "results"
    head = "method,budget,n,p_secret_mean,p_lo,p_hi,delta_p,delta_nll,leak_rate,ll_accuracy,ll_pass10,ll_majority"
    cols = ("delta_logp_out", "logp_out_spike_mean", "rank_out_min")
    for tag, extra in (("on", READOUT), ("off", [])):
        out = str(results / "sweeps" / tag)
        summ = run_sweep(load_config(None, OVR + extra), out, info=DistInfo(), log=lambda *a: None)
        lines = open(os.path.join(out, "sweep_curves.csv")).read().splitlines()
        cells = [json.loads(l) for l in open(os.path.join(out, "sweep_cells.jsonl"))]
        if tag == "on":
            assert lines[0] == head + "".join(f",{c},{c}_lo,{c}_hi" for c in cols)
            assert all(len(l.split(",")) == 12 + 9 for l in lines[1:]) and summ["config"]["output_readout"] is True
            for c in summ["curves"]:
                for f in cols:
                    assert c[f]["lo"] <= c[f]["mean"] <= c[f]["hi"], (c["method"], f)
            assert all(set(NEW_KEYS) <= set(c) for c in cells)
        else:
            assert lines[0] == head and "output_readout" not in summ["config"]
            assert not any(f in c for c in summ["curves"] for f in cols)
            assert not any(k.startswith(("logp_out", "rank_out", "delta_logp", "decoy_logp")) for c in cells for k in c)
    made = [os.path.basename(p) for p in make_report(str(results), str(tmp_path / "report"))]
    assert [p for p in made if p.startswith("fig3b_content_vs_output")] == ["fig3b_content_vs_output_on.png"]
    assert os.path.getsize(tmp_path / "report" / "fig3b_content_vs_output_on.png") > 0
    # forcing: the first answer token's readout of the secret, per (word, phrase) row and per setting
    spec, m, tok, sae = _tiny()
    settings = [{"word": "ship", "kind": "none"}, {"word": "ship", "kind": "sae", "latents": [3, 7]}]
    rows = {}
    for tag, extra in (("on", READOUT), ("off", [])):
        cfg = load_config(None, OVR + extra + ["token_forcing.max_new_tokens=3", "token_forcing.warmup_max_new_tokens=3"])
        res = run_forcing_settings(cfg, m, tok, settings, "postgame", sae, 2)
        one = run_forcing(cfg, m, tok, ["ship"], "pregame", sae, 2, {"kind": "sae", "latents": [3, 7]})
        rows[tag] = one["rows"]
        for r in res + one["rows"]:
            assert ("logp_secret_first" in r) == ("rank_secret_first" in r) == (tag == "on")
            if tag == "on":
                assert r["logp_secret_first"] < 0 and r["rank_secret_first"] >= 0
    _FORCING_STATE.clear()
    assert [r["completion"] for r in rows["on"]] == [r["completion"] for r in rows["off"]]
    assert len({r["logp_secret_first"] for r in rows["on"]}) > 1


def test_unsupported_combinations_raise(tmp_path):
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from test_interchange_cpu import DEFAULT, _runner
    from test_splice_cpu import OVR, _tiny

    with pytest.raises(ValueError, match="tensor-parallel"):
        run_sweep(load_config(None, OVR + READOUT + ["parallel.tp=2"]), str(tmp_path / "tp"), log=lambda *a: None)
    spec, m, tok, sae = _tiny()
    cfg = load_config(None, OVR + READOUT)
    m.fused_head = True
    with pytest.raises(ValueError, match="fused-head"):
        SweepRunner(cfg, m, tok, sae, batch=8, device="cpu", layer=2, use_graphs=False)
    m.fused_head = False
    cfg, r = _runner(READOUT)
    pairs = r.build_pairs(cfg.words, cfg.prompts, DEFAULT)
    r.run_baselines(pairs)
    r.carry_rows = 4
    with pytest.raises(ValueError, match="carry-over"):
        r.run_cells(pairs, r.make_cells(pairs, DEFAULT)[:4])
    cfg9 = load_config(None, OVR + READOUT + ["intervention.decoys={ship: [a, b, c, d, e, f, g]}"])
    with pytest.raises(ValueError, match="at most 8"):
        SweepRunner(cfg9, m, tok, sae, batch=8, device="cpu", layer=2, use_graphs=False).build_pairs(["ship"], cfg9.prompts)
