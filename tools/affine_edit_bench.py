"""What latent clamping / steering costs, on the GPU:

* ``ops.latent_affine_edit`` against ``ops.lowrank_edit`` (the error-preserving edit) on the same rows at the 9B
  shapes (D = 3584, d_sae = 16384, fp32 SAE tables): m = 1 / 8 / 32 selected latents on 64 / 512 / 2048 decode rows,
  every row flagged.  The two kernels alternate window by window in one process, so clock and cache state drift hits
  both alike; the ratio is the median over the window pairs.  Twice: with ``val = 0``, where both do the same work
  (the same coefficients, the same skipped terms: the cost of the extra input alone), and with ``val = 4``, where the
  clamp also adds the decoder rows of the latents that do not fire -- terms the ablation skips.
* one sweep step in clamp mode against the error-preserving one at equal cells (a random ``gemma2-mini`` and a 2048-
  latent SAE: the reuse levels and the row counts are what differ between the modes, not the model): seconds per
  ``run_cells`` call, alternating, and ``tf_rows`` per cell -- clamp mode loses the no-op spike skip.

Report only (no threshold):

    python tools/affine_edit_bench.py [--out FILE.json] [--no-sweep]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from taboo_brittleness_amd import ops  # noqa: E402
from taboo_brittleness_amd.interp.sae import JumpReLUSAE  # noqa: E402

BF = torch.bfloat16


def window(fn, inner: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def interleaved(fa, fb, warm: int = 3, reps: int = 12, inner: int = 5) -> dict:
    """Milliseconds per call of ``fa`` and ``fb`` over ``reps`` alternating windows of ``inner`` calls (device
    events), and ``fa / fb`` per window pair."""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window(fa, inner))
        tb.append(window(fb, inner))
    ratio = [x / y for x, y in zip(ta, tb)]
    st = lambda v: {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}  # noqa: E731
    return {"affine": st(ta), "lowrank": st(tb),
            "ratio": {"median": round(statistics.median(ratio), 4), "min": round(min(ratio), 4),
                      "max": round(max(ratio), 4)}}


def kernels(dev, rows_list, ms_list) -> list:
    D, L = 3584, 16384
    g = torch.Generator().manual_seed(0)
    sae = JumpReLUSAE.random(D, L, seed=1, device=dev)                 # fp32 tables
    wn = (torch.randn(D, generator=g) * 0.1).to(BF).to(dev)
    out = []
    for M in rows_list:
        h0 = torch.randn(M, D, generator=g).to(BF).to(dev)
        # half of the selected latents fire on their row (the targeted latents of a sweep), half are drawn at random
        acts = sae.encode(h0)
        fired = torch.topk(acts, 16, dim=1).indices.to(torch.int32).cpu()
        for m in ms_list:
            idx = torch.randint(0, L, (M, m), generator=g, dtype=torch.int32)
            idx[:, : m // 2] = fired[:, : m // 2]
            idx = idx.to(dev)
            cnt = torch.full((M,), m, dtype=torch.int32, device=dev)
            vals = {v: torch.full((M, m), v, device=dev) for v in (0.0, 4.0)}
            apply = torch.ones(M, dtype=torch.uint8, device=dev)
            x = torch.zeros(M, D, dtype=BF, device=dev)
            coef = torch.zeros(M, m, device=dev)
            h = h0.clone()

            def affine(val):
                h.copy_(h0)                                             # the edits are in place: same input every call
                ops.latent_affine_edit(h, apply, idx, cnt, val, sae.W_encT, sae.W_dec, sae.b_enc, sae.threshold, None,
                                       1.0, wn, 1e-6, x, coef)

            def lowrank():
                h.copy_(h0)
                ops.lowrank_edit(h, apply, idx, cnt, sae.W_encT, sae.W_dec, sae.b_enc, sae.threshold, None, 1.0, wn,
                                 1e-6, x, coef)

            ent = {"rows": M, "m": m, "val0": interleaved(lambda: affine(vals[0.0]), lowrank),
                   "val4": interleaved(lambda: affine(vals[4.0]), lowrank)}
            lowrank()
            ent["firing_selected_latents_pct"] = round(100 * float((coef != 0).float().mean()), 1)
            out.append(ent)
            print(json.dumps(ent), flush=True)
    return out


def sweep(dev, reps: int, spec=None, nwords: int = 2, extra=()) -> dict:
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.models.gemma2 import Gemma2Model
    from taboo_brittleness_amd.models.spec import GEMMA2_MINI
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.models.weights import random_gemma2
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    spec = spec or GEMMA2_MINI
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    model = Gemma2Model(random_gemma2(spec, dtype=BF, seed=5, norm_std=0.1, device=dev, post_norm_gain=8.0), dev)
    tok = SyntheticTokenizer(vocab_size=spec.vocab_size)
    layer = min(5, spec.layers - 2)
    base = ["experiment.max_new_tokens=24", f"model.layer_idx={layer}"] + list(extra)
    runs = {}
    for name, mode_set in (("error_preserving", []),
                           ("clamp", ["intervention.ablation_mode=clamp", "intervention.clamp_value=4.0"])):
        cfg = load_config(None, base + mode_set)
        sae = JumpReLUSAE.random(spec.hidden, 2048, seed=2, device=dev)
        words = list(cfg.words)[:nwords]
        npairs = len(words) * len(cfg.prompts)
        ncell = npairs * len(cfg.intervention.budgets) * (1 + cfg.intervention.random_trials)
        r = SweepRunner(cfg, model, tok, sae, batch=ncell + 8, device=dev, layer=layer, kv_pairs=npairs + 1,
                        use_graphs=dev.type == "cuda")
        pairs = r.build_pairs(words, cfg.prompts)
        r.run_baselines(pairs)
        cells = r.make_cells(pairs, ("sae_targeted", "sae_random"))
        runs[name] = (r, pairs, cells)
    res = {"model": spec.name, "d_sae": 2048, "max_new_tokens": 24, "cells": len(runs["clamp"][2]), "modes": {}}
    assert len(runs["clamp"][2]) == len(runs["error_preserving"][2])
    times = {k: [] for k in runs}
    for i in range(reps + 1):                                           # the first round warms up (graph captures)
        for name, (r, pairs, cells) in runs.items():
            before = dict(r.stats)
            sync()
            t0 = time.perf_counter()
            r.run_cells(pairs, cells)
            sync()
            if i:
                times[name].append(time.perf_counter() - t0)
            d = {k: r.stats[k] - before[k] for k in ("cells", "diverged", "tf_rows", "decode_rows_run", "lens_rows")}
            res["modes"][name] = {"per_call": d, "tf_rows_per_cell": round(d["tf_rows"] / max(1, d["cells"]), 3)}
    for name, v in times.items():
        res["modes"][name]["seconds"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                                         "max": round(max(v), 4)}
    res["clamp_over_error_preserving"] = round(res["modes"]["clamp"]["seconds"]["median"] /
                                               res["modes"]["error_preserving"]["seconds"]["median"], 4)
    print(json.dumps(res), flush=True)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="64,512,2048")
    ap.add_argument("--m", default="1,8,32")
    ap.add_argument("--no-sweep", action="store_true", help="kernels only")
    ap.add_argument("--sweep-reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("affine_edit_bench needs the GPU (a CPU time says nothing about this path)")
    from taboo_brittleness_amd.runtime import gemm_dispatch as GD

    GD.set_mode("tb")
    dev = torch.device("cuda:0")
    res = {"shapes": {"D": 3584, "d_sae": 16384, "tables": "fp32", "alpha": 1.0, "val": 4.0},
           "kernels": kernels(dev, [int(r) for r in args.rows.split(",")], [int(m) for m in args.m.split(",")])}
    if not args.no_sweep:
        res["sweep"] = sweep(dev, args.sweep_reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
