"""What reconstruct-mode ablation costs at the 9B shapes (D = 3584, d_sae = 16384, fp32 SAE tables), on the GPU:

* the reconstruct hook's work on a decode bucket of 64 / 512 / 2048 rows -- full-bucket ``sae.encode`` +
  ``ops.sae_splice_edit`` -- beside ``ops.lowrank_edit`` (the error-preserving edit) on the same rows and beside one
  unhooked decode step (all blocks + vocab head) of a random Gemma-2-9B at that row count;
* the teacher-forced tail's splice: ~30k flagged rows reading a 480-row activation table through ``src_row``.

Device-event times, medians over repeated windows after a warm-up.  Report only (no threshold):

    python tools/splice_bench.py [--out FILE.json] [--no-model]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from taboo_brittleness_amd import ops  # noqa: E402
from taboo_brittleness_amd.interp.sae import JumpReLUSAE  # noqa: E402

BF = torch.bfloat16


def timed(fn, warm: int = 3, reps: int = 10, inner: int = 5) -> dict:
    """Median / min / max milliseconds per call of ``fn`` over ``reps`` windows of ``inner`` calls (device events)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-model", action="store_true", help="skip the 9B decode step (kernels only)")
    ap.add_argument("--rows", default="64,512,2048")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("splice_bench needs the GPU (a CPU time says nothing about this path)")
    from taboo_brittleness_amd.runtime import gemm_dispatch as GD

    GD.set_mode("tb")
    dev = torch.device("cuda:0")
    D, L, mmax, K = 3584, 16384, 32, 4
    g = torch.Generator().manual_seed(0)
    sae = JumpReLUSAE.random(D, L, seed=1, device=dev)                 # fp32 tables, L0 ~ 76 on unit-variance rows
    wn = (torch.randn(D, generator=g) * 0.1).to(BF).to(dev)
    res = {"shapes": {"D": D, "d_sae": L, "mmax": mmax, "tables": "fp32"}, "decode": [], "tail": None}
    rows_list = [int(r) for r in args.rows.split(",")]

    model = cache = None
    if not args.no_model:
        from taboo_brittleness_amd.models.gemma2 import Gemma2Model
        from taboo_brittleness_amd.models.spec import GEMMA2_9B
        from taboo_brittleness_amd.models.weights import random_gemma2

        model = Gemma2Model(random_gemma2(GEMMA2_9B, device=dev, post_norm_gain=4.0), dev)
        cache = model.new_cache(max(rows_list), 64)

    for M in rows_list:
        h0 = torch.randn(M, D, generator=g).to(BF).to(dev)
        x = torch.zeros(M, D, dtype=BF, device=dev)
        apply = torch.ones(M, dtype=torch.uint8, device=dev)
        idx = torch.randint(0, L, (M, mmax), generator=g, dtype=torch.int32).to(dev)
        cnt = torch.full((M,), mmax, dtype=torch.int32, device=dev)
        coef = torch.zeros(M, mmax, device=dev)
        h = h0.clone()
        acts = sae.encode(h0)
        ent = {"rows": M, "l0": round(float((acts != 0).sum(1).float().mean()), 1)}

        def hook_work():
            a = sae.encode(h0)
            ops.sae_splice_edit(h, apply, a, idx, cnt, sae.W_dec, sae.b_dec, 1.0, wn, 1e-6, x)

        ent["encode"] = timed(lambda: sae.encode(h0))
        ent["splice"] = timed(lambda: ops.sae_splice_edit(h, apply, acts, idx, cnt, sae.W_dec, sae.b_dec, 1.0, wn,
                                                          1e-6, x))
        ent["encode+splice"] = timed(hook_work)

        def lowrank():
            h.copy_(h0)                                                 # the edit is in place: same input every call
            ops.lowrank_edit(h, apply, idx, cnt, sae.W_encT, sae.W_dec, sae.b_enc, sae.threshold, None, 1.0, wn,
                             1e-6, x, coef)

        ent["lowrank_edit"] = timed(lowrank)
        if model is not None:
            ids = torch.randint(0, 1000, (M, 1), generator=g, dtype=torch.int32).to(dev)
            pos = torch.full((M, 1), 32, dtype=torch.int32, device=dev)
            slot = torch.arange(M, dtype=torch.int32, device=dev)

            def step():
                xo = model.forward(ids, pos, cache, slot)
                ops.decode_head(model.logits(xo), model.spec.final_softcap)

            # replayed from a hipGraph as the engine runs it (eager launches would inflate the step); eager if the
            # capture is refused
            run, ent["decode_step_graph"] = step, False
            try:
                for _ in range(2):
                    step()
                torch.cuda.synchronize()
                cg = torch.cuda.CUDAGraph()
                with torch.cuda.graph(cg):
                    step()
                run, ent["decode_step_graph"] = cg.replay, True
            except RuntimeError as e:
                print(f"graph capture failed, timing the eager step: {e}", flush=True)
                torch.cuda.synchronize()
            ent["decode_step"] = timed(run, warm=2, reps=5, inner=2)
            ent["hook_share_of_step_pct"] = round(100 * ent["encode+splice"]["ms"] / ent["decode_step"]["ms"], 2)
        res["decode"].append(ent)
        print(json.dumps(ent), flush=True)

    # the teacher-forced tail: ~30k flagged rows (7920 cells x ~4 spikes) splicing from a 480-row per-step table
    M, R = 30720, 480
    tab = sae.encode(torch.randn(R, D, generator=g).to(BF).to(dev))
    h = torch.randn(M, D, generator=g).to(BF).to(dev)
    x = torch.zeros(M, D, dtype=BF, device=dev)
    apply = torch.ones(M, dtype=torch.uint8, device=dev)
    src = torch.randint(0, R, (M,), generator=g, dtype=torch.int32).to(dev)
    idx = torch.randint(0, L, (M, mmax), generator=g, dtype=torch.int32).to(dev)
    cnt = torch.full((M,), mmax, dtype=torch.int32, device=dev)
    res["tail"] = {"rows": M, "table_rows": R,
                   "splice": timed(lambda: ops.sae_splice_edit(h, apply, tab, idx, cnt, sae.W_dec, sae.b_dec, 1.0, wn,
                                                               1e-6, x, src), reps=5, inner=2),
                   "table_encode": timed(lambda: sae.encode(h[:R]))}
    flags = (torch.rand(64 * 512, generator=g) < K / 512).to(torch.uint8).to(dev)
    rows = torch.empty(64 * K * 2, dtype=torch.int32, device=dev)
    inv = torch.empty(flags.numel(), dtype=torch.int32, device=dev)
    res["flag_compact"] = {"flags": flags.numel(), "cap": rows.numel(),
                           **timed(lambda: ops.flag_compact(flags, rows.numel(), rows=rows, inv=inv))}
    print(json.dumps({"tail": res["tail"], "flag_compact": res["flag_compact"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
