"""What the norm-matched control costs, on the GPU: ``ops.matched_noise_edit`` against ``ops.lowrank_edit`` (the
error-preserving edit whose norm it matches) on the same rows at the 9B shapes (D = 3584, d_sae = 16384, fp32 SAE
tables): m = 1 / 8 / 32 selected latents on 64 / 512 / 2048 decode rows, every row flagged.  The control reads what
``lowrank_edit`` reads (the encoder and decoder rows of the selected latents); what it adds is D Box-Muller evaluations
in fp64 per edited row.  The two kernels alternate window by window in one process, so clock and cache state drift
hits both alike; the ratio is the median over the window pairs.

Report only (no threshold):

    python tools/matched_noise_bench.py [--out FILE.json]
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


def window(fn, inner: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def interleaved(fa, fb, warm: int = 3, reps: int = 12, inner: int = 5) -> dict:
    """Milliseconds per call of ``fa`` (the control) and ``fb`` (``lowrank_edit``) over ``reps`` alternating windows
    of ``inner`` calls (device events), and ``fa / fb`` per window pair."""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window(fa, inner))
        tb.append(window(fb, inner))
    ratio = [x / y for x, y in zip(ta, tb)]
    st = lambda v: {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}  # noqa
    return {"noise": st(ta), "lowrank": st(tb),
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
        seeds = torch.randint(0, 2 ** 62, (M,), generator=g, dtype=torch.int64).to(dev)
        pos = torch.randint(0, 512, (M,), generator=g, dtype=torch.int32).to(dev)
        for m in ms_list:
            idx = torch.randint(0, L, (M, m), generator=g, dtype=torch.int32)
            idx[:, : m // 2] = fired[:, : m // 2]
            idx = idx.to(dev)
            cnt = torch.full((M,), m, dtype=torch.int32, device=dev)
            apply = torch.ones(M, dtype=torch.uint8, device=dev)
            x = torch.zeros(M, D, dtype=BF, device=dev)
            coef = torch.zeros(M, m, device=dev)
            norm = torch.zeros(M, device=dev)
            h = h0.clone()

            def noise():
                h.copy_(h0)                                             # the edits are in place: same input every call
                ops.matched_noise_edit(h, apply, idx, cnt, sae.W_encT, sae.W_dec, seeds, pos, None, sae.b_enc,
                                       sae.threshold, None, 1.0, wn, 1e-6, x, coef, norm)

            def lowrank():
                h.copy_(h0)
                ops.lowrank_edit(h, apply, idx, cnt, sae.W_encT, sae.W_dec, sae.b_enc, sae.threshold, None, 1.0, wn,
                                 1e-6, x, coef)

            ent = {"rows": M, "m": m, **interleaved(noise, lowrank)}
            noise()
            ent["edited_rows_pct"] = round(100 * float((norm > 0).float().mean()), 1)   # rows that drew their noise
            out.append(ent)
            print(json.dumps(ent), flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="64,512,2048")
    ap.add_argument("--m", default="1,8,32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("matched_noise_bench needs the GPU (a CPU time says nothing about this path)")
    dev = torch.device("cuda:0")
    res = {"shapes": {"D": 3584, "d_sae": 16384, "tables": "fp32", "alpha": 1.0},
           "kernels": kernels(dev, [int(r) for r in args.rows.split(",")], [int(m) for m in args.m.split(",")])}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
