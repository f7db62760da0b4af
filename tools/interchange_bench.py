"""What the interchange (donor-swap) edit costs, on the GPU: ``ops.interchange_edit`` against ``ops.lowrank_edit`` on
identical rows, ``idx`` and ``cnt`` at the 9B shapes (D = 3584, d_sae = 16384, fp32 SAE tables): m = 16 / 64 selected
latents (budgets 8 / 32: the target's and the donor's sets) and a rank-8 basis on 64 / 512 / 2048 decode rows, every
row flagged, every row with a donor row of its own.  The interchange kernel runs the coefficient stage twice (on the
row and on its donor row) and shares everything else with ``lowrank_edit``, so the ratio should lie between 1x and
2x.  The two kernels alternate window by window in one process, so clock and cache state drift hits both alike; the
ratio is the median over the window pairs.

Report only (no threshold):

    python tools/interchange_bench.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from taboo_brittleness_amd import ops  # noqa: E402
from taboo_brittleness_amd.interp.analysis import random_subspace  # noqa: E402
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
    """Milliseconds per call of ``fa`` (``interchange_edit``) and ``fb`` (``lowrank_edit``) over ``reps`` alternating
    windows of ``inner`` calls (device events), and ``fa / fb`` per window pair."""
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
    return {"interchange": st(ta), "lowrank": st(tb),
            "ratio": {"median": round(statistics.median(ratio), 4), "min": round(min(ratio), 4),
                      "max": round(max(ratio), 4)}}


def kernels(dev, rows_list, ms_list, rank: int) -> list:
    D, L = 3584, 16384
    g = torch.Generator().manual_seed(0)
    sae = JumpReLUSAE.random(D, L, seed=1, device=dev)                 # fp32 tables
    U = random_subspace(D, rank, seed=7, device=dev)                   # [rank, D] fp32, orthonormal rows
    wn = (torch.randn(D, generator=g) * 0.1).to(BF).to(dev)
    out = []
    for M in rows_list:
        h0 = torch.randn(M, D, generator=g).to(BF).to(dev)
        donor = torch.randn(M, D, generator=g).to(BF).to(dev)          # one donor row per row, in another order
        src = torch.randperm(M, generator=g).to(torch.int32).to(dev)
        # a quarter of the selected latents fire on the row, a quarter on its donor row, the rest are drawn at random
        fired = torch.topk(sae.encode(h0), 16, dim=1).indices.to(torch.int32).cpu()
        dfired = torch.topk(sae.encode(donor.index_select(0, src.long())), 16, dim=1).indices.to(torch.int32).cpu()
        apply = torch.ones(M, dtype=torch.uint8, device=dev)
        x = torch.zeros(M, D, dtype=BF, device=dev)
        cases = []
        for m in ms_list:
            idx = torch.randint(0, L, (M, m), generator=g, dtype=torch.int32)
            q = min(m // 4, 16)
            idx[:, :q] = fired[:, :q]
            idx[:, q: 2 * q] = dfired[:, :q]
            cases.append((f"sae m={m}", m, idx.to(dev), (sae.W_encT, sae.W_dec), (sae.b_enc, sae.threshold)))
        cases.append((f"basis r={rank}", rank, torch.arange(rank, dtype=torch.int32).repeat(M, 1).to(dev), (U, U),
                      (None, None)))
        for name, m, idx, (E, Dm), (be, th) in cases:
            cnt = torch.full((M,), m, dtype=torch.int32, device=dev)
            coef = torch.zeros(M, m, device=dev)
            h = h0.clone()

            def swap():
                h.copy_(h0)                                             # the edits are in place: same input every call
                ops.interchange_edit(h, apply, idx, cnt, E, Dm, donor, src, be, th, None, 1.0, wn, 1e-6, x, coef)

            def lowrank():
                h.copy_(h0)
                ops.lowrank_edit(h, apply, idx, cnt, E, Dm, be, th, None, 1.0, wn, 1e-6, x, coef)

            ent = {"rows": M, "case": name, "m": m, **interleaved(swap, lowrank)}
            swap()
            ent["edited_rows_pct"] = round(100 * float((h != h0).any(1).float().mean()), 1)
            out.append(ent)
            print(json.dumps(ent), flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="64,512,2048")
    ap.add_argument("--m", default="16,64")
    ap.add_argument("--rank", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interchange_bench needs the GPU (a CPU time says nothing about this path)")
    dev = torch.device("cuda:0")
    res = {"shapes": {"D": 3584, "d_sae": 16384, "tables": "fp32", "alpha": 1.0, "rank": args.rank},
           "kernels": kernels(dev, [int(r) for r in args.rows.split(",")], [int(m) for m in args.m.split(",")],
                              args.rank)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
