"""What the causal latent ranking costs, on the GPU: ``ops.latent_effect`` at the 9B shapes (D = 3584,
d_sae = 16384, fp32 decoder table) on the spike rows of 64 / 120 / 240 pairs (4 spikes each: 256 / 480 / 960 rows)
with about 76 and about 300 active latents per row, both modes (0 = effect_lens, one broadcast lens direction;
1 = attr_model, one gradient row per spike row), with and without the per-row ``eff`` output.  For comparison the
correlational pass of the same pairs: ``ops.latent_score`` over all their response rows (50 per pair).

Per entry: microseconds per call (median, min, max over windows timed with device events after warm-up) and, for
``latent_effect``, the decoder bytes it gathers per second (active latents x D x 4 bytes over the median time).
Report only (no threshold):

    python tools/latent_effect_bench.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from taboo_brittleness_amd import ops  # noqa: E402

BF = torch.bfloat16
D, L, SPIKES, RESP = 3584, 16384, 4, 50


def timed(fn, warm: int = 5, reps: int = 15, inner: int = 10) -> dict:
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / inner)
    return {"us": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def sparse_acts(rows: int, l0: int, g: torch.Generator, dev) -> torch.Tensor:
    """JumpReLU-like activations: each latent fires with probability l0 / L, values in 0.5 .. 4.5 (built on the
    device in row blocks; the mask and the values come from one seeded host generator)."""
    out = torch.zeros(rows, L, device=dev)
    for r0 in range(0, rows, 1024):
        n = min(1024, rows - r0)
        u = torch.rand(n, L, generator=g)
        out[r0:r0 + n] = torch.where(u < l0 / L, 0.5 + 4.0 * torch.rand(n, L, generator=g), torch.zeros(n, L)).to(dev)
    return out


def run(dev, pairs_list, l0_list) -> list:
    g = torch.Generator().manual_seed(0)
    Wd = torch.randn(L, D, generator=g)
    Wd = (Wd / Wd.norm(dim=1, keepdim=True)).to(dev)
    out = []
    for pairs in pairs_list:
        R = pairs * SPIKES
        X = torch.randn(R, D, generator=g).to(BF).to(dev)
        V = (torch.randn(R, D, generator=g) * 0.05).to(dev)
        seg = torch.arange(0, R + 1, SPIKES, dtype=torch.int32, device=dev)
        for l0 in l0_list:
            acts = sparse_acts(R, l0, g, dev)
            active = int((acts > 0).sum())
            ent = {"pairs": pairs, "spike_rows": R, "active_per_row": round(active / R, 1),
                   "decoder_bytes": active * D * 4}
            for name, mode, v, cap in (("effect_lens", 0, V[:1].contiguous(), 30.0), ("attr_model", 1, V, 0.0)):
                for eff in (False, True):
                    t = timed(lambda: ops.latent_effect(acts, X, v, Wd, seg, 1.0, 1e-6, cap, mode, want_eff=eff))
                    t["decoder_GB_per_s"] = round(ent["decoder_bytes"] / t["us"] / 1e3, 1)
                    ent[name + ("_with_eff" if eff else "")] = t
            del acts
            out.append(ent)
            print(json.dumps(ent), flush=True)
        # the correlational pass of the same pairs: every response row of every pair (its activations exist already)
        rows = pairs * RESP
        acts = sparse_acts(rows, 76, g, dev)
        p = torch.rand(rows, generator=g).to(dev)
        spike = torch.zeros(rows, dtype=torch.uint8)
        spike[torch.arange(0, rows, RESP // SPIKES)[: pairs * SPIKES]] = 1
        rseg = torch.arange(0, rows + 1, RESP, dtype=torch.int32, device=dev)
        spike = spike.to(dev)
        ent = {"pairs": pairs, "response_rows": rows,
               "corr_latent_score": timed(lambda: ops.latent_score(acts, p, spike, rseg))}
        del acts
        out.append(ent)
        print(json.dumps(ent), flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", default="64,120,240")
    ap.add_argument("--l0", default="76,300")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("latent_effect_bench needs the GPU (a CPU time says nothing about this path)")
    dev = torch.device("cuda:0")
    res = {"shapes": {"D": D, "d_sae": L, "table": "fp32", "spikes_per_pair": SPIKES, "response_rows_per_pair": RESP},
           "entries": run(dev, [int(x) for x in args.pairs.split(",")], [int(x) for x in args.l0.split(",")])}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
