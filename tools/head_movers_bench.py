"""What the output-movers readout costs, on the GPU.

Kernel (default): ``ops.head_movers`` against ``ops.head_shift`` on the same bf16 logits ``[rows, 256000]`` (cap 30)
and the same baseline table (64 distinct rows, each repeated over a run of consecutive edited rows, as the sweep's tail
has them), for 512 / 2048 / 4096 rows with ``k`` in {1, 8} and ``T`` in {0, 8} tracked ids -- every row selected --
and once with one row in ten selected, which is the sweep's regime (``head_shift`` still reads every row there: it is
the sweep's companion kernel, not a subset of it).  ``head_movers`` streams the two rows twice (the exp-sums, then the
differences) where ``head_shift`` streams them once.  The two kernels alternate window by window in one process, so
clock and cache state drift hits both alike; the ratio is the median over the window pairs.  TB/s = bytes of the
*selected edited* logits read once over the median time; ``movers_TBps_streamed`` counts what the kernel streams: both
rows, twice.

End to end (``--sweep N``): the 9B-geometry sweep (``configs/ll_baseline_9b.yaml``, random weights) run ``N`` times
with the switch off and ``N`` times with it on, alternating, each in a fresh process; the phase times are read from
each run's ``sweep_summary.json``.

Report only (no threshold):

    python tools/head_movers_bench.py [--out FILE.jsonl]
    python tools/head_movers_bench.py --sweep 2 [--out FILE.jsonl] [--sweep-args "--set runtime.batch_size=4096"]
"""
import argparse
import json
import os
import shlex
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from head_shift_bench import interleaved  # noqa: E402  (the sibling tool's alternating device-event windows)
from taboo_brittleness_amd import ops  # noqa: E402

BF = torch.bfloat16


def kernel_bench(args) -> list:
    dev = torch.device("cuda:0")
    V, cap = args.vocab, args.cap
    g = torch.Generator(device=dev).manual_seed(0)
    med = statistics.median
    lines = []
    for R in (int(r) for r in args.rows.split(",")):
        lg = (torch.randn(R, V, generator=g, device=dev) * 4).to(BF)
        Rb = min(args.base_rows, R)
        base = (torch.randn(Rb, V, generator=g, device=dev) * 4).to(BF)
        rm = (torch.arange(R, device=dev) * Rb // R).to(torch.int32)           # runs of R / Rb rows per baseline row
        kl, klr = torch.empty(R, device=dev), torch.empty(R, device=dev)
        sh = lambda: ops.head_shift(lg, base, rm, cap, kl, klr)                 # noqa: E731
        cases = [(1, k, T) for k in (1, 8) for T in (0, 8)] + [(10, 8, 8)]
        for every, k, T in cases:
            rows = torch.arange(0, R, every, device=dev, dtype=torch.int32)
            Rs = rows.numel()
            ids = torch.randint(0, V, (Rs, T), generator=g, device=dev, dtype=torch.int32) if T else None
            outs = [torch.empty(Rs, device=dev), torch.empty(Rs, k, dtype=torch.int32, device=dev),
                    torch.empty(Rs, k, device=dev), torch.empty(Rs, k, dtype=torch.int32, device=dev),
                    torch.empty(Rs, k, device=dev), torch.empty(Rs, T, device=dev)]
            mv = lambda: ops.head_movers(lg, base, rm, rows, cap, k, ids, *outs)   # noqa: E731
            mv()
            ok = bool(torch.isfinite(outs[0]).all() and (outs[0] > 0).all() and (outs[1] >= 0).all())
            n64 = min(R, 64)
            ident = ops.head_movers(base[rm.long()[:n64]].contiguous(), base, rm[:n64].contiguous(),
                                    torch.arange(n64, device=dev, dtype=torch.int32), cap, k)
            ta, tb, ratio = interleaved(mv, sh)
            gb = Rs * V * 2 / 1e9
            ent = {"rows": R, "selected": Rs, "vocab": V, "base_rows": Rb, "k": k, "T": T,
                   "movers_ms": round(med(ta), 4), "shift_ms": round(med(tb), 4),
                   "movers_TBps": round(gb / med(ta), 3), "movers_TBps_streamed": round(4 * gb / med(ta), 3),
                   "shift_TBps": round(R * V * 2 / 1e9 / med(tb), 3),
                   "ratio": {"median": round(med(ratio), 4), "min": round(min(ratio), 4), "max": round(max(ratio), 4)},
                   "per_selected_row_ratio": round(med(ratio) * R / Rs, 4),
                   "finite_positive": ok,
                   "identical_rows_exact_zero": not bool(ident[0].any() or (ident[1] >= 0).any() or
                                                         (ident[3] >= 0).any())}
            lines.append(json.dumps(ent))
            print(lines[-1], flush=True)
        del lg, base
    return lines


def sweep_ab(args) -> list:
    """``args.sweep`` alternating (off, on) pairs of the 9B-geometry sweep, each a fresh process."""
    lines = []
    tmp = tempfile.mkdtemp(prefix="head_movers_ab_")
    for i in range(args.sweep):
        for tag, flag in (("off", []), ("on", ["--output-movers"])):
            out = os.path.join(tmp, f"{tag}{i}")
            cmd = [sys.executable, "-m", "taboo_brittleness_amd", "run_sweep", args.config, "--methods", args.methods,
                   "--out", out] + shlex.split(args.sweep_args) + flag
            t0 = time.perf_counter()
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.sweep_timeout)
            wall = time.perf_counter() - t0
            ent = {"run": i, "output_movers": tag == "on", "rc": r.returncode, "wall_s": round(wall, 2)}
            sp = os.path.join(out, "sweep_summary.json")
            if r.returncode == 0 and os.path.exists(sp):
                s = json.load(open(sp))
                ent["timing"] = s.get("timing") or s.get("timings")
                ent["n_cells"] = sum(c["n"] for c in s["curves"])
                ent["tv_out_spike_mean"] = {f"{c['method']}:{c['budget']}": round(c["tv_out_spike_mean"]["mean"], 6)
                                            for c in s["curves"] if "tv_out_spike_mean" in c}
            else:
                ent["stderr_tail"] = r.stderr[-800:]
            lines.append(json.dumps(ent))
            print(lines[-1], flush=True)
            if r.returncode != 0:             # a failed run ends the series: nothing more is started on the GPU
                return lines
    return lines


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="512,2048,4096")
    ap.add_argument("--base-rows", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=256000)
    ap.add_argument("--cap", type=float, default=30.0)
    ap.add_argument("--sweep", type=int, default=0,
                    help="pairs of (off, on) end-to-end sweep runs instead of the kernel")
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "ll_baseline_9b.yaml"))
    ap.add_argument("--methods", default="all")
    ap.add_argument("--sweep-args", default="--set runtime.batch_size=4096")
    ap.add_argument("--sweep-timeout", type=float, default=900.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_movers_bench needs the GPU (a CPU time says nothing about this path)")
    lines = sweep_ab(args) if args.sweep else kernel_bench(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
