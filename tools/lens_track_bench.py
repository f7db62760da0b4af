"""What the layer-trace readout costs, on the GPU.

Kernel (default): ``ops.lens_track`` on bf16 residual rows ``[rows, 3584]`` for 512 / 2048 / 4096 rows with T = 2 and
8 tracked columns (cap 30), against a table of 64 blocks and a row map that gives each block a run of consecutive rows,
as the sweep's tail does (a pair's cells follow each other and share its block).  The yardstick is a plain bf16 copy of
the same rows (``Tensor.copy_``) in the same process: the kernel reads ``h`` once and writes ``T`` floats per row, the
copy reads and writes it, so at the same memory rate the kernel would take half the copy's time.  The two alternate
window by window, so clock and cache state drift hits both alike; the ratio is the median over the window pairs.
GB/s = bytes of ``h`` read once over the median time; ``copy_GBps`` counts the copy's bytes both ways.
``--scattered`` adds a row map that changes block at every row (every wave takes its rows one at a time against the
table in global memory): what staging the table buys.

End to end (``--sweep N``): the 9B-geometry sweep (``configs/ll_baseline_9b.yaml``, random weights) run ``N`` times
with the switch off and ``N`` times with it on, alternating, each in a fresh process; the phase times are read from
each run's ``sweep_summary.json``.

Report only (no threshold):

    python tools/lens_track_bench.py [--out FILE.jsonl] [--scattered]
    python tools/lens_track_bench.py --sweep 2 [--out FILE.jsonl] [--sweep-args "--set runtime.batch_size=4096"]
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

from taboo_brittleness_amd import ops  # noqa: E402

BF = torch.bfloat16


def window(fn, inner: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def interleaved(fa, fb, warm: int = 3, reps: int = 12, inner: int = 20):
    """Milliseconds per call of ``fa`` (trace) and ``fb`` (copy) over ``reps`` alternating windows of ``inner`` calls
    (device events), and ``fa / fb`` per window pair."""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window(fa, inner))
        tb.append(window(fb, inner))
    return ta, tb, [x / y for x, y in zip(ta, tb)]


def kernel_bench(args) -> list:
    dev = torch.device("cuda:0")
    D, cap, U = args.width, args.cap, args.blocks
    g = torch.Generator(device=dev).manual_seed(0)
    med = statistics.median
    lines = []
    for R in (int(r) for r in args.rows.split(",")):
        h = torch.randn(R, D, generator=g, device=dev).to(BF)
        dst = torch.empty_like(h)
        for T in (int(t) for t in args.cols.split(",")):
            V = 0.1 * torch.randn(U, T, D, generator=g, device=dev)
            out = torch.empty(R, T, device=dev)
            maps = {"runs": (torch.arange(R, device=dev) * U // R).to(torch.int32)}
            if args.scattered:
                maps["scattered"] = (torch.arange(R, device=dev) % U).to(torch.int32)
            for name, vr in maps.items():
                tr = lambda: ops.lens_track(h, V, vr, 1e-6, cap, out=out)          # noqa: E731
                cp = lambda: dst.copy_(h)                                          # noqa: E731
                tr()
                want = ops.lens_track(h[:64].cpu(), V.cpu(), vr[:64].cpu(), 1e-6, cap)
                ok = bool(torch.isfinite(out).all()) and bool(torch.allclose(out[:64].cpu(), want, rtol=1e-3,
                                                                             atol=1e-3))
                ta, tb, ratio = interleaved(tr, cp)
                gb = R * D * 2 / 1e9
                ent = {"rows": R, "width": D, "T": T, "blocks": U, "map": name, "trace_ms": round(med(ta), 5),
                       "copy_ms": round(med(tb), 5), "trace_GBps": round(gb / med(ta) * 1e3, 1),
                       "copy_GBps": round(2 * gb / med(tb) * 1e3, 1),
                       "ratio": {"median": round(med(ratio), 4), "min": round(min(ratio), 4),
                                 "max": round(max(ratio), 4)}, "matches_reference": ok}
                lines.append(json.dumps(ent))
                print(lines[-1], flush=True)
    return lines


def sweep_ab(args) -> list:
    """``args.sweep`` alternating (off, on) pairs of the 9B-geometry sweep, each a fresh process."""
    lines = []
    tmp = tempfile.mkdtemp(prefix="lens_track_ab_")
    for i in range(args.sweep):
        for tag, flag in (("off", []), ("on", ["--layer-trace"])):
            out = os.path.join(tmp, f"{tag}{i}")
            cmd = [sys.executable, "-m", "taboo_brittleness_amd", "run_sweep", args.config, "--methods", args.methods,
                   "--out", out] + shlex.split(args.sweep_args) + flag
            t0 = time.perf_counter()
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.sweep_timeout)
            wall = time.perf_counter() - t0
            ent = {"run": i, "layer_trace": tag == "on", "rc": r.returncode, "wall_s": round(wall, 2)}
            sp = os.path.join(out, "sweep_summary.json")
            if r.returncode == 0 and os.path.exists(sp):
                s = json.load(open(sp))
                ent["timing"] = s.get("timing") or s.get("timings")
                ent["n_cells"] = sum(c["n"] for c in s["curves"])
                ent["trace_recovery"] = {f"{c['method']}:{c['budget']}": round(c["trace_recovery"]["mean"], 4)
                                         for c in s["curves"] if "trace_recovery" in c}
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
    ap.add_argument("--cols", default="2,8")
    ap.add_argument("--width", type=int, default=3584)
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--cap", type=float, default=30.0)
    ap.add_argument("--scattered", action="store_true", help="also time a row map that changes block at every row")
    ap.add_argument("--sweep", type=int, default=0,
                    help="pairs of (off, on) end-to-end sweep runs instead of the kernel")
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "ll_baseline_9b.yaml"))
    ap.add_argument("--methods", default="all")
    ap.add_argument("--sweep-args", default="--set runtime.batch_size=4096")
    ap.add_argument("--sweep-timeout", type=float, default=900.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lens_track_bench needs the GPU (a CPU time says nothing about this path)")
    lines = sweep_ab(args) if args.sweep else kernel_bench(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
