"""What the component-trace readout costs, on the GPU.

Kernel (default): ``ops.seg_dots`` over 512 / 2048 / 4096 selected rows at the 9B attention shape (``X [M, 4096]``,
16 heads, ``R [M, 3584]``, the per-head readout) and at the 9B MLP shape (``X = R [M, 3584]``, one segment), ``T = 2``,
against a table of 64 blocks; the selected rows are every other row of ``M = 2 x rows`` source rows, in ascending
order, and each block gets a run of consecutive selected rows, as the sweep's tail gives them.  Two yardsticks run in
the same process, alternating with the kernel window by window so that clock and cache drift hit all alike:
``ops.lens_track`` at ``T = 2`` over the same number of contiguous 3584-wide rows (the layer trace's readout), and a
plain bf16 gather-copy of the same selected rows (``ops.row_gather``: reads and writes every byte the kernel reads of
``X``).  ``GBps`` counts the bytes the kernel must read once (the selected rows of ``X`` and of ``R``) over the median
time; the table (``T x K x 4`` bytes per block) is re-read per row from cache.

End to end (``--sweep N``): the 9B-geometry sweep (``configs/ll_baseline_9b.yaml``, random weights) run ``N`` times with
the switch off and ``N`` times with it on, alternating, each in a fresh process; the phase times are read from each
run's ``sweep_summary.json``.

Report only (no threshold):

    python tools/comp_trace_bench.py [--out FILE.jsonl]
    python tools/comp_trace_bench.py --sweep 2 [--out FILE.jsonl] [--sweep-args "--set runtime.batch_size=4096"]
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
SHAPES = {"attn": (4096, 16, 3584), "mlp": (3584, 1, 3584)}      # (K, S, Dn)


def window(fn, inner: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def interleaved(fns, warm: int = 3, reps: int = 12, inner: int = 20):
    """Milliseconds per call of every function over ``reps`` rounds of alternating windows of ``inner`` calls."""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(ts, fns):
            t.append(window(f, inner))
    return ts


def kernel_bench(args) -> list:
    dev = torch.device("cuda:0")
    U, T = args.blocks, 2
    g = torch.Generator(device=dev).manual_seed(0)
    med = statistics.median
    lines = []
    for name in args.shapes.split(","):
        K, S, Dn = SHAPES[name]
        for Ms in (int(r) for r in args.rows.split(",")):
            M = 2 * Ms
            X = torch.randn(M, K, generator=g, device=dev).to(BF)
            R = X if name == "mlp" else torch.randn(M, Dn, generator=g, device=dev).to(BF)
            W = 0.1 * torch.randn(U, T, K, generator=g, device=dev)
            V = 0.1 * torch.randn(U, T, Dn, generator=g, device=dev)
            rows = (2 * torch.arange(Ms, device=dev)).to(torch.int32)
            blk = (torch.arange(Ms, device=dev) * U // Ms).to(torch.int32)
            out = torch.empty(Ms, T, S, device=dev)
            rms = torch.empty(Ms, device=dev)
            dst = torch.empty(Ms, K, dtype=BF, device=dev)
            hl = R[:Ms].contiguous()
            lo = torch.empty(Ms, T, device=dev)
            rows64 = rows.long()
            sd = lambda: ops.seg_dots(X, W, rows, blk, S, R, 1e-6, out=out, rms=rms)     # noqa: E731
            lt = lambda: ops.lens_track(hl, V, blk, 1e-6, 0.0, out=lo)                   # noqa: E731
            cp = lambda: ops.row_gather(X, rows64, dst)                                  # noqa: E731
            sd()
            want, _ = ops.seg_dots(X.cpu(), W.cpu(), rows[:32].cpu(), blk[:32].cpu(), S, R.cpu(), 1e-6)
            ok = bool(torch.isfinite(out).all()) and bool(torch.allclose(out[:32].cpu(), want, rtol=1e-3, atol=1e-3))
            ta, tb, tc = interleaved([sd, lt, cp])
            gb = Ms * (K + (0 if name == "mlp" else Dn)) * 2 / 1e9
            ent = {"shape": name, "K": K, "S": S, "Dn": Dn, "T": T, "rows": Ms, "blocks": U,
                   "seg_dots_ms": round(med(ta), 5), "lens_track_ms": round(med(tb), 5),
                   "gather_copy_ms": round(med(tc), 5), "seg_dots_GBps": round(gb / med(ta) * 1e3, 1),
                   "gather_copy_GBps": round(2 * Ms * K * 2 / 1e9 / med(tc) * 1e3, 1),
                   "vs_lens_track": round(med([x / y for x, y in zip(ta, tb)]), 3),
                   "vs_gather_copy": round(med([x / y for x, y in zip(ta, tc)]), 3),
                   "spread_ms": [round(min(ta), 5), round(max(ta), 5)], "matches_reference": ok}
            lines.append(json.dumps(ent))
            print(lines[-1], flush=True)
    return lines


def sweep_ab(args) -> list:
    """``args.sweep`` alternating (off, on) pairs of the 9B-geometry sweep, each a fresh process."""
    lines = []
    tmp = tempfile.mkdtemp(prefix="comp_trace_ab_")
    for i in range(args.sweep):
        for tag, flag in (("off", []), ("on", ["--component-trace"])):
            out = os.path.join(tmp, f"{tag}{i}")
            cmd = [sys.executable, "-m", "taboo_brittleness_amd", "run_sweep", args.config, "--methods", args.methods,
                   "--out", out] + shlex.split(args.sweep_args) + flag
            t0 = time.perf_counter()
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.sweep_timeout)
            wall = time.perf_counter() - t0
            ent = {"run": i, "component_trace": tag == "on", "rc": r.returncode, "wall_s": round(wall, 2)}
            sp = os.path.join(out, "sweep_summary.json")
            if r.returncode == 0 and os.path.exists(sp):
                s = json.load(open(sp))
                ent["timing"] = s.get("timing") or s.get("timings")
                ent["n_cells"] = sum(c["n"] for c in s["curves"])
                ent["comp_top"] = {f"{c['method']}:{c['budget']}": round(max(
                    (abs(v) for row in c["comp_dz_spike"] for v in row), default=0.0), 5)
                    for c in s["curves"] if "comp_dz_spike" in c}
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
    ap.add_argument("--shapes", default="attn,mlp")
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--sweep", type=int, default=0,
                    help="pairs of (off, on) end-to-end sweep runs instead of the kernel")
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "ll_baseline_9b.yaml"))
    ap.add_argument("--methods", default="all")
    ap.add_argument("--sweep-args", default="--set runtime.batch_size=4096")
    ap.add_argument("--sweep-timeout", type=float, default=900.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("comp_trace_bench needs the GPU (a CPU time says nothing about this path)")
    lines = sweep_ab(args) if args.sweep else kernel_bench(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
