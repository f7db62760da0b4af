"""What the output-shift readout costs, on the GPU.

Kernel (default): ``ops.head_shift`` against plain ``ops.decode_head`` on the same bf16 logits ``[rows, 256000]`` (cap
30) for 512 / 2048 / 4096 rows, against baseline tables of 64 and 512 distinct rows with a rowmap that repeats each
baseline row over a run of consecutive edited rows, as the sweep's tail does (a pair's cells follow each other and
share its rows).  ``head_shift`` reads two rows per output row -- the baseline rows mostly from cache, being few -- and
does two table lookups and two exponentials per vocab entry where ``decode_head`` does one of each.  The two kernels
alternate window by window in one process, so clock and cache state drift hits both alike; the ratio is the median over
the window pairs.  TB/s = bytes of the *edited* logits read once over the median time (the same bytes ``decode_head``
reads), and ``shift_TBps_both`` counts the baseline rows' bytes as well, as if none came from cache.

End to end (``--sweep N``): the 9B-geometry sweep (``configs/ll_baseline_9b.yaml``, random weights) run ``N`` times
with the switch off and ``N`` times with it on, alternating, each in a fresh process; the phase times are read from
each run's ``sweep_summary.json``.

Report only (no threshold):

    python tools/head_shift_bench.py [--out FILE.jsonl]
    python tools/head_shift_bench.py --sweep 2 [--out FILE.jsonl] [--sweep-args "--set runtime.batch_size=4096"]
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


def interleaved(fa, fb, warm: int = 3, reps: int = 12, inner: int = 5):
    """Milliseconds per call of ``fa`` (shift) and ``fb`` (plain head) over ``reps`` alternating windows of ``inner``
    calls (device events), and ``fa / fb`` per window pair."""
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
    V, cap = args.vocab, args.cap
    g = torch.Generator(device=dev).manual_seed(0)
    med = statistics.median
    lines = []
    for R in (int(r) for r in args.rows.split(",")):
        lg = (torch.randn(R, V, generator=g, device=dev) * 4).to(BF)
        tgt = torch.randint(0, V, (R,), generator=g, device=dev, dtype=torch.int32)
        nxt = torch.empty(R, dtype=torch.int32, device=dev)
        ns, nt = torch.empty(R, device=dev), torch.empty(R, device=dev)
        kl, klr = torch.empty(R, device=dev), torch.empty(R, device=dev)
        for Rb in (int(b) for b in args.base_rows.split(",")):
            Rb = min(Rb, R)
            base = (torch.randn(Rb, V, generator=g, device=dev) * 4).to(BF)
            rm = (torch.arange(R, device=dev) * Rb // R).to(torch.int32)       # runs of R / Rb rows per baseline row
            sh = lambda: ops.head_shift(lg, base, rm, cap, kl, klr)             # noqa: E731
            pl = lambda: ops.decode_head(lg, cap, tgt, nxt, ns, nt)             # noqa: E731
            sh()
            ok = bool(torch.isfinite(kl).all() and (kl > 0).all())
            ident = ops.head_shift(base[rm.long()[: min(R, 64)]].contiguous(), base, rm[: min(R, 64)].contiguous(), cap)
            ta, tb, ratio = interleaved(sh, pl)
            gb = R * V * 2 / 1e9
            ent = {"rows": R, "vocab": V, "base_rows": Rb, "shift_ms": round(med(ta), 4), "plain_ms": round(med(tb), 4),
                   "shift_TBps": round(gb / med(ta), 3), "shift_TBps_both": round(2 * gb / med(ta), 3),
                   "plain_TBps": round(gb / med(tb), 3),
                   "ratio": {"median": round(med(ratio), 4), "min": round(min(ratio), 4), "max": round(max(ratio), 4)},
                   "finite_positive": ok, "identical_rows_exact_zero": not bool(ident[0].any() or ident[1].any())}
            lines.append(json.dumps(ent))
            print(lines[-1], flush=True)
            del base
        del lg
    return lines


def sweep_ab(args) -> list:
    """``args.sweep`` alternating (off, on) pairs of the 9B-geometry sweep, each a fresh process."""
    lines = []
    tmp = tempfile.mkdtemp(prefix="head_shift_ab_")
    for i in range(args.sweep):
        for tag, flag in (("off", []), ("on", ["--output-shift"])):
            out = os.path.join(tmp, f"{tag}{i}")
            cmd = [sys.executable, "-m", "taboo_brittleness_amd", "run_sweep", args.config, "--methods", args.methods,
                   "--out", out] + shlex.split(args.sweep_args) + flag
            t0 = time.perf_counter()
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.sweep_timeout)
            wall = time.perf_counter() - t0
            ent = {"run": i, "output_shift": tag == "on", "rc": r.returncode, "wall_s": round(wall, 2)}
            sp = os.path.join(out, "sweep_summary.json")
            if r.returncode == 0 and os.path.exists(sp):
                s = json.load(open(sp))
                ent["timing"] = s.get("timing") or s.get("timings")
                ent["n_cells"] = sum(c["n"] for c in s["curves"])
                ent["kl_out_mean"] = {f"{c['method']}:{c['budget']}": round(c["kl_out_mean"]["mean"], 6)
                                      for c in s["curves"] if "kl_out_mean" in c}
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
    ap.add_argument("--base-rows", default="64,512")
    ap.add_argument("--vocab", type=int, default=256000)
    ap.add_argument("--cap", type=float, default=30.0)
    ap.add_argument("--sweep", type=int, default=0, help="pairs of (off, on) end-to-end sweep runs instead of the kernel")
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "ll_baseline_9b.yaml"))
    ap.add_argument("--methods", default="all")
    ap.add_argument("--sweep-args", default="--set runtime.batch_size=4096")
    ap.add_argument("--sweep-timeout", type=float, default=900.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_shift_bench needs the GPU (a CPU time says nothing about this path)")
    lines = sweep_ab(args) if args.sweep else kernel_bench(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
