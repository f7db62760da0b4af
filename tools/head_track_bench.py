"""What the output-side readout costs in the vocab head, on the GPU: ``ops.decode_head_track`` against plain
``ops.decode_head`` on the same bf16 logits ``[rows, 256000]`` (cap 30, a teacher target per row), for 64 / 512 / 2048 /
4096 rows with ``T = 2`` tracked ids both ranked, ``T = 8`` of which 2 ranked, ``T = 6`` of which 3 ranked (a sweep
with swap methods over two words: the other word's secret is ranked too) and ``T = 8`` all ranked (the most the kernel
does).  The tracking kernel streams the row exactly as the plain one and adds one compare per logit
and ranked column, so the ratio should grow with the ranked columns and not with ``T``.  The two kernels alternate
window by window in one process, so clock and cache state drift hits both alike; the ratio is the median over the
window pairs.  TB/s = bytes of logits read once over the median time.

Report only (no threshold):

    python tools/head_track_bench.py [--out FILE.jsonl]
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
CASES = (("T=2 ranked 2", 2, 2), ("T=8 ranked 2", 8, 2), ("T=6 ranked 3", 6, 3), ("T=8 ranked 8", 8, 8))


def window(fn, inner: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def interleaved(fa, fb, warm: int = 3, reps: int = 12, inner: int = 5):
    """Milliseconds per call of ``fa`` (tracking) and ``fb`` (plain) over ``reps`` alternating windows of ``inner``
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="64,512,2048,4096")
    ap.add_argument("--vocab", type=int, default=256000)
    ap.add_argument("--cap", type=float, default=30.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_track_bench needs the GPU (a CPU time says nothing about this path)")
    dev = torch.device("cuda:0")
    V, cap = args.vocab, args.cap
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for R in (int(r) for r in args.rows.split(",")):
        lg = (torch.randn(R, V, generator=g, device=dev) * 4).to(BF)
        tgt = torch.randint(0, V, (R,), generator=g, device=dev, dtype=torch.int32)
        nxt = torch.empty(R, dtype=torch.int32, device=dev)
        ns, nt = torch.empty(R, device=dev), torch.empty(R, device=dev)
        p_nxt, p_ns, p_nt = (t.clone() for t in ops.decode_head(lg, cap, tgt))
        gb = R * V * 2 / 1e9
        for name, T, n_rank in CASES:
            track = torch.randint(0, V, (R, T), generator=g, device=dev, dtype=torch.int32)
            logp = torch.empty(R, T, device=dev)
            rank = torch.empty(R, T, dtype=torch.int32, device=dev)
            tr = lambda: ops.decode_head_track(lg, cap, track, n_rank, tgt, nxt, ns, nt, logp, rank)   # noqa: E731
            pl = lambda: ops.decode_head(lg, cap, tgt, nxt, ns, nt)                                    # noqa: E731
            tr()
            same = bool(torch.equal(nxt, p_nxt) and torch.equal(ns, p_ns) and torch.equal(nt, p_nt))
            ta, tb, ratio = interleaved(tr, pl)
            med = statistics.median
            ent = {"rows": R, "vocab": V, "case": name, "T": T, "n_rank": n_rank,
                   "track_ms": round(med(ta), 4), "plain_ms": round(med(tb), 4),
                   "track_TBps": round(gb / med(ta), 3), "plain_TBps": round(gb / med(tb), 3),
                   "ratio": {"median": round(med(ratio), 4), "min": round(min(ratio), 4), "max": round(max(ratio), 4)},
                   "same_bits_as_plain": same}
            lines.append(json.dumps(ent))
            print(lines[-1], flush=True)
        del lg
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
