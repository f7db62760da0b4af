"""Fixed cost per output-tile slot of the 256-row gemm4 tile: time g256 over K in {1792 .. 14336} at fixed M, N
(gate|up, vocab head, down), medians of interleaved repeats, and fit  time / rounds = a + b * (K / 64).  With a build
that has ``gemm4_set_pipe`` the plain (pipe 0) and the streamed (pipe 1) tile loop are interleaved; ``--rates`` adds the
kernel rates at the sweep's shapes against hipBLASLt.  (profiles/r7/g4pipe/)

    python tools/g4_fixed_cost.py ROOT OUT.json [--rates]      ROOT: the tree whose built package is imported"""
import json
import statistics
import sys

root, out = sys.argv[1], sys.argv[2]
rates = "--rates" in sys.argv
sys.path.insert(0, root)
import torch  # noqa: E402

from taboo_brittleness_amd import ops  # noqa: E402

k = ops._k()
dev = torch.device("cuda:0")
BF = torch.bfloat16
has_pipe = hasattr(k, "gemm4_set_pipe")
modes = [0, 1] if has_pipe else [None]
CUS = torch.cuda.get_device_properties(0).multi_processor_count
KS = [1792, 3584, 7168, 14336]
SHAPES = [("gateup", 4096, 28672, 3), ("head", 4096, 256000, 0), ("down", 20480, 3584, 0)]


def make(M, N, K, epi):
    torch.manual_seed(1)
    A = ((torch.rand(M, K, device=dev) * 2 - 1) * 0.5).to(BF)
    W = ((torch.rand(N, K, device=dev) * 2 - 1) * 0.5).to(BF)
    C = torch.empty(M, N // 2 if epi == 3 else N, device=dev, dtype=BF)
    return A, W, C


def run(A, W, C, epi, mode, n):
    if mode is not None:
        k.gemm4_set_pipe(mode)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        k.gemm4(A, W, C, None, None, epi, 256)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


res = {"cus": CUS, "fit": [], "rates": []}
for name, M, N, epi in SHAPES:
    per = {m: {} for m in modes}
    for K in KS:
        A, W, C = make(M, N, K, epi)
        flop = 2.0 * M * N * K
        n = max(3, int(2e14 / flop))          # ~0.15 s per sample
        for m in modes:
            run(A, W, C, epi, m, 3)
        samp = {m: [] for m in modes}
        for _ in range(9):
            for m in modes:                   # interleaved
                samp[m].append(run(A, W, C, epi, m, n))
        for m in modes:
            per[m][K] = samp[m]
        del A, W, C
    tiles = ((M + 255) // 256) * (N // 256)
    rounds = -(-tiles // CUS)
    for m in modes:
        xs = [K // 64 for K in KS]
        ys = [statistics.median(per[m][K]) / rounds for K in KS]
        mx, my = sum(xs) / 4, sum(ys) / 4
        b = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
        a = my - b * mx
        rec = {"shape": name, "M": M, "N": N, "epi": epi, "pipe": m, "rounds": rounds, "a_us": round(a, 3),
               "b_us": round(b, 4), "us": {K: round(statistics.median(per[m][K]), 2) for K in KS},
               "spread_us": {K: round(max(per[m][K]) - min(per[m][K]), 2) for K in KS},
               "tile_us_K3584": round(ys[1], 2), "a_frac_K3584": round(a / ys[1], 4)}
        res["fit"].append(rec)
        print(json.dumps(rec), flush=True)

if rates:
    R = [("gateup", 28672, 3584, 3), ("logits", 256000, 3584, 0), ("down", 3584, 14336, 0), ("oproj", 3584, 4096, 0),
         ("qkv_as_bf16", 8192, 3584, 0)]
    for name, N, K, epi in R:
        for M in ((4096, 20480) if name in ("down", "oproj") else (4096, 32768)):
            if name == "logits" and M == 32768:
                M = 16384                      # 32768 x 256000 bf16 logits = 16.8 GB of output: keep the box's memory
            A, W, C = make(M, N, K, epi)
            flop = 2.0 * M * N * K
            n = max(3, int(2e14 / flop))
            Cb = torch.empty(M, N, device=dev, dtype=BF) if epi == 0 else None
            samp = {m: [] for m in modes}
            blas = []
            for m in modes:
                run(A, W, C, epi, m, 3)
            if Cb is not None:
                torch.matmul(A, W.T, out=Cb)
            for _ in range(7):
                for m in modes:
                    samp[m].append(run(A, W, C, epi, m, n))
                if Cb is not None:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n):
                        torch.matmul(A, W.T, out=Cb)
                    e1.record()
                    e1.synchronize()
                    blas.append(e0.elapsed_time(e1) * 1e3 / n)
            rec = {"shape": name, "M": M, "N": N, "K": K, "epi": epi}
            for m in modes:
                md = statistics.median(samp[m])
                rec[f"pipe{m}_us"] = round(md, 2)
                rec[f"pipe{m}_spread_us"] = round(max(samp[m]) - min(samp[m]), 2)
                rec[f"pipe{m}_tflops"] = round(flop / md / 1e6, 1)
            if blas:
                rec["blas_us"] = round(statistics.median(blas), 2)
                rec["blas_tflops"] = round(flop / statistics.median(blas) / 1e6, 1)
            res["rates"].append(rec)
            print(json.dumps(rec), flush=True)
            del A, W, C, Cb

with open(out, "w") as f:
    json.dump(res, f, indent=1)
