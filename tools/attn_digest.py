"""sha256 of the attention kernels' outputs over a fixed list of calls: one line per call with the kernel route, the
shape arguments and the digest of the output's bytes.  Two builds compute the same bits iff their outputs are equal
line for line (csrc/attention.hip; profiles/r16/attn_refactor/README.md).

The calls: every case of tests/attention_cases.py through every route tests/test_attention_edges_gpu.py::_routes gives
it (cache dense and packed, tail, wave, split, decode), and the inputs of test_attention_tail_matches_decode_bitwise,
test_attention_decode_split_bitequal, test_attention_decode_wave_s2048, test_attention_decode_shared_prefix_buckets
and test_attention_varlen_shared_prefix (tests/test_kernels_gpu.py), rebuilt from the same seeds.

  python tools/attn_digest.py [--root CHECKOUT] > digest.txt

``--root``: import the package (and its built extension) from another checkout; the cases and routes are always this
tree's.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE, help="checkout whose taboo_brittleness_amd (and extension) is imported")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.abspath(args.root))
    from taboo_brittleness_amd import ops
    from taboo_brittleness_amd.models.gemma2 import packed_blocks

    import attention_cases as ac
    import test_attention_edges_gpu as edges

    gpu = torch.device("cuda:0")
    print(f"# package {os.path.dirname(ops.__file__)}", file=sys.stderr)
    d = lambda t: t.to(gpu)                                # noqa: E731
    k = ops._k()

    def emit(route, what, out):
        torch.cuda.synchronize()
        print(f"{route} {what} {tuple(out.shape)} {sha(out)}", flush=True)

    class split_rows:
        """Both split thresholds at ``n`` inside the block, restored after it."""
        def __init__(self, n):
            self.n = n

        def __enter__(self):
            self.old = k.attention_split_rows(self.n, True), k.attention_split_rows(self.n, False)

        def __exit__(self, *exc):
            k.attention_split_rows(self.old[0], True)
            k.attention_split_rows(self.old[1], False)

    # ---- the edge cases, every route
    for name in ac.CASE_NAMES:
        c = ac.case(name)
        for kernel, how in edges._routes(c):
            out = edges._run(c, kernel, how, gpu)
            emit(f"{kernel}/{how}", f"{name} HD={c.HD} G={c.G} S={c.S} B={c.B} T={c.T} window={c.window} cap={c.cap:g} "
                 f"prefix={int(c.prefix is not None)}", out)

    # ---- test_attention_tail_matches_decode_bitwise
    for G, HD in ((2, 256), (4, 256), (1, 128)):
        for S, window, qmul in [(S, w, 2) for S in (120, 272, 512) for w in (0, 16, 33)] + [(272, 33, 12)]:
            torch.manual_seed(31)
            Hkv = 4
            Hq = Hkv * G
            kc, vc = d(torch.randn(6, Hkv, S, HD, dtype=BF)), d(torch.randn(6, Hkv, S, HD, dtype=BF))
            pk, pv = d(torch.randn(3, Hkv, S, HD, dtype=BF)), d(torch.randn(3, Hkv, S, HD, dtype=BF))
            spec = [(3, 10, 23, 1, 12), (0, 40, 1, 0, 0), (4, 5, 13, 2, 9), (1, S - 50, 40, 1, S - 45), (5, 0, 9, 0, 0)]
            pos, slot_rows, seqs, ps_rows, pl_rows = [], [], [], [], []
            for sl, p0, n, ps, pl in spec:
                seqs.append((len(pos), n, sl, ps, pl))
                pos += list(range(p0, p0 + n))
                slot_rows += [sl] * n
                ps_rows += [ps] * n
                pl_rows += [pl] * n
            pos[30] = -1
            M = len(pos)
            pos_t, sr = d(torch.tensor(pos, dtype=torch.int32)), d(torch.tensor(slot_rows, dtype=torch.int32))
            q = d(torch.randn(M, Hq, HD, dtype=BF) * qmul)
            what = f"tail_bitwise HD={HD} G={G} S={S} window={window} qmul={qmul}"
            for prefix in (False, True):
                blk = d(packed_blocks(seqs if prefix else [s[:3] for s in seqs], 16 // G))
                emit("tail/packed", f"{what} prefix={int(prefix)}",
                     ops.attention_varlen(q, kc, vc, pos_t, sr, blk, HD ** -0.5, 50.0, window,
                                          prefix_kv=(pk, pv) if prefix else None))
                pre = (pk, pv, d(torch.tensor(ps_rows, dtype=torch.int32)), d(torch.tensor(pl_rows, dtype=torch.int32)))
                for route, n in (("wave/rows", 0), ("split/rows", 1 << 20)):
                    if route.startswith("split") and not (HD == 256 and G in (2, 4)):
                        continue
                    with split_rows(n):
                        emit(route, f"{what} prefix={int(prefix)}",
                             ops.attention(q, kc, vc, pos_t, sr, M, 1, HD ** -0.5, 50.0, window,
                                           prefix=pre if prefix else None))

    # ---- test_attention_decode_split_bitequal
    for G, S in ((2, 96), (2, 700), (4, 300)):
        torch.manual_seed(19)
        Hkv, HD, B, P = 4, 256, 37, 5
        kc, vc = d(torch.randn(B, Hkv, S, HD, dtype=BF)), d(torch.randn(B, Hkv, S, HD, dtype=BF))
        pk, pv = d(torch.randn(P, Hkv, S, HD, dtype=BF)), d(torch.randn(P, Hkv, S, HD, dtype=BF))
        q = d(torch.randn(B, Hkv * G, HD, dtype=BF) * 2)
        slot = torch.randperm(B).to(torch.int32)
        pos = torch.randint(0, S + 8, (B,), dtype=torch.int32)
        pos[3] = -1
        ps = torch.randint(0, P, (B,), dtype=torch.int32)
        pl = torch.minimum(torch.randint(0, S, (B,), dtype=torch.int32), pos.clamp(min=0))
        for window, pre in ((0, False), (24, False), (0, True), (40, True)):
            a = (q, kc, vc, d(pos), d(slot), B, 1, HD ** -0.5, 50.0, window)
            for route, n in (("wave/rows", 0), ("split/rows", 1 << 20)):
                with split_rows(n):
                    emit(route, f"split_bitequal G={G} S={S} window={window} prefix={int(pre)}",
                         ops.attention(*a, prefix=(pk, pv, d(ps), d(pl))) if pre else ops.attention(*a))

    # ---- test_attention_decode_wave_s2048
    for G in (2, 4):
        torch.manual_seed(23)
        Hkv, HD, B, S = 4, 256, 6, 2048
        kc, vc = torch.randn(B, Hkv, S, HD, dtype=BF), torch.randn(B, Hkv, S, HD, dtype=BF)
        q = torch.randn(B, Hkv * G, HD, dtype=BF) * 2
        slot = torch.randperm(B).to(torch.int32)
        pos = torch.tensor([S - 1, S - 2, 1500, 2000, 7, S - 1], dtype=torch.int32)
        for route, n in (("wave/rows", 0), ("split/rows", 1 << 20)):
            with split_rows(n):
                emit(route, f"wave_s2048 G={G}",
                     ops.attention(d(q), d(kc), d(vc), d(pos), d(slot), B, 1, HD ** -0.5, 50.0, 0))

    # ---- test_attention_decode_shared_prefix_buckets (the default split thresholds: 27 and 13 rows run the split kernel
    # at HD = 256)
    for HD in (256, 128):
        torch.manual_seed(11)
        Hkv, G, S, B = 2, 2, 68, 27
        Hq = Hkv * G
        kc, vc = torch.randn(B, Hkv, S, HD, dtype=BF), torch.randn(B, Hkv, S, HD, dtype=BF)
        pk, pv = torch.randn(4, Hkv, S, HD, dtype=BF), torch.randn(4, Hkv, S, HD, dtype=BF)
        slot = torch.randperm(B).to(torch.int32)
        pos = torch.randint(20, S, (B,), dtype=torch.int32)
        ps = torch.randint(0, 4, (B,), dtype=torch.int32)
        pl = torch.minimum(torch.randint(1, 40, (B,), dtype=torch.int32), pos)
        pl[[3, 10]] = 0
        q = torch.randn(B, Hq, HD, dtype=BF) * 2
        for window, nb in ((0, B), (16, B), (0, 13)):
            emit("default/rows", f"prefix_buckets HD={HD} window={window} rows={nb}",
                 ops.attention(d(q[:nb]), d(kc), d(vc), d(pos[:nb]), d(slot[:nb]), nb, 1, HD ** -0.5, 50.0, window,
                               prefix=(d(pk), d(pv), d(ps), d(pl))))

    # ---- test_attention_varlen_shared_prefix
    for G, HD in ((2, 256), (1, 128)):
        torch.manual_seed(15)
        Hkv, S = 2, 96
        Hq = Hkv * G
        kc, vc = torch.randn(5, Hkv, S, HD, dtype=BF), torch.randn(5, Hkv, S, HD, dtype=BF)
        pk, pv = torch.randn(3, Hkv, S, HD, dtype=BF), torch.randn(3, Hkv, S, HD, dtype=BF)
        spec = [(3, 10, 23, 1, 12), (0, 40, 1, 0, 0), (4, 5, 13, 2, 9), (1, 70, 26, 1, 75)]
        pos, slot_rows, seqs = [], [], []
        for sl, p0, n, ps, pl in spec:
            seqs.append((len(pos), n, sl, ps, pl))
            pos += list(range(p0, p0 + n))
            slot_rows += [sl] * n
        M = len(pos)
        pos_t, sr = torch.tensor(pos, dtype=torch.int32), torch.tensor(slot_rows, dtype=torch.int32)
        blk = packed_blocks(seqs, 16 // G)
        q = torch.randn(M, Hq, HD, dtype=BF) * 2
        for window in (0, 16):
            emit("tail/packed", f"varlen_shared_prefix HD={HD} G={G} window={window}",
                 ops.attention_varlen(d(q), d(kc), d(vc), d(pos_t), d(sr), d(blk), HD ** -0.5, 50.0, window,
                                      prefix_kv=(d(pk), d(pv))))


if __name__ == "__main__":
    main()
