"""Launch golden of the GEMM layer (ops/gemm.py over runtime/gemm_dispatch.plan), on the CPU with no extension.

Every in-tree tile gives the same bits, so a wrong launch choice costs speed and no numeric test notices it.  This
test drives the whole launch path -- 16 entry points at the Gemma-2-9B shapes (LoRA columns KP = 128), 14 row counts,
the three ``TB_GEMM`` modes with the shipped table, the ring GEMM reporting its tiles built or not -- with tensors
that claim to be on the GPU and a recording stub in place of the extension, and compares the ordered launches of each
of the 1344 cases with ``tests/golden/gemm_launches.json``.  The golden was recorded from the code before the launch
paths were folded into one plan and one executor (its ``commit`` field), with the same grid and a stub of that code's
binding surface (separate ``*_l2a`` bindings), so equality means the refactor launches exactly what its parent did.

A record is the list of normalised launches: ``["g4", r0, r1, epi, tile_rows, two_source]``, ``["ring", r0, r1, epi,
bm, bn, variant, two_source]``, ``["splitk", rows, epi, tile_rows, ks]``, ``["splitk_part", rows, tile_rows, ks]``,
``["blas"]`` and the trailing ``["rope"]`` / ``["rope_part"]`` / ``["add_rmsnorm2"]`` / ``["add_rmsnorm2_part"]``.
The stub also requires every per-row operand of a launch (x, a2, out, pos, slot_of_row) to cover the same rows.
"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.runtime import gemm_dispatch as GD

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_launches.json")
BF = torch.bfloat16
D, FFN, HQ, HKV, V, KP = 3584, 14336, 16, 8, 256000, 128
SHAPES = {"qkv": (8192, D), "o": (D, 4096), "gu": (2 * FFN, D), "down": (D, FFN), "head": (V, D)}
MS = [1, 16, 48, 64, 192, 300, 512, 1024, 1536, 2048, 4608, 6144, 9000, 32768]


class FakeGpu(torch.Tensor):
    """A storage-less tensor that says it is on the GPU, so the ops take their kernel branches."""

    @property
    def is_cuda(self):
        return True


def fake(*shape, dtype=BF):
    return torch.empty(*shape, dtype=dtype, device="meta").as_subclass(FakeGpu)


def row_range(x, *per_row):
    """``[r0, r1)`` of a launch from its A operand (a row slice of a contiguous tensor); the other per-row operands
    must be the same rows of theirs."""
    k = x.shape[-1]
    n, r0 = x.numel() // k, x.storage_offset() // k
    for t in per_row:
        if t is not None:
            assert t.is_contiguous() and t.numel() % n == 0 and t.storage_offset() == r0 * (t.numel() // n), \
                "per-row operands of one launch cover different rows"
    return [r0, r0 + n]


class Recorder:
    """Stands in for the extension module: the two shape predicates and a recording version of every binding the
    GEMM layer calls."""

    def __init__(self):
        self.log = []
        self.ring_ok = True

    def gemm4_ok(self, M, N, K):
        return M > 0 and N > 0 and N % 256 == 0 and K >= 64 and K % 64 == 0

    def gemm_ring_ok(self, M, N, K, epi, bm, bn, var):
        return self.ring_ok

    def gemm4_splitk_ks(self, M, N, K, tile_rows):
        return 4

    def gemm4(self, A, W, C, bias, thr, epi, tile_rows, a2=None):
        self.log.append(["g4"] + row_range(A, a2, C) + [epi, tile_rows, int(a2 is not None)])

    def gemm_ring(self, A, W, C, epi, bm, bn, var, a2=None):
        self.log.append(["ring"] + row_range(A, a2, C) + [epi, bm, bn, var, int(a2 is not None)])

    def gemm4_qkv_rope(self, x, w, pos, slot, cs, q, kc, vc, Hq, Hkv, tile_rows, a2=None):
        self.log.append(["g4"] + row_range(x, a2, q, pos, slot) + [4, tile_rows, int(a2 is not None)])

    def gemm_ring_qkv_rope(self, x, w, pos, slot, cs, q, kc, vc, Hq, Hkv, bm, bn, var, a2=None):
        self.log.append(["ring"] + row_range(x, a2, q, pos, slot) + [4, bm, bn, var, int(a2 is not None)])

    def gemm4_splitk(self, A, W, C, ws, epi, tile_rows, ks):
        self.log.append(["splitk", A.shape[0], epi, tile_rows, ks])

    def gemm4_splitk_part(self, A, W, ws, tile_rows, ks):
        self.log.append(["splitk_part", A.shape[0], tile_rows, ks])
        return ks

    def add_rmsnorm2_part(self, *a):
        self.log.append(["add_rmsnorm2_part"])

    def add_rmsnorm2(self, *a):
        self.log.append(["add_rmsnorm2"])

    def rope_qkv_cache_part(self, *a):
        self.log.append(["rope_part"])

    def rope_qkv_cache(self, *a):
        self.log.append(["rope"])

    def gemm_nt(self, *a):
        self.log.append(["gemm_nt"])


def install(monkeypatch, rec, modules, workspace_names):
    """Put ``rec`` in place of the extension in ``modules`` and hipBLASLt (``torch.matmul`` / ``F.linear``) behind
    a recording stand-in that returns a GPU-claiming tensor, so the unfused paths continue."""
    for m in modules:
        monkeypatch.setattr(m, "_k", lambda: rec)
        monkeypatch.setattr(m, "rope_cs", lambda c, s: None)
        for name in workspace_names:
            if hasattr(m, name):
                monkeypatch.setattr(m, name, lambda *a: None)

    def matmul(x, wt, out=None):
        rec.log.append(["blas"])
        return out if out is not None else fake(*x.shape[:-1], wt.shape[-1])

    monkeypatch.setattr(torch, "matmul", matmul)
    monkeypatch.setattr(F, "linear", lambda x, w: matmul(x, w.t()))


def record_grid(rec):
    """Run the grid; ``{case name: [launch, ...]}``.  Leaves the dispatch mode as it found it."""
    out = {}

    def run(name, fn):
        rec.log = []
        try:
            fn()
        except Exception as e:       # a path that cannot run is part of the record, not a crash of the recorder
            rec.log.append(["raise", type(e).__name__])
        out[name] = rec.log

    class Spec:
        ffn = FFN

    old = GD.mode()
    try:
        for mode in ("tb", "auto", "blas"):
            GD.set_mode(mode)
            GD.load_table()
            for ring in (True, False):
                rec.ring_ok = ring
                for M in MS:
                    pre = f"{mode}/ring{int(ring)}/M{M}/"
                    pos, h, wn = fake(M, dtype=torch.int32), fake(M, D), fake(D)
                    x, a2 = fake(M, D), fake(M, KP)
                    rope = (pos, pos, None, None, None, None, HQ, HKV, 256)
                    for nm, (N, K) in SHAPES.items():
                        run(pre + f"linear/{nm}", lambda: ops.linear(fake(M, K), fake(N, K)))
                    run(pre + "qkv", lambda: ops.qkv_rope_cache(x, fake(8192, D), *rope))
                    run(pre + "gu_wins", lambda: rec.log.append(["wins", bool(ops.fused_geglu_wins(x, Spec))]))
                    run(pre + "geglu", lambda: ops.gate_up_geglu(x, fake(2 * FFN, D)))
                    run(pre + "o_norm", lambda: ops.linear_add_rmsnorm2(fake(M, 4096), fake(D, 4096), h, wn, wn, 1e-6))
                    run(pre + "down_norm", lambda: ops.linear_add_rmsnorm2(fake(M, FFN), fake(D, FFN), h, wn, wn, 1e-6))
                    run(pre + "qkv_lora", lambda: ops.qkv_rope_cache_lora(x, a2, fake(8192, D + KP), *rope))
                    run(pre + "geglu_lora", lambda: ops.gate_up_geglu_lora(x, a2, fake(2 * FFN, D + KP)))
                    run(pre + "gu_lora", lambda: ops.linear_lora(x, a2, fake(2 * FFN, D + KP)))
                    run(pre + "o_norm_lora", lambda: ops.linear_lora_add_rmsnorm2(
                        fake(M, 4096), a2, fake(D, 4096 + KP), h, wn, wn, 1e-6))
                    run(pre + "down_norm_lora", lambda: ops.linear_lora_add_rmsnorm2(
                        fake(M, FFN), a2, fake(D, FFN + KP), h, wn, wn, 1e-6))
                    run(pre + "sae_enc", lambda: ops.gemm_nt(x, fake(16384, D), 2, None, None))
    finally:
        GD.set_mode(old)
        GD._state["loaded"] = False
    return out


def test_launches_match_parent_golden(monkeypatch):
    from taboo_brittleness_amd.ops import gemm

    golden = json.load(open(GOLDEN))
    want = golden["cases"]
    assert golden["commit"] and len(want) == 1344
    rec = Recorder()
    install(monkeypatch, rec, (ops, gemm), ("_workspace",))
    got = record_grid(rec)
    assert sorted(got) == sorted(want)
    bad = [(k, got[k], want[k]) for k in want if got[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(want)} cases launch differently, e.g. {bad[:5]}"
    kinds = {r[0] for v in want.values() for r in v}
    # (the shipped table never splits the QKV projection over K, so "rope_part" is test_qkv_splitk's below)
    assert kinds == {"g4", "ring", "splitk", "splitk_part", "blas", "rope", "add_rmsnorm2", "add_rmsnorm2_part", "wins"}
    assert any(len([r for r in v if r[0] == "g4"]) == 2 for v in want.values())      # the row split is exercised


def test_qkv_splitk(monkeypatch, tmp_path):
    """A table that splits the QKV projection over K (the shipped one does not): partials, then the RoPE pass that
    sums them; two sources never split (``fill_choice``); a bare-int entry runs as ``g<int>``."""
    from taboo_brittleness_amd.ops import gemm

    rec = Recorder()
    install(monkeypatch, rec, (ops, gemm), ("_workspace",))
    p = tmp_path / "t.json"
    json.dump({"shapes": {f"8192,{D},4": [[64, "k128"], [512, 256]]}}, open(p, "w"))
    old = GD.mode()
    try:
        GD.set_mode("auto")
        GD.load_table(str(p))
        pos = fake(64, dtype=torch.int32)
        ops.qkv_rope_cache(fake(64, D), fake(8192, D), pos, pos, None, None, None, None, HQ, HKV, 256)
        ops.qkv_rope_cache_lora(fake(64, D), fake(64, KP), fake(8192, D + KP), pos, pos, None, None, None, None, HQ,
                                HKV, 256)
        pos = fake(300, dtype=torch.int32)
        ops.qkv_rope_cache(fake(300, D), fake(8192, D), pos, pos, None, None, None, None, HQ, HKV, 256)
        assert rec.log == [["splitk_part", 64, 128, 4], ["rope_part"], ["g4", 0, 64, 4, 128, 1], ["g4", 0, 300, 4, 256, 0]]
    finally:
        GD.set_mode(old)
        GD._state["loaded"] = False


def test_forced_choices(monkeypatch):
    """``tb_gemm`` / ``gemm_l2a`` with a forced choice: every spelling, the ``gs`` split's two launches over matching
    row slices, and the errors."""
    from taboo_brittleness_amd.ops import gemm

    rec = Recorder()
    install(monkeypatch, rec, (ops, gemm), ("_workspace",))
    M, N, K = 2100, 8192, 256
    x, a2, w, w2, c = fake(M, K), fake(M, KP), fake(N, K), fake(N, K + KP), fake(M, N)
    for choice, want in (("g256", [["g4", 0, M, 0, 256, 0]]), (128, [["g4", 0, M, 0, 128, 0]]),
                         ("gs", [["g4", 0, 2048, 0, 256, 0], ["g4", 2048, M, 0, 128, 0]]),
                         ("r64x112b", [["ring", 0, M, 0, 64, 112, 1, 0]]), ("k128", [["splitk", M, 0, 128, 4]])):
        rec.log = []
        ops.tb_gemm(x, w, c, None, None, 0, choice)
        assert rec.log == want, choice
    rec.log = []
    ops.gemm_l2a(x, a2, w2, c, 0, "gs")
    ops.gemm_l2a(x, a2, w2, c, 0, "r64x64b")
    assert rec.log == [["g4", 0, 2048, 0, 256, 1], ["g4", 2048, M, 0, 128, 1], ["ring", 0, M, 0, 64, 64, 1, 1]]
    for bad in (lambda: ops.tb_gemm(x, w, c, None, None, 0, "blas"), lambda: ops.tb_gemm(x, w, c, None, None, 0, "x9"),
                lambda: ops.gemm_l2a(x, a2, w2, c, 0, "k128")):
        with pytest.raises(ValueError):
            bad()
