"""The 256-row gemm4 tile as one K-tile stream per workgroup (csrc/gemm4.hip ``PIPE``): the last two periods of an
output tile stage the next tile's first two K tiles, so a tile ends in an ordinary period.  Every accumulator's K chain
is the plain tile loop's, so the outputs must be BIT-identical to it (``gemm4_set_pipe(0)``), to the rows computed
alone, and within bf16 rounding of a float32 reference.

Shapes: M = 6437 (25 full row tiles + 37 rows) x N = 8192 is 832 output tiles, 3-4 consecutive tiles per workgroup
on 256 CUs with a partial last row tile; K = 64 and 128 (one and two K tiles: the plain loop is dispatched, the
stream needs three), 192 (the first streamed size: no main-loop period, an odd number of K tiles, so the stage parity
flips per tile), 256 (one main-loop period, even) and the model's 3584.  M = 300 x N = 512 is one tile per workgroup
(no successor anywhere)."""
import pytest
import torch

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HQ, HKV, HD, S, MAXP = 16, 8, 256, 8, 64


def _operands(gpu, M, N, K, seed=21):
    g = torch.Generator(device=gpu)
    g.manual_seed(seed)
    A = (torch.rand(M, K, device=gpu, generator=g) * 2 - 1).to(BF)
    W = (torch.rand(N, K, device=gpu, generator=g) * 2 - 1).to(BF)
    return A, W


def _run_all(k, gpu, A, W, epis):
    """{name: tensor} of every output of the given epilogues with the current tile loop."""
    M, K = A.shape
    N = W.shape[0]
    out = {}
    if 0 in epis:
        c = torch.full((M, N), float("nan"), device=gpu, dtype=BF)
        k.gemm4(A, W, c, None, None, 0, 256)
        out["bf16"] = c
    if 3 in epis:
        Wi = W[ops.geglu_interleave_index(N // 2, gpu)].contiguous()
        act = torch.full((M, N // 2), float("nan"), device=gpu, dtype=BF)
        k.gemm4(A, Wi, act, None, None, 3, 256)
        out["geglu"] = act
    if 6 in epis:
        logits = torch.full((M, N), float("nan"), device=gpu, dtype=BF)
        part = torch.zeros(ops.head_part_numel(M, N), device=gpu)
        lse = torch.full((M,), float("nan"), device=gpu)
        k.lens_gemm(A, W, logits, part, lse)
        out["lens_logits"], out["lens_part"], out["lens_lse"] = logits, part[: M * (N // 128) * 4].clone(), lse
    if 4 in epis:
        assert N == (HQ + 2 * HKV) * HD
        g = torch.Generator(device=gpu)
        g.manual_seed(3)
        pos = torch.randint(0, S + 3, (M,), device=gpu, generator=g, dtype=torch.int32)
        pos[::17] = -1
        slot = torch.randperm(M, device=gpu, generator=g).to(torch.int32)
        inv = 1.0 / (10000.0 ** (torch.arange(0, HD, 2).float() / HD))
        ang = torch.arange(MAXP).float()[:, None] * inv[None]
        cs = ops.rope_cs(ang.cos().to(gpu), ang.sin().to(gpu))
        q = torch.full((M, HQ, HD), 7.0, device=gpu, dtype=BF)
        kc = torch.full((M, HKV, S, HD), 3.0, device=gpu, dtype=BF)
        vc = torch.full((M, HKV, S, HD), 5.0, device=gpu, dtype=BF)
        k.gemm4_qkv_rope(A, W, pos, slot, cs, q, kc, vc, HQ, HKV, 256)
        out["rope_q"], out["rope_k"], out["rope_v"] = q, kc, vc
    return out


def _old_and_new(k, gpu, A, W, epis):
    try:
        k.gemm4_set_pipe(0)
        old = _run_all(k, gpu, A, W, epis)
    finally:
        k.gemm4_set_pipe(1)
    return old, _run_all(k, gpu, A, W, epis)


@pytest.mark.parametrize("M,N,K", [(6437, 8192, 64), (6437, 8192, 128), (6437, 8192, 192), (6437, 8192, 256),
                                   (6437, 8192, 3584), (300, 512, 128), (300, 512, 320)])
def test_stream_bitequal_plain_tile_loop(gpu, M, N, K):
    """EPI 0 / 3 / 6 (and 4 where N is the QKV width): raw bits of the streamed tile loop == the plain one."""
    k = ops._k()
    A, W = _operands(gpu, M, N, K)
    epis = (0, 3, 6, 4) if N == (HQ + 2 * HKV) * HD else (0, 3, 6)
    old, new = _old_and_new(k, gpu, A, W, epis)
    assert sorted(old) == sorted(new)
    for name in old:
        assert not torch.isnan(old[name].float()).any(), name          # every element was written
        assert torch.equal(old[name].view(torch.int16) if old[name].dtype == BF else old[name].view(torch.int32),
                           new[name].view(torch.int16) if new[name].dtype == BF else new[name].view(torch.int32)), name
    if 4 in epis:
        assert (new["rope_k"] != 3.0).any() and (new["rope_v"] != 5.0).any()   # the caches were written


def test_stream_vs_float32_reference(gpu):
    """The streamed loop at the model's K against a float32 GEMM of the same bf16 operands (ops/reference.py for the
    GeGLU), with test_gemm4_epilogues' tolerances."""
    M, N, K = 6437, 8192, 3584
    k = ops._k()
    A, W = _operands(gpu, M, N, K)
    new = _run_all(k, gpu, A, W, (0, 3, 6))
    r = A.float() @ W.float().T
    err = (new["bf16"].float() - r).abs()
    assert (err <= 1e-2 * K ** 0.5 + 1e-2 * r.abs()).all(), err.max().item()
    assert torch.equal(new["lens_logits"], new["bf16"])
    lse = torch.logsumexp(new["lens_logits"].float(), dim=-1)
    assert (new["lens_lse"] - lse).abs().max().item() < 1e-3
    want = ref.geglu(r.to(BF)).float()
    err = (new["geglu"].float() - want).abs()
    assert (err <= 2e-2 * K ** 0.5 + 2e-2 * want.abs()).all(), err.max().item()


def test_stream_batch_invariant(gpu):
    """Rows 0..255 of the M = 6437 call (the first of several tiles its workgroup streams) == the same rows alone."""
    M, N, K = 6437, 8192, 3584
    k = ops._k()
    A, W = _operands(gpu, M, N, K)
    full = _run_all(k, gpu, A, W, (0, 3))
    sub = _run_all(k, gpu, A[:256].contiguous(), W, (0, 3))
    for name in sub:
        assert torch.equal(sub[name].view(torch.int16), full[name][:256].view(torch.int16)), name
