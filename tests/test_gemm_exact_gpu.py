"""The in-tree MFMA GEMMs -- csrc/gemm4.hip (256 / 128 / 64-row tiles, the streamed and the plain K loop, split-K,
two-source A, the JumpReLU / GeGLU / RoPE / head / lens epilogues), csrc/gemm_ring.hip (every tile and ring variant,
``lora_t``) and ``gemm_nt`` in csrc/sae.hip -- held to exact results on integer-valued operands (criteria, cases and
runners: tests/gemm_cases.py, checked against themselves in tests/test_gemm_exact_cpu.py).  The expectations come
from float64 and never from an in-tree kernel: fp32 stores and split-K planes equal the exact value, bf16 stores its
single round-to-nearest-even as bits, fused epilogues the pinned elementwise op of that rounded tensor, with nothing
masked out; every output sits in front of sentinel guard rows.  Every test prints what it checked.

Seen on an MI355X: no output, guard cell or split count was ever off.  gemm4: 96 launches per K, among their outputs
169 353 (K = 64) to 344 649 (K = 320) bf16 ties, all rounded to even, and 15 066 to 35 898 JumpReLU inputs equal to
their threshold, all zeroed.  Several tiles per workgroup: 288 tiles on 256 compute units, the lens log-sum-exp within
0.045 of its bound.  Two sources: 6 gemm4 and 31 ring launches per shape.  Split-K: 297 partial planes at K = 640 and
126 at K = 3584, each the exact sum over its own K range.  Ring: 93 tile / variant combinations over the three M at
K = 128, 384 and 1152 and 102 at K = 512 and 3584 (epilogue 0), 60 and 66 (GeGLU, RoPE), up to 907 680 ties per test.
gemm_nt: 3 045 to 5 059 inputs on their threshold per K.  lora_t: 66 launches per K, about 515 000 masked cells read
back as +0.  Head and lens: every planted tie resolved to the lower index under both caps, NLLs within 0.08 of the
bound.  gemm_ring refused 303 tile / variant / shape combinations.  Accumulation width: all 33 024 outputs of the
``tall`` case lie in [2^23, 2^24) and came back exact from every kernel: the bf16 MFMA, the K loops and the split-K
reduction keep 24 significant bits.  Uniform operands: fp32 stores used 0.008 of ``gamma S`` or less, bf16 stores 0.93
to 0.99 of their bound, which is almost all the half step of the result."""
from types import SimpleNamespace

import pytest
import torch

import gemm_cases as gc
from taboo_brittleness_amd import ops
from taboo_brittleness_amd.runtime import gemm_dispatch as GD

pytestmark = pytest.mark.gpu


def _impl():
    k = ops._k()

    def qkv_rope(family, tile, A, W, pos, slot, cos, sin, q, kc, vc, Hq, Hkv, a2=None):
        cs = ops.rope_cs(cos, sin)
        if family == "g4":
            k.gemm4_qkv_rope(A, W, pos, slot, cs, q, kc, vc, Hq, Hkv, tile, a2)
        else:
            k.gemm_ring_qkv_rope(A, W, pos, slot, cs, q, kc, vc, Hq, Hkv, *tile, a2)

    def lens(x, W, logits, lse):
        ops.lens_unembed(x, W, fused=True, out=logits, lse_out=lse)

    def head(x, W, cap, tgt, nxt, nll_self, nll_tgt):
        ops.vocab_head(x, W, cap, tgt, nxt=nxt, nll_self=nll_self, nll_tgt=nll_tgt, fused=True)

    def run_rows(A, W, out, epi, r0, r1, tile):
        ops.run_plan((GD.Launch("g4", r0, r1, tile),), A, W, out, epi)

    return SimpleNamespace(
        gemm4=k.gemm4, gemm_ring=k.gemm_ring, gemm_nt=k.gemm_nt, splitk_part=k.gemm4_splitk_part, splitk=k.gemm4_splitk,
        splitk_ks=k.gemm4_splitk_ks, qkv_rope=qkv_rope, lora_t=k.lora_t, lens=lens, head=head, tb_gemm=ops.tb_gemm,
        run_rows=run_rows, ring_tiles=k.gemm_ring_tiles, ring_ok=k.gemm_ring_ok, lora_t_ok=k.lora_t_ok,
        set_pipe=k.gemm4_set_pipe)


@pytest.mark.parametrize("K", gc.G4_KS)
def test_gemm4_exact(gpu, K):
    """Epilogues 0 / 1 / 2 / 3 on 256-row tiles (plain and streamed K loop) and 128-row tiles, every M of
    ``G4_MS`` with N alternating between 256 and 512, all three integer classes up to K = 320 and ``wide`` at 3584;
    JumpReLU thresholds sit on attained values and nothing is masked.  Seen: 96 launches per K, 0 mismatches;
    169 353 to 344 649 ties rounded to even and 15 066 to 35 898 inputs on their threshold zeroed per K."""
    gc.run_gemm4(_impl(), gpu, K).assert_ok(f"K {K}")


@pytest.mark.parametrize("K", gc.MANY_KS)
def test_gemm4_several_tiles_per_workgroup(gpu, K):
    """M = 4400, N = 4096: 288 tiles of 256 x 256, more than the device has compute units, so a persistent workgroup
    runs several tiles: epilogues 0 and 3, the fused RoPE (Hq = 8, Hkv = 4) and the lens epilogue, both tile heights,
    against one float64 product computed on the device.  Seen: 0 mismatches, lse within 0.045 of its bound."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    gc.run_many(_impl(), gpu, K, cus=cus).assert_ok(f"K {K}")


@pytest.mark.parametrize("k0,K", gc.L2A_SHAPES)
def test_two_source_exact(gpu, k0, K):
    """``[x | a2]`` from two tensors: gemm4 at both tile heights and every ring tile with variant 1; epilogues 0, 3 and
    the fused RoPE.  Seen: 6 gemm4 and 31 ring launches per shape, 0 mismatches."""
    gc.run_two_source(_impl(), gpu, k0, K).assert_ok(f"k0 {k0} K {K}")


@pytest.mark.parametrize("K,splits", [(640, gc.SPLIT_KS), (3584, (0,))])
def test_splitk_exact(gpu, K, splits):
    """Tiles 64 / 128 / 256 at M = 1, 65, 300: the split count returned is the ceil formula's, each fp32 partial
    plane equals the exact sum over its own K range, the reduced bf16 and GeGLU outputs equal the exact expectation
    and -- on integer data -- the unsplit kernel bit for bit, and nothing is written behind the last plane.  Seen: 297
    planes at K = 640, 126 at K = 3584, all exact."""
    gc.run_splitk(_impl(), gpu, K, splits).assert_ok(f"K {K}")


@pytest.mark.parametrize("K", gc.RING_KS)
@pytest.mark.parametrize("epi", [0, 3, 4])
def test_ring_exact(gpu, epi, K):
    """Every ring tile x variant the launcher admits -- the documented set, counted -- at M = 1, 17, 130: epilogue 0
    at N = 896 (every bn divides it, 112 included), GeGLU at N = 256, RoPE at N = 1024.  Seen: 93 or 102 combinations
    per K over the three M (epilogue 0), 60 or 66 (GeGLU, RoPE), 0 mismatches."""
    gc.run_ring(_impl(), gpu, epi, K).assert_ok(f"epi {epi} K {K}")


@pytest.mark.parametrize("K", gc.NT_KS)
def test_gemm_nt_exact(gpu, K):
    """Epilogues 0 / 1 / 2 at M = 1, 129, 257 and N = 1, 130, 200, 256; K = 32, 96 and 160 end in the zero-filled
    half tile.  Seen: 0 mismatches; 3 045 to 5 059 inputs on their threshold per K."""
    gc.run_gemm_nt(_impl(), gpu, K).assert_ok(f"K {K}")


@pytest.mark.parametrize("K", gc.LORA_KS)
def test_lora_t_exact(gpu, K):
    """Every ``lora_t`` tile at N = 192 into a 224-column T, unsplit and split over 1 / 1 / 5 / 2 chunks, adapters
    -1 .. 3, ``nsr`` = 176: masked columns exactly +0, owned columns ``rn_bf16(exact)``, guards untouched.  Seen: 66
    launches per K, 0 mismatches."""
    gc.run_lora_t(_impl(), gpu, K).assert_ok(f"K {K}")


@pytest.mark.parametrize("M", gc.HEAD_MS)
def test_head_and_lens_exact(gpu, M):
    """V = 1024, K = 192, logits times 2^-3, duplicated W rows inside a 128-column slice, across slices, across the
    256-column tile boundary and at V - 1: the fused head's token is the lowest index among the maxima under cap 30
    and without a cap, its NLLs and the lens log-sum-exp lie within ``lse_bound``, the lens logits are exact.  Seen:
    every planted tie went to the lower index; NLLs within 0.08 of the bound."""
    gc.run_head_lens(_impl(), gpu, M).assert_ok(f"M {M}")


def test_dispatch_exact(gpu):
    """``ops.tb_gemm`` under "g256", "g128", "gs", "k256", "k128" at (777, 512, 192) and under two ring choices at
    K = 256 (the ring GEMM takes no K = 192, which the last lines check), then each launch of a forced two-launch row
    split alone, the rows outside its slice being its guard rows.  Seen: 0 mismatches under all nine choices and both
    launches."""
    gc.run_dispatch(_impl(), gpu).assert_ok("dispatch")
    c = gc.case("wide", *gc.DISPATCH_SHAPE)
    with pytest.raises(RuntimeError):
        ops.tb_gemm(c.A.to(gpu), c.W.to(gpu), torch.empty(777, 512, dtype=gc.BF, device=gpu), None, None, 0, "r64x64")


def test_host_checks(gpu):
    """``gemm4``, ``gemm4_splitk``, ``lens_gemm`` and ``head_fused`` raise on N % 256 != 0, K = 32 and K % 64 != 0,
    ``gemm_ring`` wherever ``gemm_ring_ok`` is false, and two sources on k0 % 128 != 0.  Seen: 303 ring
    combinations refused."""
    k = ops._k()
    M = 8

    def bf(*shape):
        return torch.zeros(*shape, dtype=gc.BF, device=gpu)

    def f32(*shape):
        return torch.zeros(*shape, device=gpu)

    for N, K in ((128, 64), (384, 128), (256, 32), (256, 96), (256, 160)):
        x, w = bf(M, K), bf(N, K)
        with pytest.raises(RuntimeError):
            k.gemm4(x, w, bf(M, N), None, None, 0, 128, None)
        with pytest.raises(RuntimeError):
            k.gemm4_splitk(x, w, bf(M, N), f32(4 * M * N), 0, 128, 2)
        with pytest.raises(RuntimeError):
            k.lens_gemm(x, w, bf(M, N), f32(M * 4 * 4), f32(M))
        with pytest.raises(RuntimeError):
            k.head_fused(x, w, f32(M * 4 * 4), 0.0, None, None, torch.zeros(M, dtype=torch.int32, device=gpu), f32(M),
                         None)
    n = 0
    for N, K in ((896, 192), (896, 64), (200, 256), (896, 256)):
        x, w = bf(M, K), bf(N, K)
        for bm, bn in list(k.gemm_ring_tiles(0)) + [(24, 24)]:
            for var in (0, 1, 2, 3):
                if not k.gemm_ring_ok(M, N, K, 0, bm, bn, var):
                    with pytest.raises(RuntimeError):
                        k.gemm_ring(x, w, bf(M, N), 0, bm, bn, var, None)
                    n += 1
    print(f"gemm_ring refused {n} tile / variant / shape combinations")
    assert n >= 200
    for k0, K in ((64, 256), (192, 384), (128, 192)):
        x, a2, w = bf(M, k0), bf(M, K - k0), bf(256, K)
        with pytest.raises(RuntimeError):
            k.gemm4(x, w, bf(M, 256), None, None, 0, 128, a2)
        with pytest.raises(RuntimeError):
            k.gemm_ring(x, w, bf(M, 256), 0, 64, 64, 1, a2)


def test_accumulation_width(gpu):
    """Positive operands 64 .. 127 at K = 1024: outputs in [2^22, 2^24), half of them odd, which only an accumulation
    of 24 significant bits from the first MFMA to the store returns exactly -- the assumption the integer classes rest
    on, measured: gemm4 (fp32, JumpReLU and bf16 stores, split-K planes and reduction), ``gemm_nt`` and three ring
    tiles.  Seen: all 33 024 outputs, every one in [2^23, 2^24), exact from every kernel."""
    gc.run_width(_impl(), gpu).assert_ok("tall")


@pytest.mark.parametrize("K", gc.UNI_KS + gc.UNI_RING_KS)
def test_uniform_operands_within_gamma_s(gpu, K):
    """Uniform (-1, 1) operands: gemm4 (both tiles) and ``gemm_nt`` at K = 64, 192, 320, one ring tile per variant
    at K = 128 and 256 (the ring takes multiples of 128 only); fp32 stores within ``gamma S``, bf16 stores within that
    plus half a bf16 step.  Seen: fp32 within 0.008 of the bound, bf16 within 0.99 (the half step itself)."""
    gc.run_uniform(_impl(), gpu, K).assert_ok(f"K {K}")
