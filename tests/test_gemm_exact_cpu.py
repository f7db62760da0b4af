"""The criteria of tests/test_gemm_exact_gpu.py, checked against themselves on the CPU (tests/gemm_cases.py): first the
property they rest on -- on the integer operand classes a float32 accumulation chain in any order equals the int64
product; then the builders' own conditions (S_max, thresholds on attained values, gate spread, planted ties), from the
reference alone; then the float64 reference passes every runner; last, every runner rejects the planted defect it is
there to catch."""
import pytest
import torch

import gemm_cases as gc

CPU = torch.device("cpu")


# ---- the property ----------------------------------------------------------------------------------------------------
def _chain32(A, W, order, block, splits=1):
    """float32 accumulation of ``A @ W^T``: K visited in ``order``, ``block`` columns per float32 partial product, the
    blocks added one after the other; with ``splits`` > 1 each contiguous share of the blocks is summed on its own
    and the shares are added last."""
    a, w = A.float()[:, order], W.float()[:, order]
    K = a.shape[1]
    blocks = [slice(k, k + block) for k in range(0, K, block)]
    per = -(-len(blocks) // splits)
    total = torch.zeros(A.shape[0], W.shape[0])
    for s in range(0, len(blocks), per):
        part = torch.zeros_like(total)
        for b in blocks[s:s + per]:
            part = part + a[:, b] @ w[:, b].t()
        total = total + part
    return total


@pytest.mark.parametrize("cls,M,N,K", [("wide", 40, 64, 14336), ("scaled", 40, 64, 14336), ("small", 300, 512, 320),
                                       ("wide", 300, 256, 3584), ("scaled", 129, 256, 192)])
def test_any_float32_order_is_exact(cls, M, N, K):
    """Shuffled, 32-blocked and K-split float32 chains all equal the int64 product (times the outputs' powers of two),
    and so does the float64 matmul the expectations are taken from."""
    op = gc.operands(cls, M, N, K)
    exact = torch.ldexp((op.ai @ op.wi.t()).double(), op.ea[:, None] + op.fw[None, :])
    assert gc.s_max(op) < 2 ** 24
    assert torch.equal(gc.exact(op.A, op.W), exact)
    g = torch.Generator().manual_seed(K)
    for order, block, splits in ((torch.arange(K), 32, 1), (torch.randperm(K, generator=g), 32, 1),
                                 (torch.randperm(K, generator=g), 1 if K <= 320 else 7, 1), (torch.arange(K), 64, 7)):
        assert torch.equal(_chain32(op.A, op.W, order, block, splits).double(), exact), (block, splits)


def test_s_max_at_the_deepest_k():
    """K = 14336 with h = 8 stays 50x below 2^24."""
    s = gc.s_max(gc.operands("wide", 64, 64, 14336))
    print(f"S_max at K = 14336, h = 8: {s}")
    assert s < 2 ** 24 // 50


def test_one_dropped_term_shows_in_almost_every_output():
    """Dropping one k term changes every fp32 output and most bf16 outputs."""
    op = gc.operands("wide", 300, 512, 3584)
    E = gc.exact(op.A, op.W)
    D = E - op.A.double()[:, -1:] * op.W.double()[:, -1:].t()
    assert bool((D != E).all())
    frac = float((gc.rn_bf16(D).view(torch.int16) != gc.rn_bf16(E).view(torch.int16)).float().mean())
    print(f"bf16 outputs changed by one dropped term at K = 3584: {frac:.3f}")
    assert frac > 0.5
    c = gc.case("small", 257, 512, 320)
    assert bool(gc.bf16_lossless(c.E).all())                         # class small at K <= 320: every defect shows


# ---- the builders' conditions ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", gc.G4_KS)
def test_builder_conditions(K):
    """Seven columns of eight have their threshold attained (1000 times or more over a ``small`` case of 255 rows or
    more); a tenth or more of the outputs of a ``wide`` case are bf16 ties; the ``small`` GeGLU cases of 255 rows or
    more hold 1000 gates in [-10, -3] and reach past both saturated ends."""
    classes = set()
    for cls, M, N in gc.g4_cases(K):
        c = gc.case(cls, M, N, K)
        classes.add(cls)
        assert c.n_eq >= N - N // 8
        if cls == "small" and M >= 255:
            print(f"K {K} M {M} N {N}: pre == thr at {c.n_eq} outputs")
            assert c.n_eq >= 1000
        if cls == "wide" and M >= 127 and K >= 128:
            print(f"K {K} M {M} N {N}: {c.n_ties} bf16 ties ({c.n_ties / (M * N):.3f})")
            assert c.n_ties >= M * N // 10
        g = gc.gate_case(cls, M, N, K)
        if cls == "small" and M >= 255:
            print(f"K {K} M {M} N {N}: {g.tail} gates in [-10, -3], range [{g.gmin}, {g.gmax}]")
            assert g.tail >= 1000 and g.gmin < -10 and g.gmax > 10
    assert classes == ({"wide"} if K > 320 else set(gc.CLASSES))


def test_case_tables_cover_what_they_claim():
    for M in gc.G4_MS:                                               # every M meets every class at some K <= 320
        assert {cls for K in gc.G4_KS[:5] for cls, m, _n in gc.g4_cases(K) if m == M} == set(gc.CLASSES)
    assert gc.many_tiles(gc.MANY_M, gc.MANY_N) == 288
    assert [gc.split_count(640, ks) for ks in gc.SPLIT_KS] == [(1, 10), (3, 4), (4, 3), (5, 2), (10, 1), (10, 1)]
    assert [gc.lora_chunks(K) for K in gc.LORA_KS] == [1, 1, 5, 2]
    assert len(gc.LORA_TILES) == 11
    assert all(gc.RING_N[0] % bn == 0 for _bm, bn in gc.RING_PLAIN + gc.RING_N112)
    assert [len(gc.ring_admitted(0, 896, K)) for K in gc.RING_KS] == [31, 31, 34, 31, 34]
    rr = gc.rope_rows(300)
    assert {rr.S, rr.T - 1, rr.T, rr.T + 17, -1, 0, rr.S - 1} <= set(rr.pos.tolist())
    for M in gc.HEAD_MS:
        gc.head_case(M)                                              # asserts its planted ties


def test_packs():
    """The two wrong packs differ from round-to-nearest-even exactly where they should."""
    x = torch.tensor([1.0, 257.0, 258.0, 259.0, 261.0, -257.0, -259.0, 1.00390625, 3.0e38])
    rn, tr, aw = gc.rn_bf16(x.double()).float(), gc.pack_trunc(x.double()).float(), gc.pack_away(x.double()).float()
    assert rn.tolist()[:7] == [1.0, 256.0, 258.0, 260.0, 260.0, -256.0, -260.0]
    assert tr.tolist()[:7] == [1.0, 256.0, 258.0, 258.0, 260.0, -256.0, -258.0]
    assert aw.tolist()[:7] == [1.0, 258.0, 258.0, 260.0, 262.0, -258.0, -260.0]
    assert rn[7] == 1.0 and tr[7] == 1.0 and aw[7] == 1.0078125
    assert gc.bf16_ties(x.double()).tolist() == [False, True, False, True, True, True, True, True, False]


# ---- the reference passes every runner -------------------------------------------------------------------------------
@pytest.mark.parametrize("K", gc.G4_KS)
def test_reference_gemm4(K):
    gc.run_gemm4(gc.RefImpl(), CPU, K).assert_ok(f"reference K {K}")


def test_reference_many_tiles():
    gc.run_many(gc.RefImpl(), CPU, 192, cus=256).assert_ok("reference")


@pytest.mark.parametrize("k0,K", gc.L2A_SHAPES)
def test_reference_two_source(k0, K):
    gc.run_two_source(gc.RefImpl(), CPU, k0, K).assert_ok("reference")


def test_reference_splitk():
    gc.run_splitk(gc.RefImpl(), CPU, 640, gc.SPLIT_KS).assert_ok("reference K 640")
    gc.run_splitk(gc.RefImpl(), CPU, 3584, (0,), tiles=(128,)).assert_ok("reference K 3584")


@pytest.mark.parametrize("epi", [0, 3, 4])
def test_reference_ring(epi):
    for K in gc.RING_KS[:4]:
        gc.run_ring(gc.RefImpl(), CPU, epi, K).assert_ok(f"reference epi {epi} K {K}")
    gc.run_ring(gc.RefImpl(), CPU, epi, 3584, Ms=(17,)).assert_ok(f"reference epi {epi} K 3584")


@pytest.mark.parametrize("K", gc.NT_KS)
def test_reference_gemm_nt(K):
    gc.run_gemm_nt(gc.RefImpl(), CPU, K).assert_ok(f"reference K {K}")


@pytest.mark.parametrize("K", gc.LORA_KS)
def test_reference_lora_t(K):
    gc.run_lora_t(gc.RefImpl(), CPU, K).assert_ok(f"reference K {K}")


@pytest.mark.parametrize("M", gc.HEAD_MS)
def test_reference_head_lens(M):
    gc.run_head_lens(gc.RefImpl(), CPU, M).assert_ok(f"reference M {M}")


def test_reference_dispatch_and_uniform():
    gc.run_dispatch(gc.RefImpl(), CPU).assert_ok("reference")
    for K in gc.UNI_KS + gc.UNI_RING_KS:
        gc.run_uniform(gc.RefImpl(), CPU, K).assert_ok(f"reference uniform K {K}")


def test_reference_width_and_narrow_accumulator():
    """The reference passes ``run_width``; an accumulator of 23 significant bits fails its fp32 stores and one of 21 its
    split-K planes -- while one of 20 bits passes the ``wide`` class at K = 3584, whose sums need 18: the exactness of
    the other classes says nothing about the last bits of the accumulator, which is why ``tall`` exists."""
    gc.run_width(gc.RefImpl(), CPU).assert_ok("reference")
    rep = gc.run_width(gc.RefImpl(acc_bits=23), CPU)
    for what in ("gemm4 epi 1", "gemm4 epi 2", "gemm_nt epi 1"):
        assert rep.failed(what), what
    rep = gc.run_width(gc.RefImpl(acc_bits=21), CPU)                 # a plane holds a quarter of K: 22 bits
    assert rep.failed("split-K planes")
    assert not gc.run_gemm4(gc.RefImpl(acc_bits=20), CPU, 3584, [("wide", 129, 256)], epis=(0, 1)).failures


# ---- every planted defect is rejected --------------------------------------------------------------------------------
SMALL = [("small", 129, 256)]
WIDE = [("wide", 129, 256)]


def _g4(K, cases=SMALL, launches=((128, 1),), epis=(0, 1, 2, 3), **mut):
    return gc.run_gemm4(gc.RefImpl(**mut), CPU, K, cases, launches, epis)


def test_mutant_one_term_dropped():
    """One k term of one element: one output of the bf16, fp32 and GeGLU stores differs (the JumpReLU store only if
    that element passes its threshold)."""
    rep = _g4(128, drop_term=True)
    assert all(rep.failed(f"gemm4 epi {e}", ": 1 of") for e in (0, 1, 3))
    assert gc.run_gemm_nt(gc.RefImpl(drop_term=True), CPU, 96, Ms=(129,), Ns=(130,)).failed("gemm_nt epi 1", ": 1 of")
    assert gc.run_ring(gc.RefImpl(drop_term=True), CPU, 0, 384, Ms=(17,)).failed("ring epi 0", ": 1 of")


def test_mutant_last_k_tile_dropped_on_the_ragged_row_tile():
    rep = _g4(192, drop_last_ktile=True)
    assert rep.failed("gemm4 epi 1", "first at (128,") and rep.failed("gemm4 epi 0", "first at (128,")
    assert not _g4(192, [("small", 128, 256)], drop_last_ktile=True).failures       # no ragged tile: nothing wrong
    assert gc.run_ring(gc.RefImpl(drop_last_ktile=True), CPU, 0, 384, Ms=(17,)).failed("ring epi 0")


def test_mutant_k_chunks_swapped_in_a():
    for epi in (0, 1, 2, 3):
        assert _g4(64, swap_chunks=True).failed(f"gemm4 epi {epi}")
    assert gc.run_two_source(gc.RefImpl(swap_chunks=True), CPU, 128, 256).failed("two-source rope")


def test_mutant_output_shifted_one_column():
    rep = _g4(64, shift_col=True)
    assert rep.failed("gemm4 epi 0") and rep.failed("gemm4 epi 1")
    assert gc.run_gemm_nt(gc.RefImpl(shift_col=True), CPU, 32, Ms=(1,), Ns=(130,)).failed("gemm_nt epi 0")
    assert gc.run_lora_t(gc.RefImpl(shift_col=True), CPU, 640, Ms=(130,)).failed("lora_t")


def test_mutant_accumulator_sub_block_transposed():
    rep = _g4(64, transpose4=True)
    assert rep.failed("gemm4 epi 0") and rep.failed("gemm4 epi 1") and rep.failed("gemm4 epi 3")


@pytest.mark.parametrize("pack", ["trunc", "away"])
def test_mutant_bf16_pack(pack):
    """Neither wrong pack shows on the lossless ``small`` class; both do wherever ``wide`` outputs round."""
    assert not _g4(128, epis=(0,), pack=pack).failures
    rep = _g4(3584, WIDE, epis=(0, 3), pack=pack)
    assert rep.failed("gemm4 epi 0") and rep.failed("gemm4 epi 3")
    assert gc.run_ring(gc.RefImpl(pack=pack), CPU, 0, 3584, Ms=(17,)).failed("ring epi 0")
    assert gc.run_lora_t(gc.RefImpl(pack=pack), CPU, 1024, Ms=(130,)).failures


def test_mutant_jumprelu_greater_or_equal():
    rep = _g4(128, jump_ge=True)
    assert rep.failed("gemm4 epi 2") and not rep.failed("gemm4 epi 1")
    assert gc.run_gemm_nt(gc.RefImpl(jump_ge=True), CPU, 96, Ms=(1,), Ns=(1, 130)).failed("gemm_nt epi 2")


def test_mutant_accumulators_not_cleared_between_tiles():
    """12 tiles on 8 workgroups: tiles 8 .. 11 start from tiles 0 .. 3."""
    args = dict(M=600, N=1024, Hq=2, Hkv=1, cus=8)
    gc.run_many(gc.RefImpl(), CPU, 192, **args).assert_ok("reference, 12 tiles")
    rep = gc.run_many(gc.RefImpl(stale_grid=8), CPU, 192, **args)
    for what in ("gemm4 epi 0", "gemm4 epi 3", "gemm4 rope", "lens logits", "lens lse"):
        assert rep.failed(what), what
    with pytest.raises(AssertionError, match="do not exceed"):
        gc.run_many(gc.RefImpl(), CPU, 192, M=600, N=1024, Hq=2, Hkv=1, cus=12)


def test_mutant_k_tile_counted_in_two_splits():
    rep = gc.run_splitk(gc.RefImpl(double_ktile=True), CPU, 640, (1, 4), Ms=(65,), tiles=(128,))
    assert rep.failed("split-K planes", "ks 4") and rep.failed("split-K reduced epi 0", "ks 4")
    assert rep.failed("differs from the unsplit kernel") and not rep.failed("ks 1")


def test_mutant_split_count():
    class Off(gc.RefImpl):
        def splitk_part(self, A, W, ws, tile, ks):
            return super().splitk_part(A, W, ws, tile, ks) + 1

    assert gc.run_splitk(Off(), CPU, 640, (7,), Ms=(1,), tiles=(64,)).failed("split count")


def test_mutant_write_into_a_guard_row():
    rep = _g4(64, guard_write=True)
    assert all(rep.failed(f"gemm4 epi {e}", "guard") for e in (0, 1, 2, 3))
    assert not rep.failed("outputs differ")


def test_mutant_unwritten_cell():
    class Skip(gc.RefImpl):
        def _store(self, C, val):
            keep = C[-1, -1].clone()
            super()._store(C, val)
            C[-1, -1] = keep

    assert _g4(64, [("small", 1, 256)], launches=((256, 0),)).failures == []
    rep = gc.run_gemm4(Skip(), CPU, 64, [("small", 1, 256)], ((256, 0),))
    assert all(rep.failed(f"gemm4 epi {e}", "1 of") for e in (0, 1, 2, 3))


@pytest.mark.parametrize("M", gc.HEAD_MS)
def test_mutant_highest_index_tie_break(M):
    rep = gc.run_head_lens(gc.RefImpl(tie_high=True), CPU, M)
    assert rep.failed("head nxt", "cap 30") and rep.failed("head nxt", "cap 0")
    assert not rep.failed("nll") and not rep.failed("lens")


def test_mutant_row_split_writes_outside_its_rows():
    class Wide(gc.RefImpl):
        def run_rows(self, A, W, out, epi, r0, r1, tile):
            super().run_rows(A, W, out, epi, r0, min(r1 + 1, A.shape[0]), tile)

    rep = gc.run_dispatch(Wide(), CPU)
    assert rep.failed("row split [0, 512)") and not rep.failed("tb_gemm")


def test_the_tolerances_replaced_let_a_dropped_k_tile_through():
    """``atol = 2e-2 sqrt(K)`` on split-K data (uniform (-0.5, 0.5), K = 3584) accepts most outputs of a GEMM that
    drops a whole 64-deep K tile; the exact criterion rejects all of them."""
    g = torch.Generator().manual_seed(9)
    A = ((torch.rand(64, 3584, generator=g) * 2 - 1) * 0.5).to(gc.BF).double()
    W = ((torch.rand(256, 3584, generator=g) * 2 - 1) * 0.5).to(gc.BF).double()
    E, D = A @ W.t(), A[:, :-64] @ W[:, :-64].t()
    inside = float(((D - E).abs() <= 2e-2 * 3584 ** 0.5 + 2e-2 * E.abs()).float().mean())
    print(f"outputs of a GEMM without its last K tile inside the old split-K tolerance: {inside:.3f}")
    assert inside > 0.5
    rep = gc.run_gemm4(gc.RefImpl(drop_last_ktile=True), CPU, 3584, [("wide", 129, 256)], ((128, 1),), (0,))
    assert rep.failed("gemm4 epi 0")
