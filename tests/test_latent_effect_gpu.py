"""Causal latent ranking on the MI355X: the ``latent_effect`` kernel against the fp64 explicit-ablation reference,
its exact zeros, bitwise batch invariance, ``_score_pairs`` against the CPU path and the sweep's reuse levels under
``intervention.latent_score = effect_lens``."""
from dataclasses import replace

import pytest
import torch

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.models.gemma2 import Gemma2Model
from taboo_brittleness_amd.models.spec import GEMMA2_TINY
from taboo_brittleness_amd.models.weights import random_gemma2
from taboo_brittleness_amd.ops import reference as ref
from test_engine_gpu import _assert_records_equal, tb_gemm  # noqa: F401  (fixture)
from test_latent_effect_cpu import EPS, GAP, ROWS, SEG, annihilated_case, check_prefixes, closed_form, effect_case

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SPEC = replace(GEMMA2_TINY, vocab_size=2048, layers=4, sliding_window=8)     # the spec of tests/test_affine_edit_gpu.py
TABLES = [torch.float32, BF]
# D = 64: most lanes idle; 328: a ragged second 16-byte pass; 3584: the 9B width.  L = 1000 and 16384: the 40 % row
# overflows the kernel's id list several times; 16384 only at the 9B width.
SHAPES = [(64, 256), (64, 1000), (328, 256), (328, 1000), (3584, 256), (3584, 1000), (3584, 16384)]
# (mode, cap, alpha, V per row): every value of each with every mode, and each pairing of cap / alpha / V form once
FULL = [(0, 30.0, 1.0, False), (0, 30.0, 0.5, True), (0, 0.0, 1.0, True), (0, 0.0, 0.5, False), (0, 30.0, 0.0, False),
        (1, 0.0, 1.0, True), (1, 0.0, 0.5, False), (1, 0.0, 0.0, True)]
LARGE = [(0, 30.0, 1.0, False), (1, 0.0, 0.5, True)]                          # the 16384-latent table: two settings


def _dev(c, gpu):
    return {k: v.to(gpu) for k, v in c.items()}


def _run(c, per_row, alpha, cap, mode):
    s, e = ops.latent_effect(c["acts"], c["X"], c["V"] if per_row else c["V"][:1], c["Wd"], c["seg"], alpha, EPS, cap,
                             mode, want_eff=True)
    return s.cpu(), e.cpu()


def _check(c, g, per_row, alpha, cap, mode):
    """One setting: GPU against the fp64 reference within 8 x the error of the same closed form with fp32 dot
    products in PyTorch on the CPU (its output stored as fp32 like the kernel's), computed on these inputs.  The
    reference reads the table the kernel reads (bf16-rounded for a bf16 table).  Returns (GPU error, bound)."""
    V = c["V"] if per_row else c["V"][:1]
    sr, er = ref.latent_effect(c["acts"], c["X"], V, c["Wd"], c["seg"], alpha, EPS, cap, mode)
    s32, e32 = closed_form(c["acts"], c["X"], V, c["Wd"], c["seg"], alpha, EPS, cap, mode, dots=torch.float32)
    tol = 8.0 * max(float((e32.float().double() - er).abs().max()), float((s32.float().double() - sr).abs().max()))
    sg, eg = _run(g, per_row, alpha, cap, mode)
    assert torch.all(eg[c["acts"] <= 0] == 0.0)
    assert torch.all(sg[2] == 0.0) and torch.all(sg[0] == 0.0)              # the empty and the all-silent segment
    if alpha == 0.0:
        assert torch.all(eg == 0.0) and torch.all(sg == 0.0)
    err = max(float((eg.double() - er).abs().max()), float((sg.double() - sr).abs().max()))
    return err, tol, float(er.abs().max())


@pytest.mark.parametrize("table", TABLES, ids=["f32", "bf16"])
@pytest.mark.parametrize("D,L", SHAPES)
def test_latent_effect_matches_reference(gpu, D, L, table):
    c = effect_case(D, L, table=table)
    g = _dev(c, gpu)
    worst, bound, size = 0.0, 0.0, 0.0
    for mode, cap, alpha, per_row in (LARGE if L > 4096 else FULL):
        err, tol, mag = _check(c, g, per_row, alpha, cap, mode)
        worst, bound, size = max(worst, err), max(bound, tol), max(size, mag)
        assert err <= tol, (mode, cap, alpha, per_row, err, tol)
    print(f"latent_effect D={D} L={L} table={table}: max GPU error {worst:.3e} (largest bound {bound:.3e}, "
          f"largest |eff| {size:.3e})")


@pytest.mark.parametrize("table", TABLES, ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [64, 328, 3584])
def test_annihilated_row(gpu, D, table):
    """``x = c d``: the edited residual is exactly 0, so the effect is the whole capped logit; finite and within the
    same bound (inputs on a 1/8 grid: every fp32 dot product is exact)."""
    c = annihilated_case(D, 256, table=table)
    g = _dev(c, gpu)
    for mode, cap, alpha, per_row in FULL:
        sr, er = ref.latent_effect(c["acts"], c["X"], c["V"] if per_row else c["V"][:1], c["Wd"], c["seg"], alpha, EPS,
                                   cap, mode)
        s32, e32 = closed_form(c["acts"], c["X"], c["V"] if per_row else c["V"][:1], c["Wd"], c["seg"], alpha, EPS,
                               cap, mode, dots=torch.float32)
        tol = 8.0 * max(float((e32.float().double() - er).abs().max()), float((s32.float().double() - sr).abs().max()))
        sg, eg = _run(g, per_row, alpha, cap, mode)
        assert torch.isfinite(eg).all() and torch.isfinite(sg).all()
        err = max(float((eg.double() - er).abs().max()), float((sg.double() - sr).abs().max()))
        assert err <= tol, (mode, cap, alpha, per_row, err, tol)
        if mode == 0 and alpha == 1.0:
            assert float(eg[0, 128].abs()) > 0.0


def test_exact_zeros(gpu):
    g = _dev(effect_case(328, 1000), gpu)
    for mode in (0, 1):
        s, e = _run(g, True, 1.0, 30.0, mode)
        silent = (g["acts"] <= 0).cpu()
        assert torch.all(e[silent] == 0.0) and float(e[~silent].abs().min()) > 0.0
        assert not torch.signbit(e[silent]).any()                               # +0.0, not -0.0
        s0, e0 = _run(g, True, 0.0, 30.0, mode)
        assert torch.all(e0 == 0.0) and torch.all(s0 == 0.0)
        assert s.shape == (len(SEG) - 1, 1000) and e.shape == (ROWS, 1000)
    # no eff requested: the same scores
    assert torch.equal(ops.latent_effect(g["acts"], g["X"], g["V"], g["Wd"], g["seg"], 1.0, EPS, 30.0, 0).cpu(),
                       _run(g, True, 1.0, 30.0, 0)[0])


@pytest.mark.parametrize("table", TABLES, ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [328, 3584])
def test_batch_invariance(gpu, D, table):
    """Bit for bit: each row's ``eff`` alone against the 5-row launch, each segment's ``score`` alone against the
    launch with the other segments."""
    g = _dev(effect_case(D, 1000, table=table), gpu)
    one = torch.tensor([0, 1], dtype=torch.int32, device=gpu)
    for mode in (0, 1):
        for per_row in (False, True):
            V = g["V"] if per_row else g["V"][:1]
            s5, e5 = ops.latent_effect(g["acts"], g["X"], V, g["Wd"], g["seg"], 0.5, EPS, 30.0, mode, want_eff=True)
            assert float(e5.abs().max()) > 0
            for t in range(ROWS):
                Vt = V[t:t + 1] if per_row else V
                _, e1 = ops.latent_effect(g["acts"][t:t + 1].contiguous(), g["X"][t:t + 1].contiguous(),
                                          Vt.contiguous(), g["Wd"], one, 0.5, EPS, 30.0, mode, want_eff=True)
                assert torch.equal(e1[0], e5[t]), (mode, per_row, t)
            for k, (a, b) in enumerate(zip(SEG[:-1], SEG[1:])):
                Vs = V[a:b] if per_row else V
                if per_row and b == a:
                    Vs = V[:1]
                sk = ops.latent_effect(g["acts"][a:b].contiguous(), g["X"][a:b].contiguous(), Vs.contiguous(),
                                       g["Wd"], torch.tensor([0, b - a], dtype=torch.int32, device=gpu), 0.5, EPS,
                                       30.0, mode)
                assert torch.equal(sk[0], s5[k]), (mode, per_row, k)


def test_unsupported_shapes_raise(gpu):
    def call(D, L=16, R=2, vrows=1, table=torch.float32, mode=0):
        return ops.latent_effect(torch.zeros(R, L, device=gpu), torch.zeros(R, D, dtype=BF, device=gpu),
                                 torch.zeros(vrows, D, device=gpu), torch.zeros(L, D, dtype=table, device=gpu),
                                 torch.tensor([0, R], dtype=torch.int32, device=gpu), 1.0, EPS, 30.0, mode)

    assert call(64).shape == (1, 16)
    for kw in (dict(D=12), dict(D=4104), dict(D=64, vrows=3), dict(D=64, table=torch.float16), dict(D=64, mode=2)):
        with pytest.raises(RuntimeError):
            call(**kw)


# ------------------------------------------------------------------------------------------------------- sweep
def _models(gpu, **kw):
    return Gemma2Model(random_gemma2(SPEC, dtype=BF, seed=5, norm_std=0.1, device=gpu, **kw), gpu)


def _runner(gpu, mg, extra=(), **kw):
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    cfg = load_config(None, ["experiment.max_new_tokens=12", "intervention.budgets=[1, 2, 4, 8]",
                             "intervention.random_trials=2", "intervention.latent_score=effect_lens"] + list(extra))
    sae = JumpReLUSAE.random(SPEC.hidden, 1024, seed=2, device=gpu)
    r = SweepRunner(cfg, mg, SyntheticTokenizer(vocab_size=SPEC.vocab_size), sae, batch=96, device=gpu, layer=2,
                    kv_pairs=8, **kw)
    return r, cfg


def test_score_pairs_gpu_matches_cpu_path(gpu, tb_gemm):
    """The GPU runner's scores on its own baselines against the CPU path (``ref.latent_effect``) on the same spike
    rows and activations, within the kernel test's bound; the targeted prefixes under the CPU tests' gap rule."""
    from taboo_brittleness_amd.interp import gradient as GR

    mg = _models(gpu)
    r, cfg = _runner(gpu, mg)
    pairs = r.build_pairs(["ship"], cfg.prompts[:4])
    r.run_baselines(pairs)
    r._score_pairs(pairs)
    u = GR.lens_direction(mg, pairs[0].track[:1]).view(1, -1).cpu()
    Wd = r.sae.W_dec.cpu()
    brute = []
    for p in pairs:
        X = p.resid[p.spikes_rel]
        acts = r.sae.encode(X).cpu()
        seg = torch.tensor([0, X.shape[0]], dtype=torch.int32)
        args = (acts, X.cpu(), u, Wd, seg, r.iv.alpha, mg.spec.eps, mg.spec.final_softcap, 0)
        want, _ = ref.latent_effect(*args)
        s32, _ = closed_form(*args, dots=torch.float32)
        tol = 8.0 * float((s32.float().double() - want).abs().max())
        got = r.word_scores[p.word][p.pidx].cpu().double()
        err = float((got - want[0]).abs().max())
        print(f"pair {p.pidx}: {int((acts > 0).any(0).sum())} active latents, score error {err:.3e}, bound {tol:.3e}")
        assert float(want.abs().max()) > 0 and err <= tol
        assert len(p.targeted) == 8 and p.targeted_corr is not None
        brute.append(want[0])
    check_prefixes(pairs, brute)
    assert GAP == 1e-6


@pytest.fixture(scope="module")
def lens_sweeps(gpu):
    """A 2-pair sweep under effect_lens from scratch and with every reuse level (in-tree GEMMs: batch-invariant)."""
    from taboo_brittleness_amd.runtime import gemm_dispatch as GD

    old = GD.mode()
    GD.set_mode("tb")
    on, off = dict(prefix_share=True, layer_resume=True), dict(prefix_share=False, layer_resume=False)
    mg = _models(gpu, post_norm_gain=8.0)
    key = lambda x: (x["word"], x["prompt_idx"], x["method"], x["budget"], x["trial"])   # noqa: E731
    out, stats, tg = {}, {}, {}
    try:
        for name, kw in (("scratch", off), ("reuse", on)):
            r, cfg = _runner(gpu, mg, ["intervention.budgets=[1, 4]"], **kw)
            pairs = r.build_pairs(["ship"], cfg.prompts[:2])
            r.run_baselines(pairs)
            res = r.run_cells(pairs, r.make_cells(pairs, ("sae_targeted", "sae_random")))
            out[name] = {key(x): x for x in res}
            stats[name] = dict(r.stats)
            tg[name] = [(p.targeted, p.targeted_scores, p.targeted_corr) for p in pairs]
    finally:
        GD.set_mode(old)
    return out, stats, tg


def test_sweep_gpu_effect_lens_reuse_is_exact(lens_sweeps):
    """Every cell from scratch against all reuse levels.  Float aggregates to 1e-6 relative: the NLL summation order
    differs as in test_sweep_gpu_prefix_share_equivalence."""
    out, stats, tg = lens_sweeps
    assert stats["reuse"]["tf_rows"] > 0 and len(out["reuse"]) == 2 * (2 + 2 * 2)
    assert tg["scratch"] == tg["reuse"] and all(t[1] is not None for t in tg["reuse"])
    _assert_records_equal(out["scratch"], out["reuse"], float_rtol=1e-6)
