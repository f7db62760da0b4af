"""Norm-matched random-direction controls on the MI355X: the ``matched_noise_edit`` kernel against its reference
and against its targeted siblings (same coefficients, same untouched rows, same norm), batch invariance, the noise
kinds of the hook inside a captured decode graph, and the sweep's reuse levels with the noise methods."""
from dataclasses import replace

import pytest
import torch

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.models.gemma2 import Gemma2Model
from taboo_brittleness_amd.models.spec import GEMMA2_TINY
from taboo_brittleness_amd.models.weights import random_gemma2
from taboo_brittleness_amd.ops import reference as ref
from test_affine_edit_cpu import INACTIVE_ROW, _close, _run, affine_case
from test_engine_gpu import _assert_records_equal, tb_gemm  # noqa: F401  (fixture)
from test_matched_noise_cpu import (NOISE_SWEEP, POS, SEEDS, check_norm_identities, edited_rows, noise_run)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SPEC = replace(GEMMA2_TINY, vocab_size=2048, layers=4, sliding_window=8)
WIDTHS = [512, 3584, 8192]     # one vector per thread with most threads idle; a ragged second slot; the VPT limit
TABLES = [torch.float32, BF]


def _gpu_case(c, gpu):
    return {k: v.to(gpu) for k, v in c.items()}


@pytest.fixture(scope="module")
def cases(gpu):
    return {D: (affine_case(D), _gpu_case(affine_case(D), gpu)) for D in WIDTHS}


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("with_val", [False, True])
def test_matched_noise_edit_matches_reference(cases, D, table, with_val):
    """The 9 rows of ``affine_case`` at alpha 1, 0.5 and 0.  Tolerances: those of
    test_latent_affine_edit_matches_reference for the same fp32-sum -> bf16 -> RMSNorm chain (the kernel's ``z``
    differs from numpy's only in the rounding of the fp64 ``log`` / ``cos``)."""
    c, g = cases[D]
    for alpha in (1.0, 0.5, 0.0):
        hr, xr, cr, nr = noise_run(ref.matched_noise_edit, c, table, alpha, with_val=with_val)
        hg, xg, cg, ng = (t.cpu() for t in noise_run(ops.matched_noise_edit, g, table, alpha, with_val=with_val))
        _close(hg, hr, 3e-2, 1e-2)
        _close(xg, xr, 3e-2, 1e-2)
        _close(cg, cr, 1e-3, 1e-3)
        _close(ng, nr, 1e-3, 1e-3)
        assert edited_rows(hg, c) == edited_rows(hr, c)
        noop = [r for r in range(9) if r not in edited_rows(hr, c)]
        assert {1, 2} <= set(noop) and (with_val or INACTIVE_ROW in noop)
        for r in noop:                                            # bit-unchanged, norm 0
            assert torch.equal(hg[r], c["h"][r]) and torch.equal(xg[r], c["x"][r]) and float(ng[r]) == 0.0
        if alpha > 0 or with_val:
            assert not torch.equal(hg[0], c["h"][0]) and float(ng[0]) > 0


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("table", TABLES)
def test_coefficients_norm_and_noops_are_the_siblings(cases, D, table):
    """``coef_out`` is bit-equal to ``lowrank_edit``'s (no ``val``) and ``latent_affine_edit``'s (``val``), the rows
    left untouched are the same rows, and the row moves as far as the sibling moves it: both norm identities on the
    kernel's own outputs."""
    c, g = cases[D]
    for with_val in (False, True):
        for full in (True, False):
            for alpha in (1.0, 0.5, 0.0):
                h, x, co, no = noise_run(ops.matched_noise_edit, g, table, alpha, full, with_val)
                ht, xt, ct = _run(ops.latent_affine_edit if with_val else ops.lowrank_edit, g, table, alpha, full,
                                  with_val=with_val)
                assert torch.equal(co, ct), (with_val, full, alpha)
                assert edited_rows(h, c) == edited_rows(ht, c), (with_val, full, alpha)
                keep = [r for r in range(9) if r not in edited_rows(ht, c)]
                assert torch.equal(x[keep], g["x"][keep]) and float(no[keep].abs().max()) == 0.0
                worst = check_norm_identities(h, no, ht, c)
                print(f"D={D} val={with_val} full={full} alpha={alpha}: norm error / bound = {worst:.4f}")


@pytest.mark.parametrize("D", [512, 3584])
def test_batch_invariance_and_purity(gpu, D):
    """One row alone, as row 13 of 17 and as row 250 of 300: bit-equal ``h`` and ``x_next``; another seed or another
    position gives another row with the same norm."""
    c = affine_case(D)
    r = 0
    E, Dm = c["We"].float().to(gpu), c["Wd"].float().to(gpu)
    be, th, pb, wn = (c[k].to(gpu) for k in ("be", "th", "pb", "wn"))
    g = torch.Generator().manual_seed(5)

    def run(M, at, seed=77, pos=19):
        h = torch.randn(M, D, generator=g).to(BF)
        h[at] = c["h"][r]
        h, x = h.to(gpu), torch.zeros(M, D, dtype=BF, device=gpu)
        idx = torch.randint(0, E.shape[0], (M, 8), generator=g, dtype=torch.int32)
        val = torch.randn(M, 8, generator=g)
        idx[at], val[at] = c["idx"][r], c["val"][r]
        cnt = torch.randint(0, 9, (M,), generator=g, dtype=torch.int32)
        cnt[at] = 8
        seeds = torch.randint(0, 2 ** 62, (M,), generator=g, dtype=torch.int64)
        ps = torch.randint(0, 600, (M,), generator=g, dtype=torch.int32)
        seeds[at], ps[at] = seed, pos
        no = torch.zeros(M, device=gpu)
        ops.matched_noise_edit(h, torch.ones(M, dtype=torch.uint8, device=gpu), idx.to(gpu), cnt.to(gpu), E, Dm,
                               seeds.to(gpu), ps.to(gpu), val.to(gpu), be, th, pb, 0.5, wn, 1e-6, x, None, no)
        return h[at].cpu(), x[at].cpu(), float(no[at])

    h1, x1, n1 = run(1, 0)
    assert not torch.equal(h1, c["h"][r]) and n1 > 0
    for M, at in ((17, 13), (300, 250)):
        hm, xm, nm = run(M, at)
        assert torch.equal(hm, h1) and torch.equal(xm, x1) and nm == n1, (M, at)
    for kw in (dict(seed=78), dict(pos=20)):
        h2, x2, n2 = run(17, 13, **kw)
        assert n2 == n1 and not torch.equal(h2, h1) and not torch.equal(x2, x1)


@pytest.mark.parametrize("D", WIDTHS)
def test_orthonormal_basis_moves_by_the_projected_norm(gpu, D):
    """The ``proj_noise`` path: ``E = Dm = U`` (orthonormal, fp32), no threshold, alpha 1: ``norm_out = |U U^T x|``
    to 1e-3 relative, and the row moves that far."""
    g = torch.Generator().manual_seed(12)
    U = torch.linalg.qr(torch.randn(D, 4, generator=g, dtype=torch.float64))[0].t().contiguous()
    Uf = U.float().to(gpu)
    M = 5
    h0 = torch.randn(M, D, generator=g).to(BF)
    h = h0.to(gpu)
    idx = torch.arange(4, dtype=torch.int32).repeat(M, 1).to(gpu)
    cnt = torch.full((M,), 4, dtype=torch.int32, device=gpu)
    no = torch.zeros(M, device=gpu)
    ops.matched_noise_edit(h, torch.ones(M, dtype=torch.uint8, device=gpu), idx, cnt, Uf, Uf,
                           torch.arange(M, dtype=torch.int64, device=gpu) + 3,
                           torch.arange(M, dtype=torch.int32, device=gpu), norm_out=no)
    want = (h0.double() @ U.t()).norm(dim=1)
    got = no.cpu().double()
    assert bool(((got - want).abs() <= 1e-3 * want).all()), (got, want)
    hd = h.cpu().double()
    moved = (hd - h0.double()).norm(dim=1)
    assert bool(((moved - got).abs() <= 2.0 ** -8 * hd.norm(dim=1)).all())


def test_unsupported_widths_and_shapes_raise(gpu):
    def call(D=512, M=2, mmax=4, val=None, seeds=None, pos=None):
        h = torch.zeros(M, D, dtype=BF, device=gpu)
        ops.matched_noise_edit(h, torch.ones(M, dtype=torch.uint8, device=gpu),
                               torch.zeros(M, mmax, dtype=torch.int32, device=gpu),
                               torch.ones(M, dtype=torch.int32, device=gpu), torch.zeros(4, D, device=gpu),
                               torch.zeros(4, D, device=gpu),
                               torch.zeros(M, dtype=torch.int64, device=gpu) if seeds is None else seeds,
                               torch.zeros(M, dtype=torch.int32, device=gpu) if pos is None else pos, val)

    call()
    for D in (12, 8200):
        with pytest.raises(RuntimeError):
            call(D=D)
    with pytest.raises(RuntimeError):                             # val must be [rows, mmax] like idx
        call(val=torch.ones(2, 1, device=gpu))
    with pytest.raises(RuntimeError):                             # one seed per row, int64
        call(seeds=torch.zeros(3, dtype=torch.int64, device=gpu))
    with pytest.raises(RuntimeError):
        call(seeds=torch.zeros(2, dtype=torch.int32, device=gpu))
    with pytest.raises(RuntimeError):                             # one position per row, int32
        call(pos=torch.zeros(1, dtype=torch.int32, device=gpu))
    with pytest.raises(RuntimeError):
        call(pos=torch.zeros(2, dtype=torch.int64, device=gpu))


# ------------------------------------------------------------------------------------------- hook and engine
def _models(gpu, **kw):
    return Gemma2Model(random_gemma2(SPEC, dtype=BF, seed=5, norm_std=0.1, device=gpu, **kw), gpu)


def test_noise_hook_graph_decode_equals_eager(gpu, tb_gemm):
    """A captured-and-replayed decode with ``sae``, ``sae_noise``, ``proj_noise`` and ``none`` rows equals the eager
    one; the ``none`` row equals the plain run; the noise rows differ from the plain run and from the ``sae`` row
    (rows 0 and 1 share their prompt and their latents)."""
    from taboo_brittleness_amd.interp.edits import EditHook, EditPlan
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.runtime.generation import Generator

    mg = _models(gpu)
    sae = JumpReLUSAE.random(SPEC.hidden, 1024, seed=2, device=gpu)
    prompts = [[2, 5, 9, 11, 13], [2, 5, 9, 11, 13], [2, 5, 9, 11, 13], [2, 3, 4, 5, 6, 7, 8]]
    U = torch.linalg.qr(torch.randn(SPEC.hidden, 2, generator=torch.Generator().manual_seed(3)))[0].t().contiguous()
    # clamp mode: every selected latent moves, firing or not, so no row's edit is a no-op
    plan = EditPlan.build(gpu, [[3, 6, 9]] * 3 + [[]], ["sae", "sae_noise", "proj_noise", "none"],
                          [[5, 9, 100], [5, 9, 100], [0, 1], []], basis=U, mode="clamp",
                          values=[[8.0, -8.0, 4.0], [8.0, -8.0, 4.0], [0.0, 0.0], []], seeds=[0, 21, 22, 0])
    hooks = {2: [EditHook(plan, sae)]}
    plain = Generator(mg, 4, 32, use_graphs=False, stop_ids=(100_000,)).generate(prompts, 10)
    eager = Generator(mg, 4, 32, use_graphs=False, stop_ids=(100_000,)).generate(prompts, 10, hooks=hooks)
    g = Generator(mg, 4, 32, use_graphs=True, stop_ids=(100_000,))
    a = g.generate(prompts, 10, hooks=hooks, graph_key="k")
    b = g.generate(prompts, 10, hooks=hooks, graph_key="k")          # replay path
    for i in range(4):
        assert eager.response_ids(i) == a.response_ids(i) == b.response_ids(i)
    assert torch.equal(eager.tok_nll[:, :10], a.tok_nll[:, :10]) and torch.equal(a.tok_nll[:, :10], b.tok_nll[:, :10])
    assert plain.response_ids(3) == eager.response_ids(3)             # the unedited row is untouched
    assert torch.equal(plain.tok_nll[3, :10], eager.tok_nll[3, :10])
    for i in range(3):
        assert not torch.equal(plain.tok_nll[i, :10], eager.tok_nll[i, :10]), i
    for i in (1, 2):
        assert not torch.equal(eager.tok_nll[0, :10], eager.tok_nll[i, :10]), i


@pytest.fixture(scope="module")
def noise_sweeps(gpu):
    """The noise methods from scratch and with every reuse level, and the same sweep without them (in-tree GEMMs:
    batch-invariant), computed once."""
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from taboo_brittleness_amd.runtime import gemm_dispatch as GD

    old = GD.mode()
    GD.set_mode("tb")
    base = ["experiment.max_new_tokens=12", "intervention.budgets=[1, 4]", "intervention.ranks=[1, 4]",
            "intervention.noise_trials=2"]
    on, off = dict(prefix_share=True, layer_resume=True), dict(prefix_share=False, layer_resume=False)
    mg = _models(gpu, post_norm_gain=8.0)
    tok = SyntheticTokenizer(vocab_size=SPEC.vocab_size)
    key = lambda r: (r["word"], r["prompt_idx"], r["method"], r["budget"], r["trial"])   # noqa: E731
    out, stats = {}, {}
    try:
        for name, methods, kw in (("scratch", NOISE_SWEEP, off), ("reuse", NOISE_SWEEP, on),
                                  ("targeted", ("sae_targeted", "proj_targeted"), on)):
            cfg = load_config(None, base)
            sae = JumpReLUSAE.random(SPEC.hidden, 1024, seed=2, device=gpu)
            r = SweepRunner(cfg, mg, tok, sae, batch=96, device=gpu, layer=2, kv_pairs=8, **kw)
            pairs = r.build_pairs(["ship"], cfg.prompts[:4])
            r.run_baselines(pairs)
            res = r.run_cells(pairs, r.make_cells(pairs, methods))
            out[name] = {key(x): x for x in res}
            stats[name] = dict(r.stats)
    finally:
        GD.set_mode(old)
    print({n: {k: s[k] for k in ("cells", "diverged", "tf_rows")} for n, s in stats.items()})
    return out, stats


def test_sweep_gpu_noise_reuse_is_exact(noise_sweeps):
    """Every cell from scratch against all reuse levels.  Float aggregates to 1e-6 relative: the NLL summation order
    differs as in test_sweep_gpu_prefix_share_equivalence."""
    out, stats = noise_sweeps
    assert stats["reuse"]["tf_rows"] > 0 and stats["reuse"]["diverged"] > 0
    assert {k[2] for k in out["reuse"]} == set(NOISE_SWEEP)
    _assert_records_equal(out["scratch"], out["reuse"], float_rtol=1e-6)
    noise = [r for k, r in out["reuse"].items() if k[2].endswith("noise")]
    assert len(noise) == 4 * 2 * 2 * 2 and all(r["edit_norm"] > 0 for r in noise)
    assert any(a["response_ids"] != b["response_ids"] for a in noise for b in noise
               if (a["prompt_idx"], a["method"], a["budget"]) == (b["prompt_idx"], b["method"], b["budget"]))


def test_sweep_gpu_targeted_records_do_not_see_the_controls(noise_sweeps):
    out, _ = noise_sweeps
    assert len(out["targeted"]) == 4 * 4
    _assert_records_equal(out["targeted"], {k: out["reuse"][k] for k in out["targeted"]})
