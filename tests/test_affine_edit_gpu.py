"""Latent clamping and steering on the MI355X: the ``latent_affine_edit`` kernel against its reference and against
``lowrank_edit``, its exact no-op, batch invariance, the clamp hook inside a captured decode graph, and the sweep's
reuse levels in clamp mode."""
from dataclasses import replace

import pytest
import torch

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.models.gemma2 import Gemma2Model
from taboo_brittleness_amd.models.spec import GEMMA2_TINY
from taboo_brittleness_amd.models.weights import random_gemma2
from taboo_brittleness_amd.ops import reference as ref
from test_affine_edit_cpu import INACTIVE_ROW, _close, _run, affine_case, basis_check
from test_engine_gpu import _assert_records_equal, tb_gemm  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SPEC = replace(GEMMA2_TINY, vocab_size=2048, layers=4, sliding_window=8)
WIDTHS = [512, 3584, 8192]     # one vector per thread with most threads idle; a ragged second slot; the VPT limit
TABLES = [torch.float32, BF]


def _gpu_case(c, gpu):
    return {k: v.to(gpu) for k, v in c.items()}


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("table", TABLES)
def test_latent_affine_edit_matches_reference(gpu, D, table):
    """Every row class of ``affine_case`` (cnt 0 / 1 / 5 / mmax, an unflagged row, firing and silent latents) with
    and without thr / bias / pre_bias at alpha 1, 0.5 and 0.  Tolerances: those of
    test_lowrank_edit_sae_and_projection for the same fp32-sum -> bf16 -> RMSNorm chain."""
    c = affine_case(D)
    g = _gpu_case(c, gpu)
    for full in (True, False):
        for alpha in (1.0, 0.5, 0.0):
            hr, xr, cr = _run(ref.latent_affine_edit, c, table, alpha, full)
            hg, xg, cg = (t.cpu() for t in _run(ops.latent_affine_edit, g, table, alpha, full))
            for r in (1, 2):                                      # unflagged / nothing selected: bit-unchanged
                assert torch.equal(hg[r], c["h"][r]) and torch.equal(xg[r], c["x"][r])
            _close(hg, hr, 3e-2, 1e-2)
            _close(xg, xr, 3e-2, 1e-2)
            _close(cg, cr, 1e-3, 1e-3)
            assert not torch.equal(hg[0], c["h"][0])


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("table", TABLES)
def test_val_zero_is_lowrank_edit_bit_for_bit(gpu, D, table):
    g = _gpu_case(affine_case(D), gpu)
    zero = torch.zeros_like(g["val"])
    for full in (True, False):
        for alpha in (1.0, 0.5, 0.0):
            a = _run(ops.latent_affine_edit, g, table, alpha, full, val=zero)
            b = _run(ops.lowrank_edit, g, table, alpha, full, with_val=False)
            for u, v in zip(a, b):
                assert torch.equal(u, v), (full, alpha)
            if full:                                             # the silent row is a no-op row of both
                r = INACTIVE_ROW
                assert torch.equal(a[0][r], g["h"][r]) and torch.equal(a[1][r], g["x"][r])
            if full and alpha > 0:
                assert not torch.equal(a[0][0], g["h"][0])


@pytest.mark.parametrize("D", WIDTHS)
def test_exact_noop_and_one_ulp(gpu, D):
    """``val = fl32(alpha * a)`` (``a`` from the kernel's own ``coef_out``) leaves ``h`` and ``x_next`` bit-unchanged;
    one entry one ulp off edits its row (``x_next`` is refreshed) and no other."""
    g = _gpu_case(affine_case(D), gpu)
    inf = torch.tensor(float("inf"), device=gpu)
    for table in TABLES:
        for alpha in (1.0, 0.5, 0.7):
            _, _, a = _run(ops.latent_affine_edit, g, table, alpha)
            v = torch.tensor(alpha, dtype=torch.float32, device=gpu) * a
            h, x, _ = _run(ops.latent_affine_edit, g, table, alpha, val=v)
            assert torch.equal(h, g["h"]) and torch.equal(x, g["x"])
            assert float(v[4, 0]) != 0.0                         # slot 0 of row 4 fires
            v[4, 0] = torch.nextafter(v[4, 0], inf)
            h, x, _ = _run(ops.latent_affine_edit, g, table, alpha, val=v)
            assert not torch.equal(x[4], g["x"][4])
            keep = [r for r in range(9) if r != 4]
            assert torch.equal(h[keep], g["h"][keep]) and torch.equal(x[keep], g["x"][keep])


@pytest.mark.parametrize("D", WIDTHS)
def test_clamp_moves_an_inactive_latent(gpu, D):
    """The case ablation cannot express: a selected latent below its threshold (``a = 0``) clamped to ``c != 0`` at
    alpha = 1 moves the row by ``c * W_dec[j]``; ``lowrank_edit`` leaves the same row untouched."""
    c = affine_case(D)
    g = _gpu_case(c, gpu)
    r = INACTIVE_ROW
    j, cv = int(c["idx"][r, 0]), float(c["val"][r, 0])
    assert int(c["cnt"][r]) == 1 and cv != 0.0
    for table in TABLES:
        h, x, a = _run(ops.latent_affine_edit, g, table, 1.0)
        assert float(a[r, 0]) == 0.0
        want = c["h"][r].float() + cv * c["Wd"].float()[j]
        _close(h[r].cpu(), want, 3e-2, 1e-2)
        assert not torch.equal(h[r], g["h"][r])
        _close(x[r].cpu(), ref.rmsnorm(want.to(BF)[None], c["wn"], 1e-6)[0], 3e-2, 1e-2)
        hl, xl, al = _run(ops.lowrank_edit, g, table, 1.0, with_val=False)
        assert float(al[r, 0]) == 0.0 and torch.equal(hl[r], g["h"][r]) and torch.equal(xl[r], g["x"][r])


@pytest.mark.parametrize("D", WIDTHS)
def test_clamp_on_an_orthonormal_basis(gpu, D):
    basis_check(ops.latent_affine_edit, D, gpu)


@pytest.mark.parametrize("D", [512, 3584])
def test_batch_invariance(gpu, D):
    """One row alone, as row 13 of 17 and as row 250 of 300: bit-equal ``h`` and ``x_next``."""
    c = affine_case(D)
    r = 0                                                        # cnt = mmax, firing and silent latents
    E, Dm = c["We"].float().to(gpu), c["Wd"].float().to(gpu)
    be, th, pb, wn = (c[k].to(gpu) for k in ("be", "th", "pb", "wn"))
    g = torch.Generator().manual_seed(5)

    def run(M, at):
        h = torch.randn(M, D, generator=g).to(BF)
        h[at] = c["h"][r]
        h, x = h.to(gpu), torch.zeros(M, D, dtype=BF, device=gpu)
        idx = torch.randint(0, E.shape[0], (M, 8), generator=g, dtype=torch.int32)
        val = torch.randn(M, 8, generator=g)
        idx[at], val[at] = c["idx"][r], c["val"][r]
        cnt = torch.randint(0, 9, (M,), generator=g, dtype=torch.int32)
        cnt[at] = 8
        ops.latent_affine_edit(h, torch.ones(M, dtype=torch.uint8, device=gpu), idx.to(gpu), cnt.to(gpu),
                               val.to(gpu), E, Dm, be, th, pb, 0.5, wn, 1e-6, x)
        return h[at].cpu(), x[at].cpu()

    h1, x1 = run(1, 0)
    assert not torch.equal(h1, c["h"][r])
    for M, at in ((17, 13), (300, 250)):
        hm, xm = run(M, at)
        assert torch.equal(hm, h1) and torch.equal(xm, x1), (M, at)


def test_unsupported_widths_raise(gpu):
    for D in (12, 8200):
        h = torch.zeros(2, D, dtype=BF, device=gpu)
        with pytest.raises(RuntimeError):
            ops.latent_affine_edit(h, torch.ones(2, dtype=torch.uint8, device=gpu),
                                   torch.zeros(2, 1, dtype=torch.int32, device=gpu),
                                   torch.ones(2, dtype=torch.int32, device=gpu), torch.ones(2, 1, device=gpu),
                                   torch.zeros(4, D, device=gpu), torch.zeros(4, D, device=gpu))
    h = torch.zeros(2, 512, dtype=BF, device=gpu)
    with pytest.raises(RuntimeError):                             # val must be [rows, mmax] like idx
        ops.latent_affine_edit(h, torch.ones(2, dtype=torch.uint8, device=gpu),
                               torch.zeros(2, 4, dtype=torch.int32, device=gpu),
                               torch.ones(2, dtype=torch.int32, device=gpu), torch.ones(2, 1, device=gpu),
                               torch.zeros(4, 512, device=gpu), torch.zeros(4, 512, device=gpu))


# ------------------------------------------------------------------------------------------- hook and engine
def _models(gpu, **kw):
    return Gemma2Model(random_gemma2(SPEC, dtype=BF, seed=5, norm_std=0.1, device=gpu, **kw), gpu)


def test_clamp_hook_graph_decode_equals_eager(gpu, tb_gemm):
    """A captured-and-replayed decode with the clamp hook equals the eager one; the unedited row equals the plain
    run and the edited rows do not."""
    from taboo_brittleness_amd.interp.edits import EditHook, EditPlan
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.runtime.generation import Generator

    mg = _models(gpu)
    sae = JumpReLUSAE.random(SPEC.hidden, 1024, seed=2, device=gpu)
    prompts = [[2, 5, 9, 11, 13], [2, 7, 8], [2, 3, 4, 5, 6, 7, 8]]
    plan = EditPlan.build(gpu, [[3, 6, 9], [4, 5], [], []], ["sae", "sae", "none", "none"],
                          [[5, 9, 100], [17], [], []], mode="clamp", values=[[8.0, -8.0, 4.0], [12.0], [], []])
    hooks = {2: [EditHook(plan, sae)]}
    plain = Generator(mg, 4, 32, use_graphs=False, stop_ids=(100_000,)).generate(prompts, 10)
    eager = Generator(mg, 4, 32, use_graphs=False, stop_ids=(100_000,)).generate(prompts, 10, hooks=hooks)
    g = Generator(mg, 4, 32, use_graphs=True, stop_ids=(100_000,))
    a = g.generate(prompts, 10, hooks=hooks, graph_key="k")
    b = g.generate(prompts, 10, hooks=hooks, graph_key="k")          # replay path
    for i in range(3):
        assert eager.response_ids(i) == a.response_ids(i) == b.response_ids(i)
    assert torch.equal(eager.tok_nll[:3, :10], a.tok_nll[:3, :10]) and torch.equal(a.tok_nll[:3, :10], b.tok_nll[:3, :10])
    assert plain.response_ids(2) == eager.response_ids(2)             # the unedited row is untouched
    assert torch.equal(plain.tok_nll[2, :10], eager.tok_nll[2, :10])
    for i in range(2):
        assert not torch.equal(plain.tok_nll[i, :10], eager.tok_nll[i, :10]), i


@pytest.fixture(scope="module")
def clamp_sweeps(gpu):
    """Clamp mode from scratch and with every reuse level, clamp to 0 and the error-preserving sweep (in-tree GEMMs:
    batch-invariant), computed once."""
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from taboo_brittleness_amd.runtime import gemm_dispatch as GD

    old = GD.mode()
    GD.set_mode("tb")
    base = ["experiment.max_new_tokens=12", "intervention.budgets=[1, 4]", "intervention.random_trials=2"]
    clamp = ["intervention.ablation_mode=clamp", "intervention.clamp_value=6.0"]
    clamp0 = ["intervention.ablation_mode=clamp", "intervention.clamp_value=0.0"]
    on, off = dict(prefix_share=True, layer_resume=True), dict(prefix_share=False, layer_resume=False)
    mg = _models(gpu, post_norm_gain=8.0)
    tok = SyntheticTokenizer(vocab_size=SPEC.vocab_size)
    key = lambda r: (r["word"], r["prompt_idx"], r["method"], r["budget"], r["trial"])   # noqa: E731
    out, stats = {}, {}
    try:
        for name, extra, kw in (("scratch", clamp, off), ("reuse", clamp, on), ("clamp0", clamp0, on), ("ep", [], on)):
            cfg = load_config(None, base + extra)
            sae = JumpReLUSAE.random(SPEC.hidden, 1024, seed=2, device=gpu)
            r = SweepRunner(cfg, mg, tok, sae, batch=96, device=gpu, layer=2, kv_pairs=8, **kw)
            pairs = r.build_pairs(["ship"], cfg.prompts[:4])
            r.run_baselines(pairs)
            res = r.run_cells(pairs, r.make_cells(pairs, ("sae_targeted", "sae_random")))
            out[name] = {key(x): x for x in res}
            stats[name] = dict(r.stats)
    finally:
        GD.set_mode(old)
    print({n: {k: s[k] for k in ("cells", "diverged", "tf_rows")} for n, s in stats.items()})
    return out, stats


def test_sweep_gpu_clamp_reuse_is_exact(clamp_sweeps):
    """Every cell from scratch against all reuse levels.  Float aggregates to 1e-6 relative: the NLL summation order
    differs as in test_sweep_gpu_prefix_share_equivalence."""
    out, stats = clamp_sweeps
    assert stats["reuse"]["tf_rows"] > 0 and stats["reuse"]["diverged"] > 0
    _assert_records_equal(out["scratch"], out["reuse"], float_rtol=1e-6)
    assert any(out["reuse"][k]["response_ids"] != out["ep"][k]["response_ids"] for k in out["ep"])


def test_sweep_gpu_clamp_to_zero_is_the_error_preserving_sweep(clamp_sweeps):
    """``clamp`` with ``clamp_value = 0`` runs the other kernel entry point and loses the no-op skip, and still
    gives the error-preserving sweep's records."""
    out, stats = clamp_sweeps
    assert stats["clamp0"]["tf_rows"] >= stats["ep"]["tf_rows"] > 0
    _assert_records_equal(out["ep"], out["clamp0"])
