"""Interchange (donor-swap) interventions on the MI355X: the ``interchange_edit`` kernel against its reference, its
bit identities with ``lowrank_edit`` and ``latent_affine_edit``, batch invariance, the swap hook inside a captured
decode graph, and the sweep's reuse levels with the swap methods."""
from dataclasses import replace

import pytest
import torch

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.models.gemma2 import Gemma2Model
from taboo_brittleness_amd.models.spec import GEMMA2_TINY
from taboo_brittleness_amd.models.weights import random_gemma2
from taboo_brittleness_amd.ops import reference as ref
from test_affine_edit_cpu import _close
from test_engine_gpu import FIELDS, _assert_records_equal, tb_gemm  # noqa: F401  (fixture)
from test_interchange_cpu import SELF_ROW, SWAP, silent_donor_case, swap_case, swap_run, untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SPEC = replace(GEMMA2_TINY, vocab_size=2048, layers=4, sliding_window=8)
WIDTHS = [512, 3584, 8192]     # one vector per thread with most threads idle; a ragged second slot; the VPT limit
TABLES = [torch.float32, BF]


def _gpu_case(c, gpu):
    return {k: v.to(gpu) for k, v in c.items()}


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("table", TABLES)
def test_interchange_edit_matches_reference(gpu, D, table):
    """The 9 rows of ``affine_case`` against the rotated donor table (one row its own donor, one ``src = -1``, one
    ``src = R``), with and without thr / bias / pre_bias at alpha 1, 0.5 and 0.  Tolerances: those of
    test_latent_affine_edit_matches_reference for the same fp32-sum -> bf16 -> RMSNorm chain.  The rows left untouched
    are the reference's."""
    c = swap_case(D)
    g = _gpu_case(c, gpu)
    for full in (True, False):
        for alpha in (1.0, 0.5, 0.0):
            hr, xr, cr, dr = swap_run(ref.interchange_edit, c, table, alpha, full)
            hg, xg, cg, dg = (t.cpu() for t in swap_run(ops.interchange_edit, g, table, alpha, full))
            for r in untouched(c):
                assert torch.equal(hg[r], c["h"][r]) and torch.equal(xg[r], c["x"][r]), (full, alpha, r)
            kept = lambda h, x: [r for r in range(9)                                       # noqa: E731
                                 if torch.equal(h[r], c["h"][r]) and torch.equal(x[r], c["x"][r])]
            assert kept(hg, xg) == kept(hr, xr), (full, alpha)
            _close(hg, hr, 3e-2, 1e-2)
            _close(xg, xr, 3e-2, 1e-2)
            _close(cg, cr, 1e-3, 1e-3)
            _close(dg, dr, 1e-3, 1e-3)
            assert torch.equal(hg[0], c["h"][0]) == (alpha == 0.0)


def _identities(g, table, alphas, full=True):
    """The three bit identities on the case ``g`` (GPU tensors)."""
    M, R = g["h"].shape[0], g["donor"].shape[0]
    E, Dm = g["We"].to(table), g["Wd"].to(table)
    b, t, p = (g["be"], g["th"], g["pb"]) if full else (None, None, None)
    ok = (g["src"] >= 0) & (g["src"] < R)
    for alpha in alphas:
        h, x, co, dc = swap_run(ops.interchange_edit, g, table, alpha, full)
        # own donor: an exact no-op
        assert torch.equal(h[SELF_ROW], g["h"][SELF_ROW]) and torch.equal(x[SELF_ROW], g["x"][SELF_ROW])
        assert torch.equal(co[SELF_ROW], dc[SELF_ROW])
        # any donor: latent_affine_edit with val = alpha * coef_out(donor rows), rows without a donor unflagged
        drows = g["donor"].index_select(0, g["src"].clamp(0, R - 1).long()).clone()
        ad = torch.zeros_like(co)
        ops.lowrank_edit(drows, g["apply"], g["idx"], g["cnt"], E, Dm, b, t, p, alpha, None, 1e-6, None, ad)
        flagged = ok & g["apply"].bool()
        assert torch.equal(ad[flagged], dc[flagged])
        ha, xa = g["h"].clone(), g["x"].clone()
        val = torch.tensor(alpha, dtype=torch.float32, device=ad.device) * ad
        ops.latent_affine_edit(ha, g["apply"] * ok.to(torch.uint8), g["idx"], g["cnt"], val, E, Dm, b, t, p, alpha,
                               g["wn"], 1e-6, xa)
        assert torch.equal(h, ha) and torch.equal(x, xa), alpha
        assert torch.equal(h, g["h"]) == (alpha == 0.0)


@pytest.mark.parametrize("D", WIDTHS)
def test_bit_identities_sae_tables(gpu, D):
    g = _gpu_case(swap_case(D), gpu)
    for table in TABLES:
        _identities(g, table, (1.0, 0.5, 0.0))
        # silent donor: lowrank_edit's bits
        silent, z, g2 = silent_donor_case(g)
        E, Dm = g["We"].to(table), g["Wd"].to(table)
        for alpha in (1.0, 0.5):
            h, x, co, dc = swap_run(ops.interchange_edit, g2, table, alpha, donor=silent, src=z)
            assert float(dc.abs().max()) == 0.0
            hl, xl, cl = g["h"].clone(), g["x"].clone(), torch.zeros_like(co)
            ops.lowrank_edit(hl, g["apply"], g["idx"], g["cnt"], E, Dm, g2["be"], g2["th"], g2["pb"], alpha, g["wn"],
                             1e-6, xl, cl)
            assert torch.equal(h, hl) and torch.equal(x, xl) and torch.equal(co, cl)
            assert not torch.equal(h, g["h"])


@pytest.mark.parametrize("D", WIDTHS)
def test_bit_identities_orthonormal_basis(gpu, D):
    """``E = Dm = U`` (fp32, rank 4) without a threshold: the same identities, and the rows take the donor's
    coordinates (``basis_check``'s bound: 2^-8 |h'| for the bf16 rounding of the row and the fp32 chain)."""
    c = swap_case(D)
    gen = torch.Generator().manual_seed(12)
    U = torch.linalg.qr(torch.randn(D, 4, generator=gen, dtype=torch.float64))[0].t().contiguous().float()
    M = c["h"].shape[0]
    c.update(We=U, Wd=U, idx=torch.arange(4, dtype=torch.int32).repeat(M, 1), cnt=c["cnt"].clamp(max=4),
             val=c["val"][:, :4].contiguous())
    g = _gpu_case(c, gpu)
    _identities(g, torch.float32, (1.0, 0.5, 0.0), full=False)
    z = torch.zeros(M, dtype=torch.int32, device=gpu)
    h, x, co, dc = swap_run(ops.interchange_edit, g, torch.float32, 1.0, False,
                            donor=torch.zeros(1, D, dtype=BF, device=gpu), src=z)
    hl, xl = g["h"].clone(), g["x"].clone()
    ops.lowrank_edit(hl, g["apply"], g["idx"], g["cnt"], g["We"], g["Wd"], None, None, None, 1.0, g["wn"], 1e-6, xl)
    assert torch.equal(h, hl) and torch.equal(x, xl) and float(dc.abs().max()) == 0.0
    h, x, co, dc = swap_run(ops.interchange_edit, g, torch.float32, 1.0, False)
    for r in (0, 8):                                              # cnt = 4: the whole basis
        got = h[r].double().cpu() @ U.double().t()
        want = c["donor"][int(c["src"][r])].double() @ U.double().t()
        assert float((got - want).abs().max()) <= 2.0 ** -8 * float(h[r].double().norm())


@pytest.mark.parametrize("D", [512, 3584])
def test_batch_invariance(gpu, D):
    """One row alone, as row 13 of 17 and as row 250 of 300; its donor row in a table of 1 row and at another place of
    a table of 40: bit-equal ``h`` and ``x_next``."""
    c = swap_case(D)
    r = 0                                                        # cnt = mmax, firing and silent latents
    E, Dm = c["We"].float().to(gpu), c["Wd"].float().to(gpu)
    be, th, pb, wn = (c[k].to(gpu) for k in ("be", "th", "pb", "wn"))
    drow = c["donor"][int(c["src"][r])]
    g = torch.Generator().manual_seed(5)

    def run(M, at, R, dat):
        h = torch.randn(M, D, generator=g).to(BF)
        h[at] = c["h"][r]
        h, x = h.to(gpu), torch.zeros(M, D, dtype=BF, device=gpu)
        donor = torch.randn(R, D, generator=g).to(BF)
        donor[dat] = drow
        src = torch.randint(-1, R + 1, (M,), generator=g, dtype=torch.int32)
        src[at] = dat
        idx = torch.randint(0, E.shape[0], (M, 8), generator=g, dtype=torch.int32)
        idx[at] = c["idx"][r]
        cnt = torch.randint(0, 9, (M,), generator=g, dtype=torch.int32)
        cnt[at] = 8
        ops.interchange_edit(h, torch.ones(M, dtype=torch.uint8, device=gpu), idx.to(gpu), cnt.to(gpu), E, Dm,
                             donor.to(gpu), src.to(gpu), be, th, pb, 0.5, wn, 1e-6, x)
        return h[at].cpu(), x[at].cpu()

    h1, x1 = run(1, 0, 1, 0)
    assert not torch.equal(h1, c["h"][r])
    for M, at, R, dat in ((17, 13, 40, 29), (300, 250, 40, 3), (300, 250, 1, 0), (1, 0, 40, 39)):
        hm, xm = run(M, at, R, dat)
        assert torch.equal(hm, h1) and torch.equal(xm, x1), (M, at, R, dat)


def test_unsupported_inputs_raise(gpu):
    def call(D=512, **kw):
        a = dict(h=torch.zeros(2, D, dtype=BF, device=gpu), apply=torch.ones(2, dtype=torch.uint8, device=gpu),
                 idx=torch.zeros(2, 4, dtype=torch.int32, device=gpu), cnt=torch.ones(2, dtype=torch.int32, device=gpu),
                 E=torch.zeros(4, D, device=gpu), Dm=torch.zeros(4, D, device=gpu),
                 donor=torch.zeros(3, D, dtype=BF, device=gpu), src=torch.zeros(2, dtype=torch.int32, device=gpu))
        a.update(kw)
        ops.interchange_edit(a["h"], a["apply"], a["idx"], a["cnt"], a["E"], a["Dm"], a["donor"], a["src"],
                             coef_out=a.get("coef_out"), dcoef_out=a.get("dcoef_out"))

    call()
    for D in (12, 8200):
        with pytest.raises(RuntimeError):
            call(D=D)
    for bad in (dict(donor=torch.zeros(3, 512, device=gpu)),                          # donor must be bf16
                dict(donor=torch.zeros(3, 256, dtype=BF, device=gpu)),                # ... of h's width
                dict(donor=torch.zeros(3 * 512, dtype=BF, device=gpu)),               # ... and [R, D]
                dict(donor=torch.zeros(3, 1024, dtype=BF, device=gpu)[:, :512]),      # ... contiguous
                dict(src=torch.zeros(2, dtype=torch.int64, device=gpu)),              # src int32
                dict(src=torch.zeros(3, dtype=torch.int32, device=gpu)),              # ... one per row
                dict(dcoef_out=torch.zeros(2, 2, device=gpu)),                        # smaller than [rows, mmax]
                dict(E=torch.zeros(4, 512, dtype=torch.float16, device=gpu),
                     Dm=torch.zeros(4, 512, dtype=torch.float16, device=gpu))):       # table dtype
        with pytest.raises(RuntimeError):
            call(**bad)
    # an empty donor table leaves every row alone
    h = torch.ones(2, 512, dtype=BF, device=gpu)
    call(h=h, donor=torch.zeros(0, 512, dtype=BF, device=gpu), E=torch.ones(4, 512, device=gpu),
         Dm=torch.ones(4, 512, device=gpu))
    assert bool((h == 1).all())


# ------------------------------------------------------------------------------------------- hook and engine
def _models(gpu, **kw):
    return Gemma2Model(random_gemma2(SPEC, dtype=BF, seed=5, norm_std=0.1, device=gpu, **kw), gpu)


def test_swap_hook_graph_decode_equals_eager(gpu, tb_gemm):
    """A captured-and-replayed decode with ``sae_swap``, ``proj_swap``, ``sae`` and ``none`` rows equals the eager one;
    the ``none`` row equals the plain run and the swap rows do not."""
    from taboo_brittleness_amd.interp.edits import EditHook, EditPlan
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.runtime.generation import Generator

    mg = _models(gpu)
    sae = JumpReLUSAE.random(SPEC.hidden, 1024, seed=2, device=gpu)
    prompts = [[2, 5, 9, 11, 13], [2, 5, 9, 11, 13], [2, 7, 8], [2, 3, 4, 5, 6, 7, 8]]
    gen = torch.Generator().manual_seed(3)
    U = torch.linalg.qr(torch.randn(SPEC.hidden, 2, generator=gen))[0].t().contiguous()
    donor = torch.randn(6, SPEC.hidden, generator=gen).to(BF).to(gpu)
    # latents that fire on the donor rows of row 0's spikes, so that its swap is a real edit at each of them
    lat = [int(torch.nonzero(sae.encode(donor[k:k + 1])[0]).flatten()[0]) for k in range(3)]
    plan = EditPlan.build(gpu, [[3, 6, 9], [3, 6, 9], [4, 5], []], ["sae_swap", "proj_swap", "sae", "none"],
                          [list(dict.fromkeys(lat)), [0, 1], [17], []], basis=U, donor=donor, donor_base=[0, 3, -1, -1])
    assert plan.has_swap == (True, True)
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
    for i in range(2):
        assert not torch.equal(plain.tok_nll[i, :10], eager.tok_nll[i, :10]), i
    assert not torch.equal(eager.tok_nll[0, :10], eager.tok_nll[1, :10])


SWEEP_METHODS = ("sae_targeted", "proj_targeted") + SWAP


@pytest.fixture(scope="module")
def swap_sweeps(gpu):
    """The swap methods from scratch and with every reuse level, and the targeted methods alone (in-tree GEMMs:
    batch-invariant), computed once."""
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from taboo_brittleness_amd.runtime import gemm_dispatch as GD

    old = GD.mode()
    GD.set_mode("tb")
    base = ["experiment.max_new_tokens=12", "intervention.budgets=[1, 4]", "intervention.ranks=[1, 4]",
            "intervention.random_trials=2", "intervention.proj_random_trials=1"]
    on, off = dict(prefix_share=True, layer_resume=True), dict(prefix_share=False, layer_resume=False)
    mg = _models(gpu, post_norm_gain=8.0)
    tok = SyntheticTokenizer(vocab_size=SPEC.vocab_size)
    key = lambda r: (r["word"], r["prompt_idx"], r["method"], r["budget"], r["trial"])   # noqa: E731
    out, stats = {}, {}
    try:
        for name, methods, kw in (("scratch", SWEEP_METHODS, off), ("reuse", SWEEP_METHODS, on),
                                  ("targeted", ("sae_targeted", "proj_targeted"), on)):
            cfg = load_config(None, base)
            sae = JumpReLUSAE.random(SPEC.hidden, 1024, seed=2, device=gpu)
            r = SweepRunner(cfg, mg, tok, sae, batch=96, device=gpu, layer=2, kv_pairs=8, **kw)
            pairs = r.build_pairs(["ship", "moon"], cfg.prompts[:3], methods)
            r.run_baselines(pairs)
            res = r.run_cells(pairs, r.make_cells(pairs, methods))
            out[name] = {key(x): x for x in res}
            stats[name] = dict(r.stats, skipped=list(r.swap_skipped))
    finally:
        GD.set_mode(old)
    print({n: {k: s[k] for k in ("cells", "diverged", "tf_rows")} for n, s in stats.items()})
    return out, stats


def test_sweep_gpu_swap_reuse_is_exact(swap_sweeps):
    """Every cell from scratch against all reuse levels.  Float aggregates to 1e-6 relative: the NLL summation order
    differs as in test_sweep_gpu_prefix_share_equivalence."""
    out, stats = swap_sweeps
    assert stats["reuse"]["tf_rows"] > 0 and stats["reuse"]["diverged"] > 0 and not stats["reuse"]["skipped"]
    assert {k[2] for k in out["reuse"]} == set(SWEEP_METHODS)
    # 6 pairs x (2 + 2 targeted, sae_swap 2, sae_swap_random 4, proj_swap 2, proj_swap_random 2)
    assert len(out["reuse"]) == 6 * 14
    _assert_records_equal(out["scratch"], out["reuse"], float_rtol=1e-6,
                          fields=FIELDS + ("p_donor_mean", "p_donor_final", "p_donor_max", "delta_p_donor",
                                           "donor_word", "donor_prompt_idx", "donor_leak", "donor_in_topk"))
    swap = [r for k, r in out["reuse"].items() if k[2] in SWAP]
    assert all(r["donor_word"] != r["word"] and r["donor_prompt_idx"] == r["prompt_idx"] for r in swap)
    top = [r for r in swap if r["budget"] == 4]
    assert 2 * sum(r["nll_edit"] != r["nll_base"] for r in top) >= len(top)


def test_sweep_gpu_targeted_records_do_not_see_the_swaps(swap_sweeps):
    out, _ = swap_sweeps
    assert len(out["targeted"]) == 6 * 4
    _assert_records_equal(out["targeted"], {k: out["reuse"][k] for k in out["targeted"]},
                          fields=FIELDS + ("decoy_probs", "p_secret_final", "p_secret_max", "nll_self"))
    assert all("donor_word" not in r for r in out["targeted"].values())
