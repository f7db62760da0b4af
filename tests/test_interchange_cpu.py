"""Interchange (donor-swap) interventions on the CPU: the ``interchange_edit`` reference and its three exact
properties, the swap kinds of the edit plan and hook, the donor rules and cells, and the swap methods through the
sweep, ``run_sweep``, the report and the CLI (tiny Gemma-2 geometry of tests/test_splice_cpu.py)."""
import json
import os
import socket
from types import SimpleNamespace

import pytest
import torch
import torch.multiprocessing as mp

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.config import load_config
from taboo_brittleness_amd.ops import reference as ref
from test_affine_edit_cpu import affine_case
from test_matched_noise_cpu import SW
from test_splice_cpu import OVR, _tiny

BF = torch.bfloat16
DEFAULT = ("sae_targeted", "sae_random", "proj_targeted", "proj_random")
SWAP = ("sae_swap", "sae_swap_random", "proj_swap", "proj_swap_random")
TWO_WORDS = ["word_plurals={ship: [ship, ships], moon: [moon, moons]}"]
SWAP_SW = SW + TWO_WORDS + ["intervention.ranks=[1, 2]"]
SELF_ROW, NONE_ROW, PAST_ROW = 4, 5, 7          # swap_case: own donor / src = -1 / src = R


def swap_case(D):
    """``affine_case(D)`` with a donor table (shared with tests/test_interchange_gpu.py): the case's rows rotated by
    one, plus one copy of row ``SELF_ROW`` -- that row is its own donor; ``NONE_ROW`` has ``src = -1`` and ``PAST_ROW``
    ``src = R``."""
    c = affine_case(D)
    M = c["h"].shape[0]
    c["donor"] = torch.cat([c["h"].roll(-1, 0), c["h"][SELF_ROW:SELF_ROW + 1]], 0).contiguous()
    src = torch.arange(M, dtype=torch.int32)
    src[SELF_ROW], src[NONE_ROW], src[PAST_ROW] = M, -1, M + 1
    c["src"] = src
    return c


def swap_run(fn, c, table, alpha, full=True, donor=None, src=None):
    """``fn`` (an interchange edit) on fresh copies of the case: ``(h, x_next, a(h), a(donor row))``."""
    E, Dm = c["We"].to(table), c["Wd"].to(table)
    h, x = c["h"].clone(), c["x"].clone()
    co = torch.zeros(c["idx"].shape, dtype=torch.float32, device=h.device)
    dc = torch.zeros(c["idx"].shape, dtype=torch.float32, device=h.device)
    b, t, p = (c["be"], c["th"], c["pb"]) if full else (None, None, None)
    fn(h, c["apply"], c["idx"], c["cnt"], E, Dm, c["donor"] if donor is None else donor,
       c["src"] if src is None else src, b, t, p, alpha, c["wn"], 1e-6, x, co, dc)
    return h, x, co, dc


def silent_donor_case(c):
    """``(donor, src, case)``: a one-row zero donor table every row points at, and the case without biases and with
    thresholds ``max(th, 0)`` taken against the bias-free pre-activations -- a zero row then has ``pre = 0 <= thr`` on
    every selected latent, while the latents of ``h`` well above zero still fire."""
    M, D = c["h"].shape
    pre = torch.einsum("rjd,rd->rj", c["We"].float()[c["idx"].long()], c["h"].float())
    off = torch.full(pre.shape, -0.3, device=pre.device)
    off[:, 1::2] = 0.3
    th = torch.zeros_like(c["th"])
    th[c["idx"].long().view(-1)] = (pre + off).clamp_min(0.0).view(-1)
    c2 = dict(c, be=torch.zeros_like(c["be"]), pb=torch.zeros_like(c["pb"]), th=th)
    dev = c["h"].device
    return torch.zeros(1, D, dtype=BF, device=dev), torch.zeros(M, dtype=torch.int32, device=dev), c2


def untouched(c):
    """Rows an interchange edit of ``swap_case`` must leave bit-identical whatever the donor holds: unflagged,
    nothing selected, its own donor, no donor row."""
    return [1, 2, SELF_ROW, NONE_ROW, PAST_ROW]


# ------------------------------------------------------------------------------------------------- reference
def test_reference_swaps_subspace_coordinates():
    """Orthonormal fp32 ``U``, alpha = 1, fp32 rows: afterwards ``U h' = U d`` and the complement of ``h`` is what it
    was.  Bound: the edit is ``r = 4`` fp32 dot products of length ``D`` and ``r`` axpys; each entry carries a few
    ulps of values of size ``|h| + |d|`` -- 64 eps (|h| + |d|) is a generous multiple of that."""
    D, r, M = 512, 4, 6
    g = torch.Generator().manual_seed(3)
    U = torch.linalg.qr(torch.randn(D, r, generator=g, dtype=torch.float64))[0].t().contiguous().float()
    h0 = torch.randn(M, D, generator=g)
    d = torch.randn(M + 2, D, generator=g)
    src = torch.tensor([1, 0, 7, 3, 2, 5], dtype=torch.int32)
    idx = torch.arange(r, dtype=torch.int32).repeat(M, 1)
    h = h0.clone()
    ref.interchange_edit(h, torch.ones(M, dtype=torch.uint8), idx, torch.full((M,), r, dtype=torch.int32), U, U, d, src)
    dd, Ud = d[src.long()].double(), U.double()
    tol = 64 * 2.0 ** -24 * (h0.double().norm(dim=1) + dd.norm(dim=1)).max()
    assert float((h.double() @ Ud.t() - dd @ Ud.t()).abs().max()) <= tol
    comp = lambda v: v - (v @ Ud.t()) @ Ud                       # noqa: E731
    assert float((comp(h.double()) - comp(h0.double())).abs().max()) <= tol
    assert not torch.equal(h, h0)
    with pytest.raises(ValueError, match="donor is"):
        ref.interchange_edit(h0.clone(), torch.ones(M, dtype=torch.uint8), idx, torch.full((M,), r, dtype=torch.int32),
                             U, U, d.to(BF), src)


def test_reference_sae_latents_take_the_donor_values():
    """SAE tables: after the edit the selected latents read the donor's activations, within the tolerance
    tests/test_affine_edit_cpu.py uses for clamped latents (``basis_check``: 2^-8 |h'| for the bf16 rounding of the
    row and the fp32 chain), here on an orthonormal encoder = decoder with a JumpReLU threshold below every value."""
    D, r, M = 512, 4, 5
    g = torch.Generator().manual_seed(12)
    U = torch.linalg.qr(torch.randn(D, r, generator=g, dtype=torch.float64))[0].t().contiguous().float()
    h = torch.randn(M, D, generator=g).to(BF)
    d = torch.randn(M, D, generator=g).to(BF)
    src = torch.tensor([1, 2, 3, 4, 0], dtype=torch.int32)
    thr = torch.full((r,), -1e4)
    co, dc = torch.zeros(M, r), torch.zeros(M, r)
    ops.interchange_edit(h, torch.ones(M, dtype=torch.uint8), torch.arange(r, dtype=torch.int32).repeat(M, 1),
                         torch.full((M,), r, dtype=torch.int32), U, U, d, src, torch.zeros(r), thr, None, 1.0,
                         coef_out=co, dcoef_out=dc)
    got = h.double() @ U.double().t()
    assert torch.allclose(dc.double(), d[src.long()].double() @ U.double().t(), atol=1e-4)
    bound = 2.0 ** -8 * h.double().norm(dim=1, keepdim=True)
    assert bool(((got - dc.double()).abs() <= bound).all()), float((got - dc.double()).abs().max())


@pytest.mark.parametrize("D", [512, 3584])
@pytest.mark.parametrize("table", [torch.float32, BF])
def test_reference_exact_properties(D, table):
    """(1) rows with all-zero coefficients -- own donor, alpha = 0 -- and rows without a donor keep their bits;
    (2) a silent donor gives ``lowrank_edit``'s bits; (3) any donor gives ``latent_affine_edit``'s bits with
    ``val = alpha * a(donor)``, ``a(donor)`` being ``lowrank_edit``'s ``coef_out`` on the donor rows."""
    c = swap_case(D)
    M = c["h"].shape[0]
    for full in (True, False):
        for alpha in (1.0, 0.5, 0.0):
            h, x, co, dc = swap_run(ref.interchange_edit, c, table, alpha, full)
            keep = untouched(c) if alpha else list(range(M))
            for r in keep:
                assert torch.equal(h[r], c["h"][r]) and torch.equal(x[r], c["x"][r]), (full, alpha, r)
            if alpha:
                assert not torch.equal(h[0], c["h"][0]) and not torch.equal(x[0], c["x"][0])
            # (3): a(d) from lowrank_edit's coef_out on the donor rows, rows without a donor unflagged
            ok = (c["src"] >= 0) & (c["src"] < c["donor"].shape[0])
            drows = c["donor"][c["src"].clamp(0, c["donor"].shape[0] - 1).long()].clone()
            E, Dm = c["We"].to(table), c["Wd"].to(table)
            b, t, p = (c["be"], c["th"], c["pb"]) if full else (None, None, None)
            ad = torch.zeros(c["idx"].shape)
            ref.lowrank_edit(drows, c["apply"], c["idx"], c["cnt"], E, Dm, b, t, p, alpha, None, 1e-6, None, ad)
            assert torch.equal(ad[ok & c["apply"].bool()], dc[ok & c["apply"].bool()])
            ha, xa = c["h"].clone(), c["x"].clone()
            ref.latent_affine_edit(ha, c["apply"] * ok.to(torch.uint8), c["idx"], c["cnt"],
                                   torch.tensor(alpha, dtype=torch.float32) * ad, E, Dm, b, t, p, alpha, c["wn"],
                                   1e-6, xa)
            assert torch.equal(h, ha) and torch.equal(x, xa), (full, alpha)
    # (2): a donor on which every selected latent is silent: the zero row, under thresholds that are >= 0
    silent, z, c2 = silent_donor_case(c)
    for alpha in (1.0, 0.5):
        h, x, co, dc = swap_run(ref.interchange_edit, c2, table, alpha, donor=silent, src=z)
        assert float(dc.abs().max()) == 0.0
        hl, xl = c["h"].clone(), c["x"].clone()
        cl = torch.zeros(c["idx"].shape)
        ref.lowrank_edit(hl, c["apply"], c["idx"], c["cnt"], c["We"].to(table), c["Wd"].to(table), c2["be"], c2["th"],
                         c2["pb"], alpha, c["wn"], 1e-6, xl, cl)
        assert torch.equal(h, hl) and torch.equal(x, xl) and torch.equal(co, cl)
        assert not torch.equal(h, c["h"])                          # ... and they are an edit's bits
    # the dispatching op takes the reference on CPU tensors
    a, b = swap_run(ops.interchange_edit, c, table, 0.5), swap_run(ref.interchange_edit, c, table, 0.5)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------- plan and hook
def test_plan_validation():
    from taboo_brittleness_amd.interp.edits import ALL_POSITIONS, KIND_CODES, EditPlan

    assert KIND_CODES["sae_swap"] == 5 and KIND_CODES["proj_swap"] == 6
    sp, sel = [[1], [2]], [[5, 9], [0]]
    donor = torch.zeros(4, 16, dtype=BF)
    for kinds in (["sae_swap", "sae"], ["proj", "proj_swap"]):
        with pytest.raises(ValueError, match="donor"):
            EditPlan.build("cpu", sp, kinds, sel)
        with pytest.raises(ValueError, match="donor"):
            EditPlan.build("cpu", sp, kinds, sel, donor=donor)
        with pytest.raises(ValueError, match="donor_base"):
            EditPlan.build("cpu", sp, kinds, sel, donor=donor, donor_base=[0])
    p = EditPlan.build("cpu", sp, ["sae_swap", "proj_swap"], sel, donor=donor, donor_base=[0, -1])
    assert p.kind.tolist() == [5, 6] and p.has_swap == (True, True) and p.donor_base.tolist() == [0, -1]
    assert p.donor_base.dtype == torch.int32 and p.has_noise == (False, False)
    with pytest.raises(ValueError, match="ALL_POSITIONS"):
        EditPlan.build("cpu", [[ALL_POSITIONS], [2]], ["proj_swap", "sae"], sel, donor=donor, donor_base=[0, -1])
    # an every-position row of another kind next to a swap row is fine
    EditPlan.build("cpu", [[ALL_POSITIONS], [2]], ["sae", "proj_swap"], sel, donor=donor, donor_base=[-1, 0])
    for mode in ("reconstruct", "clamp", "steer"):
        with pytest.raises(ValueError, match="error_preserving"):
            EditPlan.build("cpu", sp, ["sae_swap", "sae"], sel, donor=donor, donor_base=[0, -1], mode=mode)
        EditPlan.build("cpu", sp, ["proj_swap", "sae"], sel, donor=donor, donor_base=[0, -1], mode=mode)
    plain = EditPlan.build("cpu", sp, ["sae", "proj"], sel)
    assert plain.donor is None and plain.donor_base is None and plain.has_swap == (False, False)


def _hook_case():
    from taboo_brittleness_amd.interp.edits import EditHook, EditPlan

    _, _, _, sae = _tiny()
    D, B, T = sae.d_in, 4, 6
    g = torch.Generator().manual_seed(0)
    wn = (torch.randn(D, generator=g) * 0.1).to(BF)
    h0 = torch.randn(B * T, D, generator=g).to(BF)
    donor = torch.randn(6, D, generator=g).to(BF)
    donor[3] = h0[2 * T + 5]                                   # row 2's second spike is its own donor
    first = lambda row: int(torch.nonzero(sae.encode(row[None])[0]).flatten()[0])      # noqa: E731
    act3 = torch.nonzero(sae.encode(h0[3 * T + 1:3 * T + 2])[0]).flatten()
    U = torch.linalg.qr(torch.randn(D, 2, generator=g))[0].t().contiguous()
    # row 0: a latent active on each of its two spike rows and on each of their donor rows
    sel = [list(dict.fromkeys([first(h0[2]), first(donor[0]), first(h0[4]), first(donor[1])])), [], [0, 1],
           [int(act3[0])]]
    plan = EditPlan.build("cpu", [[2, 4], [1], [3, 5], [1]], ["sae_swap", "none", "proj_swap", "sae"], sel, basis=U,
                          donor=donor, donor_base=[0, -1, 2, -1])
    pos = torch.arange(T, dtype=torch.int32).repeat(B)
    ctx = SimpleNamespace(B=B, T=T, pos=pos, slot=torch.arange(B, dtype=torch.int32), w_next=wn, eps=1e-6)
    return EditHook(plan, sae), h0, ctx, wn, [2, 4, 2 * T + 3, 3 * T + 1], U, donor


def test_hook_swap_kinds_prefill_equals_decode():
    """Kinds 5 and 6 edit at their spikes only, the ``k``-th spike with donor row ``donor_base + k``; a position gets
    the same bits in a prefill and alone in a decode step; a spike whose donor row is the row itself stays; the
    ``sae`` row of the same plan is what it was."""
    from taboo_brittleness_amd.interp.edits import EditHook, EditPlan

    hook, h0, ctx, wn, edited, U, donor = _hook_case()
    T, D = ctx.T, h0.shape[1]
    h, x = h0.clone(), torch.zeros_like(h0)
    hook(h, x, ctx)
    for r in range(h0.shape[0]):
        assert torch.equal(h[r], h0[r]) == (r not in edited), r
        assert (float(x[r].float().abs().max()) == 0.0) == (r not in edited), r
    for r in edited + [2 * T + 5]:
        b, t = divmod(r, T)
        c1 = SimpleNamespace(B=1, T=1, pos=torch.tensor([t], dtype=torch.int32),
                             slot=torch.tensor([b], dtype=torch.int32), w_next=wn, eps=1e-6)
        h1, x1 = h0[r:r + 1].clone(), torch.zeros(1, D, dtype=BF)
        hook(h1, x1, c1)
        assert torch.equal(h1[0], h[r]) and torch.equal(x1[0], x[r])
    # the proj_swap row took the donor's coordinates (donor row 2 = base 2 + spike 0) and kept its complement
    r, d = 2 * T + 3, donor[2].double()
    Ud = U.double()
    tol = 2.0 ** -8 * float(h[r].double().norm())
    assert float((Ud @ h[r].double() - Ud @ d).abs().max()) <= tol
    comp = lambda v: v - Ud.t() @ (Ud @ v)                    # noqa: E731
    assert float((comp(h[r].double()) - comp(h0[r].double())).norm()) <= 2 * tol
    # the sae_swap row's second spike reads donor row 1, its first donor row 0
    s = hook.sae
    for r, dr in ((2, 0), (4, 1)):
        hh = h0[r:r + 1].clone()
        ops.interchange_edit(hh, torch.ones(1, dtype=torch.uint8), hook.plan.idx[0:1], hook.plan.cnt[0:1], s.W_encT,
                             s.W_dec, donor, torch.tensor([dr], dtype=torch.int32), s.b_enc, s.threshold,
                             s.b_dec if s.apply_b_dec_to_input else None, 1.0)
        assert torch.equal(hh[0], h[r])
    # the same plan without its swap rows runs the sae row alone, to the same bits
    p = hook.plan
    plain = EditPlan(p.spikes, torch.where(p.kind >= 5, torch.zeros_like(p.kind), p.kind), p.idx, p.cnt, basis=U)
    h2, x2 = h0.clone(), torch.zeros_like(h0)
    EditHook(plain, hook.sae)(h2, x2, ctx)
    assert torch.equal(h2[3 * T + 1], h[3 * T + 1]) and torch.equal(x2[3 * T + 1], x[3 * T + 1])
    assert "donor_src" not in EditHook(plain, hook.sae)._rows(1, 1, h0.device)      # no swap buffers either


# ------------------------------------------------------------------------------------- donor rules and cells
def _runner(extra=(), batch=60, **kw):
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    spec, m, tok, sae = _tiny()
    cfg = load_config(None, SWAP_SW + list(extra))
    return cfg, SweepRunner(cfg, m, tok, sae, batch=batch, device="cpu", layer=2, use_graphs=False, kv_pairs=8, **kw)


def _fake_baselines(r, pairs, spikes):
    D = r.D
    for i, (p, sp) in enumerate(zip(pairs, spikes)):
        p.resp = list(range(10, 18))
        p.resid = None if sp is None else torch.full((8, D), float(i), dtype=BF)
        p.spikes_rel = list(sp or [])
        p.targeted = [3 + i, 40 + i, 80 + i, 120 + i]
        p.active_pool = torch.arange(100 + 40 * i, 130 + 40 * i).numpy()       # disjoint pools


def test_donor_rules_skips_and_wrap():
    import numpy as np

    cfg, r = _runner(["word_plurals={moon: [moon, moons], smile: [smile, smiles], ship: [ship, ships]}"])
    assert cfg.words == ["moon", "smile", "ship"] and cfg.intervention.swap_donor == "next_word"
    pairs = r.build_pairs(cfg.words, cfg.prompts, SWAP)
    assert pairs[0].extra == {"smile": len(pairs[0].track) - 2, "ship": len(pairs[0].track) - 1}
    assert pairs[0].n_decoys == len(cfg.intervention.decoys["moon"])
    assert all(not p.extra for p in r.build_pairs(cfg.words, cfg.prompts))
    P = len(cfg.prompts)                                        # 3 prompts: pairs 0-2 moon, 3-5 smile, 6-8 ship
    # smile/1 has no baseline, smile/2 no spikes, ship/2 neither; ship/0 has one spike
    spikes = [[1, 4, 6], [2, 5], [0, 3], [1, 2], None, [], [5], [3, 4], None]
    _fake_baselines(r, pairs, spikes)
    d = r.swap_donors(pairs)
    #            moon/0   moon/1            moon/2 (smile/2, ship/2 skipped: none)
    assert d[:3] == [3, P * 2 + 1, -1]
    assert d[3:6] == [6, 7, 2]                                  # smile -> ship; smile/2 -> (ship/2 skipped) moon/2
    assert d[6:] == [0, 1, 2]                                   # ship -> moon (cyclic)
    r.swap_donor = "next_prompt"
    d = r.swap_donors(pairs)
    assert d[:3] == [1, 2, 0]
    assert d[3:6] == [-1, 3, 3]                                 # smile/1 and smile/2 are no donors: smile/0 has none
    assert d[6:] == [7, 6, 6]
    # cells: a pair without a donor gets none and is listed; the others get every (method, budget, trial) once
    cells = r.make_cells(pairs, DEFAULT + SWAP)
    assert r.swap_skipped == [("smile", 0)]
    assert not [c for c in cells if c.pair == 3 and c.method in SWAP]
    assert len([c for c in cells if c.pair == 3]) == len([c for c in r.make_cells(pairs, DEFAULT) if c.pair == 3])
    iv = cfg.intervention
    mine = [c for c in cells if c.pair == 6 and c.method in SWAP]
    assert [c.method for c in mine] == ["sae_swap"] * 2 + ["sae_swap_random"] * 2 * iv.random_trials + \
        ["proj_swap"] * 2 + ["proj_swap_random"] * 2 * iv.proj_random_trials
    assert all(c.donor == 7 for c in mine) and all(c.donor == -1 for c in cells if c.method not in SWAP)
    sw = [c for c in cells if c.method in SWAP]
    assert len({c.seed for c in sw}) == len(sw)
    assert [(c.method, c.budget, c.trial, c.seed) for c in cells if c.method not in SWAP] == \
        [(c.method, c.budget, c.trial, c.seed) for c in r.make_cells(pairs, DEFAULT)]
    # the plan: donor rows wrap (k mod n), sae_swap takes both targeted sets, the random swap avoids them
    r.swap_donor = "next_word"
    cells = r.make_cells(pairs[:7], ("sae_swap", "sae_swap_random"))
    c6 = [i for i, c in enumerate(cells) if c.pair == 0 and c.budget == 4]       # moon/0 (3 spikes) <- smile/0 (2)
    r._with_swap = (True, False)
    plan = r._plan_for(cells, pairs[:7], {})
    K = cfg.intervention.spikes_k
    dst, src, _ = plan["donor"]
    rows = {int(a): b for a, b in zip(dst, src)}
    ci = c6[0]
    assert plan["donor_base"][ci] == ci * K and plan["kind"][ci] == 5
    assert [rows[ci * K + k] for k in range(3)] == [(3, 1), (3, 2), (3, 1)]      # k mod n over smile/0's spikes
    assert plan["idx"].shape[1] == 2 * max(iv.budgets)
    assert plan["idx"][ci, :plan["cnt"][ci]].tolist() == pairs[0].targeted[:4] + pairs[3].targeted[:4]
    assert int(plan["f"][ci]) == -1                                           # no no-op spike skip for swap cells
    for cj in c6[1:]:
        got = plan["idx"][cj, :plan["cnt"][cj]].tolist()
        assert len(got) == 8 and len(set(got)) == 8
        assert not set(got) & set(pairs[0].targeted[:4] + pairs[3].targeted[:4])
        assert set(got[:4]) <= set(pairs[0].active_pool.tolist()) and set(got[4:]) <= set(pairs[3].active_pool.tolist())
    assert plan["idx"][c6[1]].tolist() != plan["idx"][c6[2]].tolist()
    assert np.all(plan["donor_base"][len(cells):] == -1)


def test_make_cells_and_run_sweep_raise():
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep

    for mode in ("reconstruct", "clamp", "steer"):
        cfg, r = _runner([f"intervention.ablation_mode={mode}", "intervention.clamp_value=2.0"])
        pairs = r.build_pairs(cfg.words, cfg.prompts, SWAP)
        _fake_baselines(r, pairs, [[1, 2]] * len(pairs))
        with pytest.raises(ValueError, match="error_preserving"):
            r.make_cells(pairs, ("sae_targeted", "sae_swap"))
        assert {c.method for c in r.make_cells(pairs, ("proj_swap", "proj_swap_random"))} == \
            {"proj_swap", "proj_swap_random"}
        with pytest.raises(ValueError, match="error_preserving"):
            run_sweep(cfg, "unused", ("sae_swap",), info=DistInfo(), log=lambda *a: None)
    cfg, r = _runner()
    with pytest.raises(ValueError, match="build_pairs"):                      # pairs built without the swap methods
        r.make_cells(r.build_pairs(cfg.words, cfg.prompts), SWAP)
    with pytest.raises(ValueError, match="swap_donor"):
        _runner(["intervention.swap_donor=nearest"])
    bad = load_config(None, SWAP_SW + ["intervention.swap_donor=nearest"])
    with pytest.raises(ValueError, match="swap_donor"):
        run_sweep(bad, "unused", SWAP, info=DistInfo(), log=lambda *a: None)
    forcing = load_config(None, SWAP_SW + ["intervention.measure_forcing=true"])
    with pytest.raises(ValueError, match="forcing"):
        run_sweep(forcing, "unused", DEFAULT + SWAP, info=DistInfo(), log=lambda *a: None)
    assert load_config(None, OVR).intervention.swap_donor == "next_word"


# ---------------------------------------------------------------------------------------------------- sweep
def _records(donor, methods, **kw):
    cfg, r = _runner([f"intervention.swap_donor={donor}"], **kw)
    pairs = r.build_pairs(cfg.words, cfg.prompts, methods)
    r.run_baselines(pairs)
    cells = r.make_cells(pairs, methods)
    out = []
    for c0 in range(0, len(cells), 50):                        # several batches: the donor table is refilled
        out += r.run_cells(pairs, cells[c0:c0 + 50], measure_nll=True)
    key = lambda x: (x["word"], x["prompt_idx"], x["method"], x["budget"], x["trial"])   # noqa: E731
    return {key(x): x for x in out}, r


@pytest.fixture(scope="module")
def sweeps():
    on, off = dict(prefix_share=True, layer_resume=True), dict(prefix_share=False, layer_resume=False)
    out = {}
    for donor in ("next_word", "next_prompt"):
        out[donor, "reuse"] = _records(donor, DEFAULT + SWAP, **on)
        out[donor, "scratch"] = _records(donor, DEFAULT + SWAP, **off)
    out["default"] = _records("next_word", DEFAULT, **on)
    return out


DONOR_STATS = ("p_donor_mean", "p_donor_final", "p_donor_max", "delta_p_donor")


@pytest.mark.parametrize("donor", ["next_word", "next_prompt"])
def test_sweep_reuse_equals_from_scratch(sweeps, donor):
    """Every reuse level on against ``prefix_share = layer_resume = False``, with the float tolerances of
    tests/test_matched_noise_cpu.py::test_sweep_reuse_equals_from_scratch."""
    a, b = sweeps[donor, "scratch"][0], sweeps[donor, "reuse"][0]
    assert set(a) == set(b) and {k[2] for k in a} == set(DEFAULT + SWAP)
    assert sweeps[donor, "reuse"][1].stats["tf_rows"] > 0
    for k in a:
        assert set(a[k]) == set(b[k]), k
        assert a[k]["response_ids"] == b[k]["response_ids"], k
        assert a[k]["topk_ids"] == b[k]["topk_ids"], k
        assert abs(a[k]["nll_edit"] - b[k]["nll_edit"]) < 1e-5, k
        for f in ("p_secret_mean", "p_secret_final", "p_secret_max") + (DONOR_STATS if k[2] in SWAP else ()):
            assert abs(a[k][f] - b[k][f]) < 1e-6 + 1e-5 * abs(a[k][f]), (k, f)
        if k[2] in SWAP:
            for f in ("donor_word", "donor_prompt_idx", "donor_leak", "donor_in_topk"):
                assert a[k][f] == b[k][f], (k, f)


@pytest.mark.parametrize("donor", ["next_word", "next_prompt"])
def test_sweep_swap_cells_edit_and_name_their_donor(sweeps, donor):
    """The condition on the inputs: at the largest budget and at the largest rank at least half of the swap cells
    leave their baseline (``nll_edit``).  Donor fields follow the rule."""
    got, runner = sweeps[donor, "reuse"]
    assert not runner.swap_skipped
    for meth, bud in (("sae_swap", 4), ("sae_swap_random", 4), ("proj_swap", 2), ("proj_swap_random", 2)):
        rs = [r for k, r in got.items() if k[2] == meth and k[3] == bud]
        assert rs and 2 * sum(r["nll_edit"] != r["nll_base"] for r in rs) >= len(rs), (meth, bud)
    n_prompts = 3
    for k, r in got.items():
        if k[2] not in SWAP:
            continue
        if donor == "next_word":
            assert r["donor_word"] == ("moon" if r["word"] == "ship" else "ship")
            assert r["donor_prompt_idx"] == r["prompt_idx"]
        else:
            assert r["donor_word"] == r["word"] and r["donor_prompt_idx"] == (r["prompt_idx"] + 1) % n_prompts
            # the donor's secret is the pair's own: the donor readouts are the secret readouts
            assert r["p_donor_max"] == r["p_secret_max"] and r["p_donor_final"] == r["p_secret_final"]
            assert abs(r["delta_p_donor"] - (r["p_secret_mean"] - r["p_secret_mean_base"])) < 1e-6
        assert 0.0 <= r["p_donor_mean"] <= r["p_donor_max"] <= 1.0
        assert isinstance(r["donor_leak"], bool) and isinstance(r["donor_in_topk"], bool)
    assert runner._plan.has_swap == (True, True) and runner._plan.donor.shape[0] == runner.B * 4


def test_default_methods_are_untouched(sweeps):
    from taboo_brittleness_amd.pipelines.sweep import METHODS, NOISE_METHODS, SWAP_METHODS

    assert METHODS == DEFAULT and NOISE_METHODS == ("sae_noise", "proj_noise") and SWAP_METHODS == SWAP
    got, runner = sweeps["default"]
    assert runner._plan.donor is None and runner._plan.has_swap == (False, False)
    assert runner._plan.idx.shape[1] == 4                       # max(budgets): no room for a second latent set
    keys = None
    for donor in ("next_word", "next_prompt"):
        both = sweeps[donor, "reuse"][0]
        for k, r in got.items():
            assert r == both[k], k                               # decoy_probs included
            assert not [f for f in r if f.startswith("donor") or f.startswith("p_donor") or f == "delta_p_donor"]
            assert len(r["decoy_probs"]) == 3
            keys = keys or set(r)
        for k, r in both.items():
            assert set(r) - keys == (set(DONOR_STATS) | {"donor_word", "donor_prompt_idx", "donor_leak",
                                                         "donor_in_topk"} if k[2] in SWAP else set()), k
            assert len(r["decoy_probs"]) == 3


# ------------------------------------------------------------------------------------- files and entry points
RUN = OVR + TWO_WORDS


def test_run_sweep_swap_files_and_report(tmp_path):
    from taboo_brittleness_amd.cli.run_sweep import METHOD_SETS
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.report.figures import make_report

    results = tmp_path / "results"
    out = str(results / "sweeps" / "swap")
    summ = run_sweep(load_config(None, RUN), out, METHOD_SETS["swap"], info=DistInfo(), log=lambda *a: None)
    disk = json.load(open(os.path.join(out, "sweep_summary.json")))
    assert disk["config"]["swap_donor"] == "next_word" and summ["config"]["swap_donor"] == "next_word"
    assert disk["swap_skipped"] == []
    by = {(c["method"], c["budget"]): c for c in disk["curves"]}
    for meth in SWAP:
        for b in (1, 2):
            c = by[(meth, b)]
            for f in ("p_donor_mean", "delta_p_donor"):
                assert set(c[f]) >= {"mean", "lo", "hi"} and c[f]["lo"] <= c[f]["mean"] <= c[f]["hi"]
            assert 0.0 <= c["donor_leak_rate"] <= 1.0 and 0.0 <= c["donor_topk_rate"] <= 1.0
    assert all("p_donor_mean" not in c for k, c in by.items() if k[0] not in SWAP)
    lines = open(os.path.join(out, "swap_curves.csv")).read().splitlines()
    assert lines[0].startswith("method,budget,n,p_secret_mean,delta_p,p_donor_mean") and len(lines) == 1 + 8
    cells = [json.loads(l) for l in open(os.path.join(out, "sweep_cells.jsonl"))]
    assert all(("donor_word" in c) == (c["method"] in SWAP) for c in cells)
    # 4 pairs x (default 10 + sae_swap 2 + sae_swap_random 4 + proj_swap 2 + proj_swap_random 2)
    assert len(cells) == 4 * 20
    made = make_report(str(results), str(tmp_path / "report"))
    figs = [p for p in made if os.path.basename(p).startswith("fig4_interchange")]
    assert len(figs) == 1 and os.path.getsize(figs[0]) > 0
    # a sweep without the swap methods: no such file, no such figure, the curves file keeps its header
    plain = str(results / "sweeps" / "plain")
    s2 = run_sweep(load_config(None, RUN), plain, info=DistInfo(), log=lambda *a: None)
    assert not os.path.exists(os.path.join(plain, "swap_curves.csv"))
    assert "swap_donor" not in s2["config"] and "swap_skipped" not in s2
    assert open(os.path.join(plain, "sweep_curves.csv")).readline().strip() == \
        "method,budget,n,p_secret_mean,p_lo,p_hi,delta_p,delta_nll,leak_rate,ll_accuracy,ll_pass10,ll_majority"
    made = make_report(str(results), str(tmp_path / "report2"))
    assert len([p for p in made if os.path.basename(p).startswith("fig4_interchange")]) == 1     # the swap sweep's only
    # the default records of the swap run are those of the plain run
    pc = {c["cell_id"]: c for c in map(json.loads, open(os.path.join(plain, "sweep_cells.jsonl")))}
    dflt = [c for c in cells if c["method"] not in SWAP]
    assert len(dflt) == len(pc)
    strip = lambda c: {k: v for k, v in c.items() if k != "cell_id"}          # noqa: E731
    assert sorted(map(json.dumps, map(strip, dflt))) == sorted(map(json.dumps, map(strip, pc.values())))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir, q):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    torch.set_num_threads(2)
    from taboo_brittleness_amd.parallel import dist as D
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep

    info = D.init_distributed("gloo", "cpu")
    run_sweep(load_config(None, RUN), out_dir, ("sae_swap", "proj_swap"), info=info, log=lambda *a: None)
    D.barrier(info)
    D.destroy(info)
    q.put(rank)


def test_swap_sweep_single_and_two_rank_gloo_agree(tmp_path):
    """One rank against two: the donors of rank 0's pairs are baselined on rank 1 and reach it through
    ``share_baselines``.  The swap records agree field by field (floats to the reuse test's tolerances)."""
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep

    def cells(d):
        return {r["cell_id"]: r for r in map(json.loads, open(os.path.join(d, "sweep_cells.jsonl")))}

    one = str(tmp_path / "dp1")
    run_sweep(load_config(None, RUN), one, ("sae_swap", "proj_swap"), info=DistInfo(), log=lambda *a: None)
    c1 = cells(one)
    assert len(c1) == 4 * 4
    two = str(tmp_path / "dp2")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, two, q)) for r in range(2)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(timeout=600)
        assert p.exitcode == 0
    c2 = cells(two)
    assert set(c1) == set(c2)
    for k in c1:
        a, b = c1[k], c2[k]
        assert set(a) == set(b)
        for f in a:
            if isinstance(a[f], float):
                assert a[f] == b[f] or abs(a[f] - b[f]) < 1e-6 + 1e-5 * abs(a[f]), (k, f)
            elif f != "decoy_probs":
                assert a[f] == b[f], (k, f)


def test_cli_accepts_the_swap_method_sets(tmp_path):
    from taboo_brittleness_amd.cli import run_sweep as cli

    S = cli.METHOD_SETS
    assert S["sae_swap"] == S["sae"] + ("sae_swap", "sae_swap_random")
    assert S["proj_swap"] == S["proj"] + ("proj_swap", "proj_swap_random")
    assert S["swap"] == S["all"] + SWAP and S["all"] == DEFAULT
    sets = [a for o in RUN + ["intervention.budgets=[1]", "intervention.ranks=[1]", "intervention.random_trials=1",
                              "intervention.swap_donor=next_prompt"] for a in ("--set", o)]
    for name in ("sae_swap", "proj_swap", "swap"):
        summ = cli.main(sets + ["--methods", name, "--out", str(tmp_path / name)])
        assert {c["method"] for c in summ["curves"]} == set(S[name])
        assert summ["config"]["swap_donor"] == "next_prompt"
        assert os.path.exists(os.path.join(str(tmp_path / name), "swap_curves.csv"))
    with pytest.raises(SystemExit):
        cli.main(sets + ["--methods", "interchange", "--out", str(tmp_path / "bad")])
