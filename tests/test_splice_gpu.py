"""Reconstruct-mode SAE ablation on the MI355X: the ``sae_splice_edit`` and ``flag_compact`` kernels against their
references, batch invariance of encode + splice, the reconstruct hook inside a captured decode graph, and the
sweep's per-pair activation table against fresh encodes."""
from dataclasses import replace
from types import SimpleNamespace

import pytest
import torch

from taboo_brittleness_amd import ops
from taboo_brittleness_amd.models.gemma2 import Gemma2Model
from taboo_brittleness_amd.models.spec import GEMMA2_TINY
from taboo_brittleness_amd.models.weights import random_gemma2
from taboo_brittleness_amd.ops import reference as ref
from test_engine_gpu import _assert_records_equal, tb_gemm  # noqa: F401  (fixture)
from test_splice_cpu import _close, dense_fp64, splice_case

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SPEC = replace(GEMMA2_TINY, vocab_size=2048, layers=4, sliding_window=8)


@pytest.mark.parametrize("D", [512, 3584])
@pytest.mark.parametrize("table", [torch.float32, BF])
def test_sae_splice_edit_matches_reference(gpu, D, table):
    """Every row class of ``splice_case`` (unflagged, pure splice, cnt = mmax, inactive ablated latent, everything
    ablated, nothing active, ~1100 active latents, a shared table row) at alpha 1 and 0.5, fp32 and bf16 W_dec.
    Tolerances: those of test_lowrank_edit_sae_and_projection for the same fp32-sum -> bf16 -> RMSNorm chain."""
    c = splice_case(D)
    Wd = c["Wd"].to(table)
    g = {k: v.to(gpu) for k, v in c.items()}
    for alpha in (1.0, 0.5):
        for bd in (c["bd"], None):
            hr, xr = c["h"].clone(), c["x"].clone()
            ref.sae_splice_edit(hr, c["apply"], c["acts"], c["idx"], c["cnt"], Wd, bd, alpha, c["wn"], 1e-6, xr,
                                c["src"])
            hg, xg = g["h"].clone(), g["x"].clone()
            ops.sae_splice_edit(hg, g["apply"], g["acts"], g["idx"], g["cnt"], Wd.to(gpu),
                                bd.to(gpu) if bd is not None else None, alpha, g["wn"], 1e-6, xg, g["src"])
            hg, xg = hg.cpu(), xg.cpu()
            assert torch.equal(hg[0], c["h"][0]) and torch.equal(xg[0], c["x"][0])     # unflagged: bit-unchanged
            _close(hg, hr, 3e-2, 1e-2)
            _close(xg, xr, 3e-2, 1e-2)
            want_h, want_x = dense_fp64(c, Wd, bd, alpha)
            _close(hg[1:], want_h[1:], 3e-2, 1e-2)
            _close(xg[1:], want_x[1:], 3e-2, 1e-2)
            zero = torch.zeros(D, dtype=BF)
            assert torch.equal(hg[5], bd.to(BF) if bd is not None else zero)            # no active latent
            if alpha == 1.0:
                assert torch.equal(hg[4], bd.to(BF) if bd is not None else zero)        # every active one ablated
            if bd is None:
                assert torch.equal(xg[5], zero)                                         # zeros in, no NaN out
            assert not torch.equal(hg[7], hg[8])                                        # one table row, two cells


def test_sae_splice_edit_src_row_out_of_table_and_limits(gpu):
    """A flagged row whose ``src_row`` points outside the activation table is left alone (never read out of
    bounds); row widths the kernel cannot cover fail loudly, as ``lowrank_edit`` does."""
    c = splice_case(512)
    g = {k: v.to(gpu) for k, v in c.items()}
    src = g["src"].clone()
    src[2], src[3] = -1, 12
    h, x = g["h"].clone(), g["x"].clone()
    ops.sae_splice_edit(h, g["apply"], g["acts"], g["idx"], g["cnt"], g["Wd"], g["bd"], 1.0, g["wn"], 1e-6, x, src)
    for r in (0, 2, 3):
        assert torch.equal(h[r], g["h"][r]) and torch.equal(x[r], g["x"][r])
    assert not torch.equal(h[1], g["h"][1])
    for D in (8200, 12):
        hh = torch.zeros(2, D, dtype=BF, device=gpu)
        with pytest.raises(RuntimeError):
            ops.sae_splice_edit(hh, torch.ones(2, dtype=torch.uint8, device=gpu), torch.zeros(2, 4, device=gpu),
                                torch.zeros(2, 1, dtype=torch.int32, device=gpu),
                                torch.zeros(2, dtype=torch.int32, device=gpu), torch.zeros(4, D, device=gpu))


@pytest.mark.parametrize("case", ["zeros", "ones", "last", "ragged"])
def test_flag_compact(gpu, case):
    n = {"zeros": 700, "ones": 1024, "last": 2049, "ragged": 3001}[case]      # 1024-thread workgroup: 3001 is ragged
    f = torch.zeros(n, dtype=torch.uint8)
    if case == "ones":
        f[:] = 1
    elif case == "last":
        f[-1] = 1
    elif case == "ragged":
        f[torch.randperm(n, generator=torch.Generator().manual_seed(1))[:137]] = 1
        f[-1] = 1
    nz = torch.nonzero(f).flatten().int()
    cap = nz.numel() + 5
    inv = torch.full((n,), 7, dtype=torch.int32, device=gpu)
    rows = ops.flag_compact(f.to(gpu), cap, inv=inv).cpu()
    assert sorted(rows[rows >= 0].tolist()) == nz.tolist() and int((rows == -1).sum()) == cap - nz.numel()
    inv = inv.cpu()
    assert torch.equal(torch.nonzero(inv >= 0).flatten().int(), nz)
    assert torch.equal(rows[inv[nz.long()].long()], nz) and bool((inv[f == 0] == -1).all())
    # a capacity below the flag count drops flags, in range
    if nz.numel() > 3:
        small = ops.flag_compact(f.to(gpu), 3).cpu()
        assert set(small.tolist()) <= set(nz.tolist()) and len(set(small.tolist())) == 3


@pytest.mark.parametrize("D,L", [(512, 1024), (3584, 16384)])
def test_encode_splice_batch_invariance(gpu, tb_gemm, D, L):
    """encode + splice of one residual row: bit-equal h and x_next alone, as row 13 of 17, as row 250 of 300, and
    through ``flag_compact`` from a [B, T] layout with scattered flags (one encode kernel family at every M)."""
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE

    sae = JumpReLUSAE.random(D, L, seed=4, device=gpu, target_l0=40.0)
    g = torch.Generator().manual_seed(9)
    wn = (torch.randn(D, generator=g) * 0.1).to(BF).to(gpu)
    row = torch.randn(1, D, generator=g).to(BF)
    mmax = 4
    acts1 = sae.encode(row.to(gpu))
    active = torch.nonzero(acts1[0]).flatten()
    assert active.numel() >= 2
    sel = torch.tensor([[int(active[0]), int(active[-1]), 3, 0]], dtype=torch.int32)

    def run(h_all, at, flags=None):
        M = h_all.shape[0]
        h, x = h_all.clone().to(gpu), torch.zeros(M, D, dtype=BF, device=gpu)
        apply = torch.zeros(M, dtype=torch.uint8)
        apply[at] = 1
        if flags is not None:
            apply = flags
        idx = sel.repeat(M, 1).to(gpu)
        cnt = torch.full((M,), 3, dtype=torch.int32, device=gpu)
        apply = apply.to(gpu)
        if flags is None:
            ops.sae_splice_edit(h, apply, sae.encode(h), idx, cnt, sae.W_dec, sae.b_dec, 1.0, wn, 1e-6, x)
        else:
            cap = int(flags.sum()) + 2
            inv = torch.empty(M, dtype=torch.int32, device=gpu)
            rows = ops.flag_compact(apply, cap, inv=inv)
            acts = sae.encode(h.index_select(0, rows.clamp_min(0).long()))
            ops.sae_splice_edit(h, apply, acts, idx, cnt, sae.W_dec, sae.b_dec, 1.0, wn, 1e-6, x, inv)
        return h[at].cpu(), x[at].cpu()

    h1, x1 = run(row, 0)
    assert not torch.equal(h1, row[0])
    for M, at in ((17, 13), (300, 250)):
        h_all = torch.randn(M, D, generator=g).to(BF)
        h_all[at] = row[0]
        hm, xm = run(h_all, at)
        assert torch.equal(hm, h1) and torch.equal(xm, x1), (M, at)
    B, T, at = 6, 37, 4 * 37 + 11
    h_all = torch.randn(B * T, D, generator=g).to(BF)
    h_all[at] = row[0]
    flags = (torch.rand(B * T, generator=g) < 0.1).to(torch.uint8)
    flags[at] = 1
    hc, xc = run(h_all, at, flags)
    assert torch.equal(hc, h1) and torch.equal(xc, x1)


def _models(gpu, **kw):
    return Gemma2Model(random_gemma2(SPEC, dtype=BF, seed=5, norm_std=0.1, device=gpu, **kw), gpu)


def test_reconstruct_hook_graph_decode_equals_eager(gpu, tb_gemm):
    """A captured-and-replayed decode with the reconstruct hook (full-bucket encode + splice inside the graph,
    compacted encode in the prefill) equals the eager one, and the edit is not a no-op."""
    from taboo_brittleness_amd.interp.edits import EditHook, EditPlan
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.runtime.generation import Generator

    mg = _models(gpu)
    sae = JumpReLUSAE.random(SPEC.hidden, 1024, seed=2, device=gpu)
    prompts = [[2, 5, 9, 11, 13], [2, 7, 8], [2, 3, 4, 5, 6, 7, 8]]
    plan = EditPlan.build(gpu, [[3, 6, 9], [4, 5], [], []], ["sae", "sae", "none", "none"],
                          [[5, 9, 100], [], [], []], mode="reconstruct")
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
    assert not torch.equal(plain.tok_nll[:2, :10], eager.tok_nll[:2, :10])


def test_sweep_gpu_reconstruct_reuse_is_exact(gpu, tb_gemm):
    """Reconstruct mode: every cell from scratch (prefix_share off: every flagged row encoded fresh, in prefills
    through the compaction and in decode buckets) against all reuse levels (the teacher-forced tail splicing from
    the per-pair activation table, diverged cells encoding fresh in the trie decode).  Float aggregates to 1e-6
    relative: the NLL summation order differs as in test_sweep_gpu_prefix_share_equivalence."""
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner

    cfg = load_config(None, ["experiment.max_new_tokens=12", "intervention.budgets=[1, 4]",
                             "intervention.random_trials=2", "intervention.ablation_mode=reconstruct"])
    mg = _models(gpu, post_norm_gain=8.0)
    tok = SyntheticTokenizer(vocab_size=SPEC.vocab_size)
    key = lambda r: (r["word"], r["prompt_idx"], r["method"], r["budget"], r["trial"])   # noqa: E731
    out, stats = {}, {}
    for name, kw, skip in (("scratch", dict(prefix_share=False, layer_resume=False), True),
                           ("reuse", dict(prefix_share=True, layer_resume=True), True),
                           ("reuse_noskip", dict(prefix_share=True, layer_resume=True), False)):
        sae = JumpReLUSAE.random(SPEC.hidden, 1024, seed=2, device=gpu)
        r = SweepRunner(cfg, mg, tok, sae, batch=96, device=gpu, layer=2, kv_pairs=8, **kw)
        r.skip_noop_spikes = skip
        pairs = r.build_pairs(["ship"], cfg.prompts[:4])
        r.run_baselines(pairs)
        res = r.run_cells(pairs, r.make_cells(pairs, ("sae_targeted", "sae_random")))
        out[name] = {key(x): x for x in res}
        stats[name] = dict(r.stats)
    print({n: {k: s[k] for k in ("cells", "diverged", "tf_rows", "splice_table_rows", "splice_decode_rows")}
           for n, s in stats.items()})
    assert sum(k[2] == "sae_splice" for k in out["reuse"]) == 4
    # both activation sources were exercised (host-known: each cell's divergence point against its plan's spikes)
    assert stats["reuse"]["splice_table_rows"] > 0, stats["reuse"]
    assert stats["reuse"]["splice_decode_rows"] > 0, stats["reuse"]
    assert stats["scratch"]["splice_table_rows"] == 0
    _assert_records_equal(out["scratch"], out["reuse"], float_rtol=1e-6)
    assert stats["reuse"]["tf_rows"] == stats["reuse_noskip"]["tf_rows"] > 0
    _assert_records_equal(out["reuse"], out["reuse_noskip"])
