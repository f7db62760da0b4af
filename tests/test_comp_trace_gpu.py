"""Component trace on the MI355X: ``ops.seg_dots`` (csrc/comp_trace.hip) against the derived criterion of
tests/comp_trace_cases.py at every shape, exact zeros for skipped rows and the zero segment, the independence of a
row's bits from the launch around it, the inputs that raise, and ``ComponentHook`` on the tiny model in GEMM mode
``tb``: every number against the CPU path's criterion on the captured rows, the same bits whether the rows run as one
chunk or two, nothing launched without the hook, and a refusal outside mode ``tb``."""
from dataclasses import replace

import pytest
import torch

from comp_trace_cases import EPS, SEG_M, SEG_SHAPES, SEG_U, check_seg, run_seg, seg_case, seg_truth
from taboo_brittleness_amd import ops
from taboo_brittleness_amd.models.gemma2 import Gemma2Model, packed_blocks
from taboo_brittleness_amd.models.spec import GEMMA2_TINY
from taboo_brittleness_amd.models.weights import random_gemma2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SPEC = replace(GEMMA2_TINY, vocab_size=2048, layers=4, sliding_window=8)      # as in tests/test_layer_trace_gpu.py
IDS = lambda s: f"K{s[0]}-S{s[1]}-Dn{s[2]}"                                    # noqa: E731


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("shape", SEG_SHAPES, ids=IDS)
def test_kernel_meets_the_criterion(gpu, shape):
    """T in {1, 2, 4}, Ms in {1, 5, 257} with unsorted, repeated and out-of-range rows and blocks, with and without
    ``R``, NaN-filled outputs: every element and every ``rms`` within its bound, skipped rows and the zero table
    segment exactly +0.0."""
    K, S, Dn = shape
    bad = run_seg(ops.seg_dots, gpu, K, S, Dn)
    assert not bad, bad[:6]


@pytest.mark.parametrize("shape", ((1024, 4, 512), (4096, 16, 3584)), ids=IDS)
@pytest.mark.parametrize("T", (1, 2, 4))
def test_row_bits_do_not_depend_on_the_launch(gpu, shape, T):
    """One source row against one table block: launched alone, as selected row 130 of 257, with its neighbours' ``blk``
    changed, with its neighbours skipped, and as the last selected row: the same bits each time, ``rms`` too."""
    K, S, Dn = shape
    X, W, _, _, R = seg_case(K, S, Dn, T, 257, seed=7)
    X, W, R = X.to(gpu), W.to(gpu), R.to(gpu)
    g = torch.Generator().manual_seed(11)
    rows = torch.randint(0, SEG_M, (257,), generator=g).to(torch.int32).to(gpu)
    src = int(rows[130])
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=gpu)            # noqa: E731
    for Rr in (R, None):
        for u in range(SEG_U):
            alone, q1 = ops.seg_dots(X, W, i32([src]), i32([u]), S, Rr, EPS)
            same = torch.full((257,), u, dtype=torch.int32, device=gpu)
            runs = {"middle of 257": (rows, same, 130)}
            for nb in ([129], [131], [128, 129, 131], list(range(112, 130)) + list(range(131, 160))):
                b = same.clone()
                b[nb] = i32([(u + 1 + i) % (SEG_U + 2) - 1 for i in range(len(nb))])   # other blocks, -1 and U
                runs[f"blk changed at {nb[:3]}"] = (rows, b, 130)
                r = rows.clone()
                r[nb] = i32([-1 if i % 2 else SEG_M for i in range(len(nb))])
                runs[f"rows skipped at {nb[:3]}"] = (r, same, 130)
            r = rows.clone()
            r[256] = src
            runs["last row"] = (r, same, 256)
            for name, (r, b, at) in runs.items():
                out, q = ops.seg_dots(X, W, r, b, S, Rr, EPS)
                assert torch.equal(_bits(out[at]), _bits(alone[0])), (Rr is None, u, name)
                assert torch.equal(_bits(q[at]), _bits(q1[0])), (Rr is None, u, name, "rms")


def test_unsupported_inputs_raise(gpu):
    X = torch.zeros(4, 64, dtype=BF, device=gpu)
    W = torch.zeros(2, 2, 64, device=gpu)
    rows = torch.arange(4, dtype=torch.int32, device=gpu)
    blk = torch.zeros(4, dtype=torch.int32, device=gpu)
    out, rms = ops.seg_dots(X, W, rows, blk, 8, X, EPS)
    assert out.shape == (4, 2, 8) and not _bits(out).any()               # zero rows: exactly +0.0
    assert torch.equal(rms.cpu(), torch.full((4,), EPS).double().sqrt().float())
    z = lambda *s, **k: torch.zeros(*s, device=gpu, **k)                 # noqa: E731
    for bad in (dict(W=W.cpu()), dict(rows=rows.long()), dict(blk=blk.long()), dict(blk=blk[:3]),
                dict(W=W[:, :, :32].contiguous()), dict(X=X.float()), dict(W=z(2, 5, 64)), dict(W=z(2, 0, 64)),
                dict(S=0), dict(S=65), dict(S=3), dict(S=16), dict(R=X.float()), dict(R=X[:3]), dict(R=X.cpu()),
                dict(R=z(4, 60, dtype=BF)), dict(R=z(4, 4104, dtype=BF)),
                dict(X=z(4, 60, dtype=BF), W=z(2, 2, 60), S=1), dict(X=z(4, 4104, dtype=BF), W=z(2, 2, 4104), S=1),
                dict(out=z(4, 8, 2)), dict(rms=z(3))):
        with pytest.raises(ValueError):
            ops.seg_dots(bad.get("X", X), bad.get("W", W), bad.get("rows", rows), bad.get("blk", blk),
                         bad.get("S", 8), bad.get("R", X), EPS, out=bad.get("out"), rms=bad.get("rms"))
    e = ops.seg_dots(X, W, rows[:0], blk[:0], 8, X, EPS)
    assert e[0].numel() == 0 and e[1].numel() == 0
    none = ops.seg_dots(X, W[:0], rows, blk, 8, X, EPS)                  # U = 0: every block is out of range
    assert not _bits(none[0]).any() and not _bits(none[1]).any()


# -------------------------------------------------------------------------------------------------- hook on the model
class _Grab:
    def __init__(self, ws):
        self.ws, self.h, self.sub = ws, {}, {}

    def __call__(self, h, x, ctx):
        self.h[ctx.layer] = h.detach().reshape(-1, h.shape[-1]).clone()

    def on_sub(self, kind, inp, o, ctx):
        self.sub[(kind, ctx.layer)] = (inp.detach().clone(), o.detach().clone())


@pytest.fixture(scope="module")
def hooked(gpu):
    """The tiny model in GEMM mode ``tb``: a packed forward of three sequences (40 rows) with ``ComponentHook`` at
    hooked layer 1 over 9 selected rows of two table blocks, once as one chunk and once as two chunks of the same
    sequences, a grab of the rows each number is made of, and a forward without the hook under a spy."""
    from taboo_brittleness_amd.interp.edits import ComponentHook, component_tables
    from taboo_brittleness_amd.runtime import gemm_dispatch as GD

    old = GD.mode()
    GD.set_mode("tb")
    try:
        m = Gemma2Model(random_gemma2(SPEC, dtype=BF, seed=5, norm_std=0.1, device=gpu, post_norm_gain=8.0), gpu)
        s, ls = m.spec, m.lspec
        L0 = 1
        tabs = [component_tables(m, L0, ids, 2) for ids in ([5, 17], [41])]
        A = torch.stack([t[0] for t in tabs], 1).contiguous()
        F = torch.stack([t[1] for t in tabs], 1).contiguous()
        Vd = torch.stack([t[2] for t in tabs], 0).contiguous()
        lens = [17, 12, 11]
        g = torch.Generator().manual_seed(3)
        toks = torch.randint(0, s.vocab_size, (sum(lens),), generator=g).to(torch.int32).to(gpu)
        sel = torch.tensor([1, 4, 16, 17, 20, 28, 29, 38, 39], dtype=torch.int32, device=gpu)
        sblk = torch.tensor([0, 0, 0, 1, 1, 1, 0, 0, 0], dtype=torch.int32, device=gpu)
        rpb = 16 // (ls.heads // ls.kv_heads)
        real, n = ops.seg_dots, [0]

        def spy(*a, **kw):
            n[0] += 1
            return real(*a, **kw)

        def run(chunks, hook=True):
            hk = ComponentHook(A, F, Vd, sel, sblk, L0, ls.heads, s.eps)
            grabs = []
            cache = m.new_cache(3, 24)
            for seqs in chunks:                                          # seqs: indices of the chunk's sequences
                r0 = sum(lens[: seqs[0]])
                nrow = sum(lens[i] for i in seqs)
                pos = torch.cat([torch.arange(lens[i], dtype=torch.int32) for i in seqs]).to(gpu)
                sr = torch.cat([torch.full((lens[i],), i, dtype=torch.int32) for i in seqs]).to(gpu)
                off, table = 0, []
                for i in seqs:
                    table.append((off, lens[i], i))
                    off += lens[i]
                ws = m.workspace(nrow)
                gr = _Grab(ws)
                hk.use_rows(r0, r0 + nrow)
                hooks = {L0: [gr, hk], s.layers - 1: [gr, hk]} if hook else None
                sub = {l: [gr.on_sub, hk.sub] for l in hk.layers} if hook else None
                m.forward_packed(toks[r0:r0 + nrow], pos, sr, packed_blocks(table, rpb).to(gpu), cache, hooks=hooks,
                                 ws=ws, sub_hooks=sub)
                grabs.append((r0, gr))
            torch.cuda.synchronize()
            return hk, grabs

        one = run([[0, 1, 2]])
        two = run([[0, 1], [2]])
        ops.seg_dots = spy
        try:
            off = run([[0, 1, 2]], hook=False)
        finally:
            ops.seg_dots = real
        GD.set_mode("auto")
        refused = None
        try:
            run([[0, 1, 2]])
        except ValueError as e:
            refused = str(e)
        return dict(m=m, one=one, two=two, off=off, spied=n[0], refused=refused, sel=sel.cpu().tolist(),
                    sblk=sblk.cpu().tolist(), A=A, F=F, Vd=Vd, L0=L0)
    finally:
        GD.set_mode(old)


def test_hook_numbers_meet_the_criterion_on_the_models_own_rows(hooked):
    """Every slab of the hook against the float64 truth of ``seg_dots`` on the rows the model showed it: the direct
    term, each head and each MLP of blocks 2 and 3, and ``z_pre`` with ``rho_f``; a pair without a donor has an
    exactly zero column 1; the numbers are not all small."""
    hk, grabs = hooked["one"]
    r0, gr = grabs[0]
    m, L0 = hooked["m"], hooked["L0"]
    heads, eps = m.lspec.heads, m.spec.eps
    rows = torch.tensor(hooked["sel"], dtype=torch.int32)
    blk = torch.tensor(hooked["sblk"], dtype=torch.int32)
    cpu = lambda t: t.detach().cpu()                                      # noqa: E731
    Vd = cpu(hooked["Vd"])
    t = seg_truth(cpu(gr.h[L0]), Vd, rows, blk, 1, None, eps)
    bad = check_seg(hk.direct[:, :, None], t["rho"].float(), t, "direct")
    hl = cpu(gr.h[m.spec.layers - 1])
    t = seg_truth(hl, Vd, rows, blk, 1, hl, eps)
    bad += check_seg(hk.total[:, :, None], hk.rho_f, t, "total")
    for k, l in enumerate(hk.layers):
        a, o = (cpu(x) for x in gr.sub[("attn", l)])
        t = seg_truth(a, cpu(hooked["A"][k]), rows, blk, heads, o, eps)
        bad += check_seg(hk.comp[k, :, :, :heads].contiguous(), t["rho"].float(), t, f"attn {l}")
        assert float(t["z"].abs().max()) > 100 * float(t["bound"].max())
        _, d = (cpu(x) for x in gr.sub[("ffn", l)])
        t = seg_truth(d, cpu(hooked["F"][k]), rows, blk, 1, d, eps)
        bad += check_seg(hk.comp[k, :, :, heads:].contiguous(), t["rho"].float(), t, f"ffn {l}")
    assert not bad, bad[:6]
    solo = [i for i, u in enumerate(hooked["sblk"]) if u == 1]
    assert not _bits(hk.comp[:, solo, 1]).any() and not _bits(hk.direct[solo, 1]).any()
    assert bool(hk.comp[:, :, 0].abs().gt(1e-3).any()) and hk.calls == 2 + 4


def test_hook_bits_do_not_depend_on_the_chunking(hooked):
    """The same sequences as one chunk and as two (in-tree GEMMs and attention are batch-invariant in mode ``tb``):
    every slab bit-equal."""
    a, b = hooked["one"][0], hooked["two"][0]
    for name in ("direct", "comp", "total", "rho_f"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert b.calls == 2 * (2 + 4)


def test_without_the_hook_nothing_is_launched_and_other_modes_refuse(hooked):
    assert hooked["spied"] == 0 and hooked["off"][0].calls == 0
    assert hooked["refused"] is not None and "tb" in hooked["refused"]


# -------------------------------------------------------------------------------------------------- sweep
METHODS = ("sae_targeted", "sae_random", "proj_targeted")
MATS = ("comp_dz_spike", "comp_dz_next", "comp_base_spike")
DELTAS = ("comp_dz_spike", "comp_dz_next")
CKEYS = MATS + ("comp_attn_dz_spike", "comp_mlp_dz_spike", "comp_direct_dz_spike", "comp_total_dz_spike",
                "comp_top_spike")


@pytest.fixture(scope="module")
def comp_sweeps(gpu):
    """The tiny-model sweep of tests/test_layer_trace_gpu.py (in-tree GEMMs: batch-invariant) at hooked layer 1, so
    two later blocks exist, with ``intervention.component_trace`` at every reuse level switched one at a time, an
    all-no-op run forced through the tail, the layer trace beside it and alone, and a run without the switch -- each
    under a spy on ``ops.seg_dots``; computed once."""
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from taboo_brittleness_amd.runtime import gemm_dispatch as GD

    old = GD.mode()
    GD.set_mode("tb")
    base = ["experiment.max_new_tokens=12", "intervention.budgets=[1, 4]", "intervention.ranks=[1, 4]",
            "intervention.random_trials=2", "intervention.proj_random_trials=1"]
    ct, lt = ["intervention.component_trace=true"], ["intervention.layer_trace=true"]
    mg = Gemma2Model(random_gemma2(SPEC, dtype=BF, seed=5, norm_std=0.1, device=gpu, post_norm_gain=8.0), gpu)
    tok = SyntheticTokenizer(vocab_size=SPEC.vocab_size)
    key = lambda r: (r["word"], r["prompt_idx"], r["method"], r["budget"], r["trial"])   # noqa: E731
    out, runners, calls = {}, {}, {}
    real = ops.seg_dots
    try:
        for name, extra, flags in (("default", ct, {}), ("no_skip", ct, dict(skip_noop_spikes=False)),
                                   ("no_trie", ct, dict(trie_decode=False)), ("no_dedup", ct, dict(_no_dedup=True)),
                                   ("noop", ct + ["intervention.alpha=0.0"], dict(skip_noop_spikes=False)),
                                   ("with_trace", ct + lt, {}), ("trace_only", lt, {}), ("switch_off", [], {})):
            cfg = load_config(None, base + extra)
            sae = JumpReLUSAE.random(SPEC.hidden, 1024, seed=2, device=gpu)
            r = SweepRunner(cfg, mg, tok, sae, batch=64, device=gpu, layer=1, kv_pairs=8)
            for k, v in flags.items():
                if k == "_no_dedup":                     # lens rows one by one, the trie decode still on
                    r._lens_row_keys = lambda *a, **kw: None
                else:
                    setattr(r, k, v)
            n = [0]

            def spy(*a, _n=n, **kw):
                _n[0] += 1
                return real(*a, **kw)

            ops.seg_dots = spy
            methods = ("sae_targeted",) if name == "noop" else METHODS
            pairs = r.build_pairs(["ship"], cfg.prompts[:3], methods)
            r.run_baselines(pairs)
            res = r.run_cells(pairs, r.make_cells(pairs, methods))
            out[name] = {key(x): x for x in res}
            runners[name] = (r, pairs)
            calls[name] = n[0]
    finally:
        ops.seg_dots = real
        GD.set_mode(old)
    return out, runners, calls


def test_sweep_fields_are_bit_equal_across_reuse_levels(comp_sweeps):
    """The no-op spike skip, the prefix-trie decode and the lens row dedup change which rows share a launch, never a
    row's bits: the component fields are equal as floats, bit for bit."""
    out, runners, calls = comp_sweeps
    ref_ = out["default"]
    st = runners["default"][0].stats
    assert st["tf_rows"] > 0 and st["diverged"] > 0 and calls["default"] > 0 and st["comp_rows"] > 0
    assert runners["no_skip"][0].stats["tf_rows"] > st["tf_rows"]              # the skip did skip rows
    for name in ("no_skip", "no_trie", "no_dedup"):
        assert set(out[name]) == set(ref_)
        for k, r in out[name].items():
            assert r["response_ids"] == ref_[k]["response_ids"], (name, k)
            for f in CKEYS:
                assert r[f] == ref_[k][f], (name, k, f, r[f], ref_[k][f])
    assert any(abs(r["comp_top_spike"][2]) > 1e-3 for r in ref_.values())
    assert all(len(r[f]) == 2 and len(r[f][0]) == SPEC.heads + 1 for r in ref_.values() for f in MATS)
    for r in ref_.values():                                                     # the parts against the total
        s = r["comp_direct_dz_spike"] + sum(v for row in r["comp_dz_spike"] for v in row)
        print(f"{r['method']} {r['budget']}: direct + parts {s:+.6f}, total {r['comp_total_dz_spike']:+.6f}")


def test_noop_cells_through_the_tail_are_exactly_zero(comp_sweeps):
    """``alpha = 0`` makes every edit an exact no-op; with the skip off the cells still run their tail from the first
    spike, in a batch of their own shape.  Its rows repeat the baseline pass's bits in every sublayer, so every
    difference is exactly 0."""
    out, runners, calls = comp_sweeps
    r_, pairs = runners["noop"]
    assert r_.stats["tf_rows"] > 0 and r_.stats["diverged"] == 0 and calls["noop"] > 0 and len(out["noop"]) == 3 * 2
    base = {(p.word, p.pidx): p for p in pairs}
    for k, r in out["noop"].items():
        assert r["response_ids"] == base[k[0], k[1]].resp
        assert all(v == 0.0 for f in DELTAS for row in r[f] for v in row), (k, [r[f] for f in DELTAS])
        assert all(v == 0.0 for f in ("comp_attn_dz_spike", "comp_mlp_dz_spike") for v in r[f])
        assert r["comp_direct_dz_spike"] == 0.0 and r["comp_total_dz_spike"] == 0.0 and r["comp_top_spike"][2] == 0.0
        assert any(v != 0.0 for row in r["comp_base_spike"] for v in row)


def test_switch_off_launches_nothing_and_keeps_the_records(comp_sweeps):
    from test_engine_gpu import FIELDS, _assert_records_equal

    out, runners, calls = comp_sweeps
    r0, pairs = runners["switch_off"]
    assert calls["switch_off"] == 0 and calls["trace_only"] == 0 and not r0.component_trace
    assert all(p.c_base is None and p.z_base is None and p.x_base is None for p in pairs)
    assert not any(k.startswith("comp_") or k.startswith("trace_") or k.startswith("shift_") for k in r0.stats)
    for k, r in out["switch_off"].items():
        assert set(out["default"][k]) - set(r) == set(CKEYS) and not set(r) - set(out["default"][k]), k
    _assert_records_equal(out["switch_off"], out["default"],
                          fields=FIELDS + ("decoy_probs", "p_secret_final", "p_secret_max", "nll_self"))


def test_layer_trace_beside_it_is_unchanged_and_shares_the_baseline_pass(comp_sweeps):
    out, runners, calls = comp_sweeps
    both, alone = runners["with_trace"][0].stats, runners["trace_only"][0].stats
    assert both["trace_base_rows"] == alone["trace_base_rows"] > 0 and both["trace_rows"] == alone["trace_rows"]
    assert both["comp_base_rows"] == runners["default"][0].stats["comp_base_rows"]
    for k, r in out["with_trace"].items():
        for f, v in r.items():
            src = out["default"][k] if f.startswith("comp_") else out["trace_only"][k]
            assert v == src[f] or (v != v and src[f] != src[f]), (k, f, v, src[f])
