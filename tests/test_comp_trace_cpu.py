"""Component trace off the GPU: the criterion of tests/comp_trace_cases.py cannot pass vacuously, ops/reference.py meets
it and planted bugs do not, ``ops.seg_dots`` validates its arguments, the kernel compiles without scratch,
``ComponentHook`` fills its slabs over chunked windows, and on ``gemma2-tiny`` (4 blocks, hooked layer 1) every head's
number against an fp64 recomputation from the captured rows and the direct term plus every component against
``z_pre`` of the last residual, within the derived completeness bound."""
import math
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

from comp_trace_cases import (EPS, MUTANTS, SEG_M, SEG_MS, SEG_SHAPES, SEG_T, SEG_U, check_seg, completeness_bound,
                              head_truth, lens_dirs, rho_of, run_seg, seg_case, seg_mutant, seg_sel, seg_truth,
                              sublayer_slack)
from taboo_brittleness_amd import ops
from taboo_brittleness_amd.ops import reference as ref

BF = torch.bfloat16
CPU = torch.device("cpu")
IDS = [lambda s: f"K{s[0]}-S{s[1]}-Dn{s[2]}"]


# ---------------------------------------------------------------------------------------------- criterion and op
@pytest.mark.parametrize("shape", SEG_SHAPES, ids=IDS[0])
def test_cases_hold_what_they_must_and_the_bound_can_fail(shape):
    """The selections are unsorted, repeated and hold every out-of-range value; the truth is far above its bound on
    most elements (a result of 0, or one not tied to the inputs, fails); skipped rows and the zero segment are
    marked."""
    K, S, Dn = shape
    for Ms in SEG_MS[1:]:
        rows, blk = seg_sel(Ms)
        r, b = rows.tolist(), blk.tolist()
        assert -1 in r and SEG_M in r and -1 in b and SEG_U in b and len(set(r)) < len(r) and r != sorted(r)
    for T in SEG_T:
        X, W, rows, blk, R = seg_case(K, S, Dn, T, 257)
        for Rr in (R, None):
            t = seg_truth(X, W, rows, blk, S, Rr, EPS)
            live = t["ok"][:, None, None] & ~t["zero"]
            assert int(live.sum()) > 200 * T * S and bool((t["bound"][live] > 0).all())
            assert float((t["z"].abs() > 10 * t["bound"])[live].double().mean()) > 0.8, (T, Rr is None)
            assert bool(t["zero"][~t["ok"]].all()) and bool((t["z"][t["zero"]] == 0).all())
            assert bool(t["zero"][(blk == 1) & t["ok"]][:, T - 1, S - 1].all())
            assert check_seg(torch.zeros(257, T, S), torch.zeros(257), t)      # all zeros is rejected


@pytest.mark.parametrize("shape", SEG_SHAPES, ids=IDS[0])
def test_reference_meets_the_criterion(shape):
    K, S, Dn = shape
    assert not run_seg(ops.seg_dots, CPU, K, S, Dn)

    def fn(X, W, rows, blk, S_, R, eps, out=None, rms=None):
        o, q = ref.seg_dots(X, W, rows, blk, S_, R, eps)
        return o.float(), q.float()
    assert not run_seg(fn, CPU, K, S, Dn, Mss=(5, 257))


@pytest.mark.parametrize("shape", SEG_SHAPES, ids=IDS[0])
def test_planted_bugs_are_rejected(shape):
    """Each stand-in fails wherever its bug can show: the dropped group, the shifted boundary, the wrong ``rho`` source
    and the missing ``eps`` at every shape with ``R``; the wrong table stride from two columns on; ``K`` for ``Dn``
    wherever the two differ.  Bugs of ``rho`` cannot show without ``R``."""
    K, S, Dn = shape
    assert not run_seg(seg_mutant(), CPU, K, S, Dn, Mss=(5, 257))        # the stand-in itself is sound
    assert set(MUTANTS) == {"drop_last", "shift", "rho_from_x", "no_eps", "t_stride", "dn_is_k"}
    for bug in ("drop_last", "shift"):
        for wr in (True, False):
            bad = run_seg(seg_mutant(bug), CPU, K, S, Dn, Mss=(5, 257), with_R=(wr,))
            assert bad and all("want exactly" not in b for b in bad), (bug, wr, bad[:2])
    for bug in ("rho_from_x", "no_eps"):
        assert run_seg(seg_mutant(bug), CPU, K, S, Dn, Mss=(5, 257), with_R=(True,)), bug
        assert not run_seg(seg_mutant(bug), CPU, K, S, Dn, Mss=(5,), with_R=(False,)), bug
    for T in SEG_T:
        bad = run_seg(seg_mutant("t_stride"), CPU, K, S, Dn, Ts=(T,), Mss=(5, 257))
        assert bool(bad) == (T > 1), (T, bad[:2])
    bad = run_seg(seg_mutant("dn_is_k"), CPU, K, S, Dn, Mss=(5, 257), with_R=(True,))
    assert bool(bad) == (K != Dn), bad[:2]


def test_op_validates_and_maps():
    X, W, rows, blk, R = seg_case(64, 8, 64, 2, 5)
    out, rms = ops.seg_dots(X, W, rows, blk, 8, R, EPS)
    assert out.dtype == torch.float32 and out.shape == (5, 2, 8) and rms.shape == (5,) and rms.dtype == torch.float32
    o64, r64 = ref.seg_dots(X, W, rows, blk, 8, R, EPS)
    assert torch.equal(out, o64.float()) and torch.equal(rms, r64.float())
    for i in (1, 2, 3, 4):                                              # blk -1, row M, blk U, row -1
        assert not out[i].any() and float(rms[i]) == 0.0
    assert out[0].all() and float(rms[0]) > 0
    o, q = torch.full((5, 2, 8), 7.0), torch.full((5,), 7.0)
    got = ops.seg_dots(X, W, rows, blk, 8, R, EPS, out=o, rms=q)
    assert got[0] is o and got[1] is q and torch.equal(o, out) and torch.equal(q, rms)
    plain, one = ops.seg_dots(X, W, rows, blk, 8, None, EPS)
    assert float(one[0]) == 1.0 and float(one[1]) == 0.0
    assert torch.equal(plain[0], ref.seg_dots(X, W, rows, blk, 8, None, EPS)[0][0].float())
    e = ops.seg_dots(X, W, rows[:0], blk[:0], 8, R, EPS)
    assert e[0].shape == (0, 2, 8) and e[1].shape == (0,)
    none = ops.seg_dots(X, W[:0], rows, blk, 8, R, EPS)                 # no table block: every row is skipped
    assert not none[0].any() and not none[1].any()
    xb = torch.zeros(4, 4104, dtype=BF)
    for bad in (dict(X=X.float()), dict(X=X[0]), dict(W=W.double()), dict(W=W[0]), dict(W=W[:, :, :32]),
                dict(W=torch.zeros(3, 5, 64)), dict(W=torch.zeros(3, 0, 64)), dict(rows=rows.long()),
                dict(blk=blk.long()), dict(blk=blk[:4]), dict(rows=rows.view(5, 1), blk=blk.view(5, 1)),
                dict(S=0), dict(S=65), dict(S=3), dict(S=16), dict(R=R.float()), dict(R=R[:5]), dict(R=R[:, :60]),
                dict(R=torch.zeros(SEG_M, 4104, dtype=BF)), dict(out=torch.zeros(5, 8, 2)),
                dict(out=torch.zeros(5, 2, 8, dtype=torch.float64)), dict(rms=torch.zeros(4)),
                dict(X=xb, W=torch.zeros(3, 2, 4104), S=1), dict(X=xb[:, :60], W=torch.zeros(3, 2, 60), S=1)):
        with pytest.raises(ValueError):
            ops.seg_dots(bad.get("X", X), bad.get("W", W), bad.get("rows", rows), bad.get("blk", blk),
                         bad.get("S", 8), bad.get("R", R), EPS, out=bad.get("out"), rms=bad.get("rms"))


def test_seg_dots_kernel_uses_no_scratch(tmp_path):
    """comp_trace.hip compiled for gfx950 with the extension's flags: the compiler's resource-usage remarks list one
    kernel per T = 1..4, each with 0 bytes of scratch, no LDS and a register count that lets several of its 256-thread
    workgroups share a CU."""
    from taboo_brittleness_amd import build as b

    hipcc = os.path.join(b.ROCM, "bin", "hipcc")
    cmd = [hipcc, f"--offload-arch={b.ARCH}", "-c", os.path.join(b.CSRC, "comp_trace.hip"), "-o",
           str(tmp_path / "comp_trace.o"), "--cuda-device-only", "-munsafe-fp-atomics", "-fPIC", "-O3", "-std=c++17",
           "-I", b.CSRC, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    mine = [x for x in blocks if "seg_dots_kernel" in x.split()[0]]
    assert len(mine) == 4, [x.split()[0] for x in blocks]
    for x in mine:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", x).group(1)) == 0, x
        assert int(re.search(r"VGPRs: (\d+)", x).group(1)) <= 128, x
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", x).group(1)) == 0, x


# ---------------------------------------------------------------------------------------------- hook
def _ctx(layer):
    return SimpleNamespace(layer=layer)


def test_component_hook_fills_its_slabs():
    """Two chunks of a launch (7 and 6 rows, each padded to 8) with 5 selected rows, hooked layer 1 of 4 blocks: every
    slab row equals the op on that row alone, whichever chunk it came in; a chunk without selected rows launches
    nothing; a block outside the hook's range and a forward of another size raise."""
    from taboo_brittleness_amd.interp.edits import ComponentHook

    heads, hd, D, T, U, L0, layers = 4, 16, 32, 2, 2, 1, 4
    g = torch.Generator().manual_seed(5)
    A = torch.randn(2, U, T, heads * hd, generator=g)
    F = torch.randn(2, U, T, D, generator=g)
    Vd = torch.randn(U, T, D, generator=g)
    sel = torch.tensor([1, 2, 6, 7, 12], dtype=torch.int32)            # launch rows, sorted
    sblk = torch.tensor([0, 0, 1, 1, 0], dtype=torch.int32)
    hk = ComponentHook(A, F, Vd, sel, sblk, L0, heads, EPS)
    assert list(hk.layers) == [2, 3] and hk.comp.shape == (2, 5, T, heads + 1) and hk.direct.shape == (5, T)
    chunks = ((0, 7), (7, 13))
    rowsets = {}
    for ci, (r0, r1) in enumerate(chunks):
        hk.use_rows(r0, r1, 8)
        h = torch.randn(8, D, generator=g).to(BF)
        rowsets[("h", L0, ci)] = h
        hk(h, None, _ctx(L0))
        for l in (2, 3):
            for kind, K in (("attn", heads * hd), ("ffn", D)):
                x, o = torch.randn(8, K, generator=g).to(BF), torch.randn(8, D, generator=g).to(BF)
                rowsets[(kind, l, ci)] = (x, o)
                hk.sub(kind, x, o, _ctx(l))
        h = torch.randn(8, D, generator=g).to(BF)
        rowsets[("h", 3, ci)] = h
        hk(h, None, _ctx(3))
    one = torch.zeros(1, dtype=torch.int32)
    for i, (r, u) in enumerate(zip(sel.tolist(), sblk.tolist())):
        ci = 0 if r < 7 else 1
        k = r - chunks[ci][0]
        ub = torch.tensor([u], dtype=torch.int32)
        want, _ = ops.seg_dots(rowsets[("h", L0, ci)][k:k + 1], Vd, one, ub, 1, None, EPS)
        assert torch.equal(hk.direct[i], want[0, :, 0]), i
        hl = rowsets[("h", 3, ci)][k:k + 1]
        want, rho = ops.seg_dots(hl, Vd, one, ub, 1, hl, EPS)
        assert torch.equal(hk.total[i], want[0, :, 0]) and torch.equal(hk.rho_f[i], rho[0]), i
        for l in (2, 3):
            x, o = rowsets[("attn", l, ci)]
            want, _ = ops.seg_dots(x[k:k + 1], A[l - 2], one, ub, heads, o[k:k + 1], EPS)
            assert torch.equal(hk.comp[l - 2, i, :, :heads], want[0]), (l, i)
            x, o = rowsets[("ffn", l, ci)]
            want, _ = ops.seg_dots(o[k:k + 1], F[l - 2], one, ub, 1, o[k:k + 1], EPS)
            assert torch.equal(hk.comp[l - 2, i, :, heads], want[0, :, 0]), (l, i)
    assert hk.calls == 2 * (2 + 4)
    hk.use_rows(8, 12, 8)                                              # no selected row in [8, 12)
    hk(torch.zeros(8, D, dtype=BF), None, _ctx(L0))
    assert hk.calls == 2 * (2 + 4)
    hk.use_rows(0, 7, 8)
    with pytest.raises(ValueError):
        hk.sub("attn", torch.zeros(8, heads * hd, dtype=BF), torch.zeros(8, D, dtype=BF), _ctx(1))
    with pytest.raises(ValueError):
        hk.sub("resid", torch.zeros(8, heads * hd, dtype=BF), torch.zeros(8, D, dtype=BF), _ctx(2))
    with pytest.raises(ValueError):
        hk(torch.zeros(5, D, dtype=BF), None, _ctx(L0))
    with pytest.raises(ValueError):
        hk(torch.zeros(8, D, dtype=BF), None, _ctx(2))
    with pytest.raises(ValueError):
        ComponentHook(A, F, Vd, sel.flip(0), sblk, L0, heads, EPS)       # selected rows must be sorted
    with pytest.raises(ValueError):
        ComponentHook(A, F[:1], Vd, sel, sblk, L0, heads, EPS)


# ---------------------------------------------------------------------------------------------- tiny model
class _Grab:
    """Clones of what the hook sites show, per block; ``ws.h`` right after a sublayer is the new residual."""

    def __init__(self, ws):
        self.ws, self.h, self.sub = ws, {}, {}

    def __call__(self, h, x, ctx):
        self.h[ctx.layer] = h.detach().reshape(-1, h.shape[-1]).clone()

    def on_sub(self, kind, inp, o, ctx):
        self.sub[(kind, ctx.layer)] = (inp.detach().clone(), o.detach().clone(), self.ws.h.detach().clone())


@pytest.fixture(scope="module")
def tiny_run():
    """gemma2-tiny (4 blocks) on the CPU: one packed forward of two sequences, 11 rows, with the component hook at
    hooked layer 1 over 6 selected rows of two table blocks (one with a donor column, one without), and a grab of
    every row the truth needs."""
    from taboo_brittleness_amd.interp.edits import ComponentHook, component_tables
    from taboo_brittleness_amd.models.gemma2 import Gemma2Model, packed_blocks
    from taboo_brittleness_amd.models.spec import GEMMA2_TINY
    from taboo_brittleness_amd.models.weights import random_gemma2

    m = Gemma2Model(random_gemma2(GEMMA2_TINY, dtype=BF, seed=7, norm_std=0.1), "cpu")
    s, ls = m.spec, m.lspec
    assert s.layers == 4 and ls.heads * ls.head_dim == 1024 and s.hidden == 512
    L0 = 1
    ids = [[5, 17], [41, None]]                                         # column 0 = secret, column 1 = donor or absent
    tabs = [component_tables(m, L0, [t for t in pair if t is not None], 2) for pair in ids]
    A = torch.stack([t[0] for t in tabs], 1).contiguous()
    F = torch.stack([t[1] for t in tabs], 1).contiguous()
    Vd = torch.stack([t[2] for t in tabs], 0).contiguous()
    toks = torch.tensor([3, 50, 12, 9, 77, 21, 8, 64, 33, 90, 2], dtype=torch.int32)
    lens = [6, 5]
    pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens])
    slot_rows = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(lens)])
    blk = packed_blocks([(0, 6, 0), (6, 5, 1)], 16 // (ls.heads // ls.kv_heads))
    sel = torch.tensor([1, 4, 5, 6, 9, 10], dtype=torch.int32)
    sblk = torch.tensor([0, 0, 0, 1, 1, 1], dtype=torch.int32)
    hk = ComponentHook(A, F, Vd, sel, sblk, L0, ls.heads, s.eps)
    hk.use_rows(0, 11)
    ws = m.workspace(11)
    g = _Grab(ws)
    hooks = {L0: [g, hk], s.layers - 1: [g, hk]}
    sub = {l: [g.on_sub, hk.sub] for l in hk.layers}
    m.forward_packed(toks, pos, slot_rows, blk, m.new_cache(2, 8), hooks=hooks, ws=ws, sub_hooks=sub)
    return SimpleNamespace(m=m, hk=hk, g=g, sel=sel.tolist(), sblk=sblk.tolist(), L0=L0, ids=ids)


def test_per_head_numbers_match_the_fp64_recomputation(tiny_run):
    """Each head's number against ``(a_head . A_head) / rho(o)`` in fp64 from the captured ``ws.attn`` row, ``W_o``,
    the bf16 ``o`` and ``ln_post_attn``; the MLP's against ``d . ((1 + ln_post_ffn) v) / rho(d)``; an absent donor
    column is exactly zero."""
    t = tiny_run
    m, hk = t.m, t.hk
    heads = m.lspec.heads
    seen = 0
    for i, (r, u) in enumerate(zip(t.sel, t.sblk)):
        for col, tid in enumerate(t.ids[u]):
            if tid is None:
                assert not hk.comp[:, i, col].any() and float(hk.direct[i, col]) == 0.0
                continue
            v = lens_dirs(m, [tid])[0]
            for k, l in enumerate(hk.layers):
                L = m.w.layers[l]
                a, o, _ = t.g.sub[("attn", l)]
                tr = head_truth(a[r], o[r], L.wo, L.ln_post_attn, v, heads, m.spec.eps)
                err = (hk.comp[k, i, col, :heads].double() - tr["c"]).abs()
                assert bool((err <= tr["bound"]).all()), (l, r, col, err.tolist(), tr["bound"].tolist())
                assert bool((tr["c"].abs() > 10 * tr["bound"]).any())
                _, d, _ = t.g.sub[("ffn", l)]
                w = ((1.0 + L.ln_post_ffn.double()) * v).float().double()
                want = float((d[r].double() * w).sum() / rho_of(d[r], m.spec.eps))
                X1 = d[r:r + 1]
                tt = seg_truth(X1, w.float()[None, None], torch.zeros(1, dtype=torch.int32),
                               torch.zeros(1, dtype=torch.int32), 1, X1, m.spec.eps)
                assert abs(float(tt["z"]) - want) <= 1e-12 * max(1.0, abs(want))
                assert abs(float(hk.comp[k, i, col, heads]) - want) <= float(tt["bound"]), (l, r, col)
                seen += 1
    assert seen == 2 * (3 * 2 + 3)


def test_direct_plus_components_is_the_last_residuals_logit(tiny_run):
    """Completeness: ``(direct + sum of components) / rho_f`` against ``z_pre = (h_last . v) / rho_f`` of the last
    block's residual, within the bound of comp_trace_cases.py: per later sublayer the three bf16 roundings and their
    fp32 riders, in fp64 from the captured rows, plus the kernel criterion of every number in the sum."""
    t = tiny_run
    m, hk = t.m, t.hk
    heads, eps = m.lspec.heads, m.spec.eps
    last = m.spec.layers - 1
    caught = 0
    for i, (r, u) in enumerate(zip(t.sel, t.sblk)):
        tid = t.ids[u][0]
        v = lens_dirs(m, [tid])[0]
        h_last = t.g.h[last][r]
        rho_f = float(rho_of(h_last, eps))
        z_pre = float((h_last.double() * v).sum()) / rho_f
        assert abs(float(hk.rho_f[i]) - rho_f) <= 1e-3 * rho_f
        one = torch.zeros(1, dtype=torch.int32)
        vt = v.float()[None, None]
        kb = [float(seg_truth(t.g.h[t.L0][r:r + 1], vt, one, one, 1, None, eps)["bound"]) / rho_f,
              float(seg_truth(h_last[None], vt, one, one, 1, h_last[None], eps)["bound"])]
        assert abs(float(hk.total[i, 0]) - z_pre) <= kb[1]
        slacks = []
        for l in hk.layers:
            L = m.w.layers[l]
            a, o, h1 = t.g.sub[("attn", l)]
            x, d, h2 = t.g.sub[("ffn", l)]
            slacks.append(sublayer_slack(o[r], L.ln_post_attn, h1[r], v, eps, attn=a[r], Wo=L.wo))
            slacks.append(sublayer_slack(d[r], L.ln_post_ffn, h2[r], v, eps))
            kb += (head_truth(a[r], o[r], L.wo, L.ln_post_attn, v, heads, eps)["bound"] / rho_f).tolist()
            w = ((1.0 + L.ln_post_ffn.double()) * v).float()[None, None]
            kb.append(float(seg_truth(d[r:r + 1], w, one, one, 1, d[r:r + 1], eps)["bound"]) / rho_f)
        total = (float(hk.direct[i, 0]) + float(hk.comp[:, i, 0].double().sum())) / float(hk.rho_f[i])
        bound = completeness_bound(slacks, kb, rho_f)
        big = float(hk.comp[:, i, 0].flatten()[hk.comp[:, i, 0].abs().argmax()]) / float(hk.rho_f[i])
        assert abs(total - z_pre) <= bound, (r, total, z_pre, bound)
        caught += abs(total - big - z_pre) > bound
    assert caught >= len(t.sel) // 2, caught       # the bound is not vacuous: the sum without its largest term fails it


# ------------------------------------------------------------------------------------------------------ sweep
COMP = ["intervention.component_trace=true"]
MATS = ("comp_dz_spike", "comp_dz_next", "comp_base_spike")
CKEYS = MATS + ("comp_attn_dz_spike", "comp_mlp_dz_spike", "comp_direct_dz_spike", "comp_total_dz_spike",
                "comp_top_spike")


def tiny4():
    """The tiny sweep model of tests/test_head_shift_cpu.py with 4 blocks, so two blocks lie behind hooked layer 1."""
    from dataclasses import replace

    from taboo_brittleness_amd.interp.sae import JumpReLUSAE
    from taboo_brittleness_amd.models.gemma2 import Gemma2Model
    from taboo_brittleness_amd.models.spec import GEMMA2_TINY
    from taboo_brittleness_amd.models.tokenizer import SyntheticTokenizer
    from taboo_brittleness_amd.models.weights import random_gemma2

    spec = replace(GEMMA2_TINY, vocab_size=1024, layers=4, hidden=256, ffn=512)
    m = Gemma2Model(random_gemma2(spec, dtype=BF, seed=7, norm_std=0.1), "cpu")
    return spec, m, SyntheticTokenizer(vocab_size=spec.vocab_size), JumpReLUSAE.random(spec.hidden, 512, seed=2,
                                                                                      device="cpu")


@pytest.fixture(scope="module")
def sweeps():
    from test_head_shift_cpu import run_tiny

    on = run_tiny(COMP, model=tiny4())
    return {"on": on, "off": run_tiny([], model=on[4])}


_GrabAll = _Grab


def _full_forward(m, r, p, b, hook=None):
    """A plain packed forward of prompt + baseline response in slot ``b`` (every row attends to the whole sequence
    before it), the edit hook of plan row ``b`` at the hooked layer, and a grab of every row the truth needs."""
    from taboo_brittleness_amd.models.gemma2 import packed_blocks

    full = p.ids + p.resp
    n = len(full)
    ws = m.new_workspace(n)
    g = _GrabAll(ws)
    last = m.spec.layers - 1
    hooks = {r.layer: ([hook] if hook is not None else []) + [g], last: [g]}
    sub = {l: [g.on_sub] for l in range(r.layer + 1, last + 1)}
    rpb = 16 // (m.lspec.heads // m.lspec.kv_heads)
    m.forward_packed(torch.tensor(full, dtype=torch.int32), torch.arange(n, dtype=torch.int32),
                     torch.full((n,), b, dtype=torch.int32), packed_blocks([(0, n, b)], rpb),
                     m.new_cache(r.B, n + 1), hooks=hooks, ws=ws, sub_hooks=sub)
    return g


def _truth(m, L0, g, n0, ids):
    """Float64 components in logit units of rows ``n0 ..`` of a grabbed forward, with each number's tolerance: the
    kernel criterion of its numerator over ``rho_f`` plus the criterion of ``rho_f`` itself."""
    from taboo_brittleness_amd.interp.edits import component_tables

    A, F, Vd = component_tables(m, L0, ids, 2)
    eps, H = m.spec.eps, m.lspec.heads
    hl = g.h[m.spec.layers - 1][n0:]
    n = hl.shape[0]
    rows, blk = torch.arange(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    tt = seg_truth(hl, Vd[None], rows, blk, 1, hl, eps)
    rho = tt["rho"]
    rel = (tt["rho_bound"] / rho)[:, None, None]
    over = lambda t: (t["z"] / rho[:, None, None],                                    # noqa: E731
                      t["bound"] / rho[:, None, None] + (t["z"] / rho[:, None, None]).abs() * rel)
    direct = over(seg_truth(g.h[L0][n0:], Vd[None], rows, blk, 1, None, eps))
    comp, ctol = [], []
    slack = torch.zeros(n, dtype=torch.float64)
    v = Vd[0].double()
    for k, l in enumerate(range(L0 + 1, m.spec.layers)):
        a, o, h1 = g.sub[("attn", l)]
        _, d, h2 = g.sub[("ffn", l)]
        L = m.w.layers[l]
        # the later sublayers' bf16 roundings, per row
        slack += (sublayer_slack(o[n0:], L.ln_post_attn, h1[n0:], v, eps, attn=a[n0:], Wo=L.wo)
                  + sublayer_slack(d[n0:], L.ln_post_ffn, h2[n0:], v, eps)) / rho
        za, ba = over(seg_truth(a[n0:], A[k][None], rows, blk, H, o[n0:], eps))
        zf, bf = over(seg_truth(d[n0:], F[k][None], rows, blk, 1, d[n0:], eps))
        comp.append(torch.cat([za, zf], -1))
        ctol.append(torch.cat([ba, bf], -1))
    return {"comp": torch.stack(comp), "ctol": torch.stack(ctol), "direct": direct[0][:, :, 0],
            "dtol": direct[1][:, :, 0], "total": tt["z"][:, :, 0], "ttol": tt["bound"][:, :, 0], "h0": g.h[L0][n0:],
            "slack": slack}


def _cell_rows(p, he, hb):
    """``(sp, hit, nxt)`` of a cell from its two full forwards: the pair's spikes inside the response, those at or past
    the cell's first effective edit (the first hooked-layer row that differs from the baseline's; earlier spikes were
    exact no-ops), and those of them whose next row lies in the cell's tail."""
    n = len(p.resp)
    diff = (he != hb).any(-1).nonzero().flatten().tolist()
    f = diff[0] if diff else n
    E = min(max([len(p.gen_toks) - 2] + list(p.spikes_rel)), n - 1)
    sp = [t for t in p.spikes_rel if t < n]
    hit = [t for t in sp if f <= t <= E]
    return sp, hit, [t for t in hit if t + 1 <= E]


def test_sweep_fields_match_full_forwards(sweeps):
    """Per cell: a plain forward of prompt + baseline response through the edited model (the cell's plan row) and one
    through the unedited model, a grab of every sublayer's rows, the float64 components of every row, then the
    record's own reductions.  A number's tolerance is its kernel bound, a difference's the sum of the two, a field's
    the same reduction of those.  The record's direct term plus its components meets its total within the
    completeness bound's kernel part plus the bf16 slack of the later sublayers."""
    _got, r, pairs, cells, (spec, m, _tok, _sae) = sweeps["on"]
    assert spec.layers - 1 - r.layer == 2
    H = m.lspec.heads
    moved = 0
    base = {}
    for b, (c, rec) in enumerate(cells):
        p = pairs[c.pair]
        ids = [p.track[0]]
        if id(p) not in base:
            base[id(p)] = _truth(m, r.layer, _full_forward(m, r, p, b), p.plen, ids)
        tb = base[id(p)]
        te = _truth(m, r.layer, _full_forward(m, r, p, b, r._hook), p.plen, ids)
        sp, hit, nxt = _cell_rows(p, te["h0"], tb["h0"])
        den = len(sp)
        dc, tol = (te["comp"] - tb["comp"])[:, :, 0], (te["ctol"] + tb["ctol"])[:, :, 0]     # [Lc, n, H + 1]
        red = lambda a, rows: (a[:, rows].sum(1) / den if den else a[:, :0].sum(1))           # noqa: E731
        want = {"comp_dz_spike": (red(dc, hit), red(tol, hit)),
                "comp_dz_next": (red(dc, [t + 1 for t in nxt]), red(tol, [t + 1 for t in nxt])),
                "comp_base_spike": (red(tb["comp"][:, :, 0], sp), red(tb["ctol"][:, :, 0], sp))}
        for f, (w, tl) in want.items():
            got = torch.tensor(rec[f], dtype=torch.float64)
            assert got.shape == (2, H + 1)
            assert bool(((got - w).abs() <= tl + 1e-300).all()), (b, c.method, c.budget, f, got, w, tl)
        moved += bool((want["comp_dz_spike"][0].abs() > 10 * want["comp_dz_spike"][1]).any())
        for f, key, tk in (("comp_direct_dz_spike", "direct", "dtol"), ("comp_total_dz_spike", "total", "ttol")):
            w = float((te[key] - tb[key])[hit, 0].sum()) / den if den else 0.0
            tl = float((te[tk] + tb[tk])[hit, 0].sum()) / den if den else 0.0
            assert abs(rec[f] - w) <= tl + 1e-300, (b, f, rec[f], w, tl)
        mat = rec["comp_dz_spike"]
        assert rec["comp_attn_dz_spike"] == [math.fsum(row[:H]) for row in mat]
        assert rec["comp_mlp_dz_spike"] == [row[H] for row in mat]
        blk, name, val = rec["comp_top_spike"]
        flat = [(abs(v), kk, j) for kk, row in enumerate(mat) for j, v in enumerate(row)]
        assert abs(val) == max(x[0] for x in flat)
        assert mat[blk - r.layer - 1][H if name == "mlp" else int(name[1:])] == val
        # the sum of the parts against the total, within the completeness bound (comp_trace_cases.py): each side's
        # rows differ from the exact telescoped sum by the later sublayers' bf16 roundings, edited plus baseline
        slack = float((te["slack"] + tb["slack"])[hit].sum()) / den if den else 0.0
        kern = sum(float(want[f][1].sum()) for f in ("comp_dz_spike",)) + float(
            (te["dtol"] + tb["dtol"] + te["ttol"] + tb["ttol"])[hit, 0].sum()) / max(den, 1)
        s = rec["comp_direct_dz_spike"] + math.fsum(v for row in mat for v in row)
        assert abs(s - rec["comp_total_dz_spike"]) <= slack + kern + 1e-300, (b, s, rec["comp_total_dz_spike"])
    assert moved >= len(cells) // 2                             # the comparison is not one of zeros


def test_sweep_zero_cells_and_unchanged_records(sweeps):
    """A cell none of whose latents fire at any spike is its baseline: every difference exactly 0.  Without the switch
    the records have no such keys and are otherwise what the run with it gives, and neither a ``seg_dots`` launch nor
    the baseline pass shows in the stats."""
    on, r, pairs, cells, _ = sweeps["on"]
    off, r_off = sweeps["off"][0], sweeps["off"][1]
    assert set(on) == set(off) and not r_off.component_trace and r.component_trace
    for k in on:
        assert set(on[k]) - set(off[k]) == set(CKEYS) and not set(off[k]) - set(on[k]), k
        for f in off[k]:
            assert on[k][f] == off[k][f] or (on[k][f] != on[k][f] and off[k][f] != off[k][f]), (k, f)
    sae_cells = [(c, rec) for c, rec in cells if c.kind == "sae"]
    f = r._plan_for([c for c, _ in sae_cells], pairs, {}, with_carry=False)["f"][: len(sae_cells)]
    noop = [(c, rec) for (c, rec), fc in zip(sae_cells, f) if fc >= len(pairs[c.pair].resp)]
    for c, rec in noop:
        assert all(v == 0.0 for k in ("comp_dz_spike", "comp_dz_next") for row in rec[k] for v in row), (c, rec)
        assert rec["comp_direct_dz_spike"] == 0.0 and rec["comp_total_dz_spike"] == 0.0
        assert rec["response_ids"] == pairs[c.pair].resp
    first = {}
    for c, rec in cells:
        assert all(math.isfinite(v) for k in MATS for row in rec[k] for v in row)
        assert rec["comp_base_spike"] == first.setdefault(c.pair, rec)["comp_base_spike"]
    assert any(v != 0.0 for _, rec in cells for row in rec["comp_base_spike"] for v in row)
    for key in ("comp_rows", "comp_base_rows", "shift_base_pass_rows", "trace_base_rows"):
        assert key not in r_off.stats
    assert r.stats["comp_rows"] > 0 and r.stats["comp_base_rows"] > 0 and "trace_rows" not in r.stats
    assert all(p.x_base is None and p.z_base is None and p.c_base is not None for p in pairs)
    assert all(p.c_base is None for p in sweeps["off"][2])


def test_sweep_noop_cell_is_exactly_zero():
    """Cells whose latents never fire, made so by hand, next to pair 1's cells, which do edit: exact zeros in every
    difference, while the batch's other cells move."""
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from test_head_shift_cpu import OVR

    spec, m, tok, sae = tiny4()
    cfg = load_config(None, OVR + COMP)
    r = SweepRunner(cfg, m, tok, sae, batch=40, device="cpu", layer=1, use_graphs=False, kv_pairs=8)
    pairs = r.build_pairs(["ship"], cfg.prompts[:2], ("sae_targeted",))
    r.run_baselines(pairs)
    p = pairs[0]
    enc = sae.encode(p.resid[[t for t in p.spikes_rel if t < len(p.resp)]])
    dead = [int(i) for i in (enc.float().abs().sum(0) == 0).nonzero().reshape(-1)[:8]]
    assert len(dead) == 8 and p.spikes_rel
    p.targeted = dead
    cells = r.make_cells(pairs, ("sae_targeted",))
    res = r.run_cells(pairs, cells, measure_nll=True)
    mine = [x for c, x in zip(cells, res) if c.pair == 0]
    assert mine and len(mine) < len(res)
    for x in mine:
        assert all(v == 0.0 for k in ("comp_dz_spike", "comp_dz_next") for row in x[k] for v in row), x
        assert x["comp_direct_dz_spike"] == 0.0 and x["comp_total_dz_spike"] == 0.0 and x["comp_top_spike"][2] == 0.0
        assert any(v != 0.0 for row in x["comp_base_spike"] for v in row) and x["response_ids"] == p.resp
    assert any(abs(x["comp_top_spike"][2]) > 1e-4 for c, x in zip(cells, res) if c.pair == 1)


def test_swap_cells_report_the_donor_column():
    """Swap cells carry ``comp_dz_donor_spike`` (table column 1: the donor word's secret), the others do not; it is
    not the secret's own matrix."""
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from test_head_shift_cpu import OVR

    ovr = [o for o in OVR if not o.startswith("word_plurals")] + ["word_plurals={ship: [ship, ships], moon: [moon]}"]
    methods = ("sae_targeted", "sae_swap")
    spec, m, tok, sae = tiny4()
    cfg = load_config(None, ovr + COMP)
    r = SweepRunner(cfg, m, tok, sae, batch=40, device="cpu", layer=1, use_graphs=False, kv_pairs=8)
    pairs = r.build_pairs(["ship", "moon"], cfg.prompts[:2], methods)
    r.run_baselines(pairs)
    cells = r.make_cells(pairs, methods)
    res = r.run_cells(pairs, cells, measure_nll=True)
    sw = [x for c, x in zip(cells, res) if c.method == "sae_swap"]
    H = m.lspec.heads
    assert sw and all(len(x["comp_dz_donor_spike"]) == 2 and len(x["comp_dz_donor_spike"][0]) == H + 1 for x in sw)
    assert any(x["comp_dz_donor_spike"] != x["comp_dz_spike"] and any(v != 0.0 for row in x["comp_dz_donor_spike"]
                                                                     for v in row) for x in sw)
    assert all("comp_dz_donor_spike" not in x for c, x in zip(cells, res) if c.method != "sae_swap")


def test_unsupported_combinations_raise(tmp_path):
    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.pipelines.sweep import SweepRunner
    from test_head_shift_cpu import OVR

    with pytest.raises(ValueError, match="tensor-parallel"):
        run_sweep(load_config(None, OVR + COMP + ["parallel.tp=2"]), str(tmp_path / "tp"), log=lambda *a: None)
    spec, m, tok, sae = tiny4()
    cfg = load_config(None, OVR + COMP)
    mk = lambda **kw: SweepRunner(cfg, m, tok, sae, batch=8, device="cpu", use_graphs=False,        # noqa: E731
                                  **{"layer": 1, **kw})
    with pytest.raises(ValueError, match="layer resume"):
        mk(layer_resume=False)
    with pytest.raises(ValueError, match="layer resume"):
        mk(prefix_share=False)
    with pytest.raises(ValueError, match="last"):
        mk(layer=spec.layers - 1)
    for attr, val, match in (("tp", object(), "tensor-parallel"), ("lora", object(), "LoRA")):
        old = getattr(m, attr, None)
        setattr(m, attr, val)
        try:
            with pytest.raises(ValueError, match=match):
                mk()
        finally:
            setattr(m, attr, old)
    from dataclasses import replace

    ls = m.lspec
    m.lspec = replace(ls, head_dim=4)                            # a head narrower than one 8-column group
    try:
        with pytest.raises(ValueError, match="kernel's range"):
            mk()
    finally:
        m.lspec = ls
    m.fused_head = True                                          # the hook does not touch the head: no objection
    try:
        assert mk().component_trace
    finally:
        m.fused_head = False
    assert mk(layer=1).component_trace and load_config(None, OVR + COMP + ["intervention.layer_trace=true",
                                                       "intervention.output_shift=true"]) is not None
    r = mk(kv_pairs=8)
    pairs = r.build_pairs(["ship"], cfg.prompts[:2])
    r.run_baselines(pairs)
    r.carry_rows = 4
    with pytest.raises(ValueError, match="carry-over"):
        r.run_cells(pairs, r.make_cells(pairs)[:4])
    r.carry_rows = 0
    r.layer_resume = False                                       # switched off behind the constructor's back
    with pytest.raises(ValueError, match="layer-resume"):
        r.run_cells(pairs, r.make_cells(pairs)[:4])


def test_combines_with_the_other_readouts():
    """With the layer trace, the output shift and the output movers beside it the pairs' unedited pass is shared: it
    runs over as many rows as without the component trace, the other readouts' fields are what they are without it,
    and the component fields are what they are alone."""
    from test_head_shift_cpu import run_tiny

    others = ["intervention.layer_trace=true", "intervention.output_shift=true", "intervention.output_movers=true"]
    model = tiny4()
    alone = run_tiny(COMP, model=model)
    both = run_tiny(COMP + others, model=model)
    rest = run_tiny(others, model=model)
    assert both[1].stats["shift_base_pass_rows"] == rest[1].stats["shift_base_pass_rows"]
    assert both[1].stats["trace_base_rows"] == rest[1].stats["trace_base_rows"]
    for k, rec in both[0].items():
        for f, v in rec.items():
            src = alone[0][k] if f.startswith("comp_") else rest[0][k]
            assert v == src[f] or (v != v and src[f] != src[f]), (k, f)
        assert set(rec) == set(alone[0][k]) | set(rest[0][k])


def test_run_sweep_files_and_report(tmp_path):
    """``sweep_components.csv``, the summary's matrices and CIs, the cell records and fig8 carry the component trace
    only when enabled; the other files of the run are what they are without it."""
    import json

    from taboo_brittleness_amd.config import load_config
    from taboo_brittleness_amd.parallel.dist import DistInfo
    from taboo_brittleness_amd.pipelines.run_sweep import run_sweep
    from taboo_brittleness_amd.report.figures import make_report
    from test_head_shift_cpu import OVR

    results = tmp_path / "results"
    ovr = [o for o in OVR if not o.startswith("experiment.max_new_tokens")] + ["experiment.max_new_tokens=5"]
    texts, curves = {}, {}
    for tag, extra in (("on", COMP + ["intervention.layer_trace=true"]), ("off", ["intervention.layer_trace=true"])):
        out = str(results / "sweeps" / tag)
        summ = run_sweep(load_config(None, ovr + extra), out, info=DistInfo(), log=lambda *a: None)
        texts[tag] = open(os.path.join(out, "sweep_cells.jsonl")).read()
        curves[tag] = open(os.path.join(out, "sweep_curves.csv")).read()
        cells = [json.loads(l) for l in texts[tag].splitlines()]
        if tag == "off":
            assert not {"component_trace", "comp_blocks", "comp_names"} & set(summ["config"])
            assert not os.path.exists(os.path.join(out, "sweep_components.csv"))
            assert not any(k.startswith("comp_") for c in summ["curves"] for k in c)
            assert not any(k.startswith("comp_") for c in cells for k in c)
            continue
        blocks, names = summ["config"]["comp_blocks"], summ["config"]["comp_names"]
        assert summ["config"]["component_trace"] is True and blocks == list(range(2, 2 + len(blocks))) and blocks
        assert names[-1] == "mlp" and names[:-1] == [f"h{j}" for j in range(len(names) - 1)]
        assert all(set(CKEYS) <= set(c) for c in cells)
        lines = open(os.path.join(out, "sweep_components.csv")).read().splitlines()
        assert lines[0] == "method,budget,n,block,component,mean"
        assert len(lines) == 1 + len(blocks) * len(names) * len(summ["curves"])
        assert {l.split(",")[3] for l in lines[1:]} == {str(b) for b in blocks}
        assert {l.split(",")[4] for l in lines[1:]} == set(names)
        for c in summ["curves"]:
            assert len(c["comp_dz_spike"]) == len(blocks) and len(c["comp_dz_spike"][0]) == len(names)
            for key in ("comp_attn_dz_spike", "comp_mlp_dz_spike"):
                assert len(c[key]) == len(blocks)
                for ci in c[key]:
                    assert ci["lo"] <= ci["mean"] <= ci["hi"], c["method"]
    drop = set(CKEYS) | {"comp_dz_donor_spike"}
    strip = lambda t: [{k: v for k, v in json.loads(l).items() if k not in drop} for l in t.splitlines()]   # noqa: E731
    assert json.dumps(strip(texts["on"])) == json.dumps([json.loads(l) for l in texts["off"].splitlines()])
    assert curves["on"] == curves["off"]
    made = [os.path.basename(p) for p in make_report(str(results), str(tmp_path / "report"))]
    assert [p for p in made if p.startswith("fig8_components")] == ["fig8_components_on.png"]
    assert os.path.getsize(tmp_path / "report" / "fig8_components_on.png") > 0


def test_cli_flag_sets_the_switch():
    import inspect

    from taboo_brittleness_amd.cli import run_sweep as cli
    from taboo_brittleness_amd.config import load_config

    src = inspect.getsource(cli.main)
    assert "--component-trace" in src and "component_trace = True" in src
    assert load_config(None, []).intervention.component_trace is False
