"""The five attention kernels of csrc/attention.hip against the fp64 ground truth of tests/attention_cases.py, on the
inputs that tests/test_attention_edges_cpu.py shows to tell wrong kernels apart.

Every case is a [B, T] grid of query rows that is run through each kernel that can take it:

  cache   attn_cache_kernel: the dense prefill (T > 1, no prefix), packed rows over a cache of more than 512
          positions (3- and 5-column block table), and T = 1 rows over a cache of more than 8192 positions
  tail    attn_tail_exact_kernel: packed rows over a cache of at most 512 positions
  wave    attn_decode_wave_kernel: each row as a decode step, S <= 2048, split threshold 0
  split   attn_decode_split_kernel: the same with the split threshold at 1 << 20 (HD = 256, G = 2 or 4)
  decode  attn_decode_kernel: T = 1 rows, 2048 < S <= 8192

All compare under the existing attention tests' tolerance, atol = rtol = 2e-2, with 0 elements allowed outside;
padding rows (pos = -1) must be exact zeros.
"""
import pytest
import torch

from attention_cases import case, case_truth, family_names, off_count
from taboo_brittleness_amd import ops
from taboo_brittleness_amd.models.gemma2 import packed_blocks

pytestmark = pytest.mark.gpu


def _routes(c):
    """(kernel, how to call it) for every kernel that can run the case."""
    if c.T == 1 and c.S > 2048:
        return [("cache", "dense")] if c.S > 8192 else [("decode", "rows")]
    out = []
    if c.S > 512:
        out.append(("cache", "packed"))
    else:
        out.append(("tail", "packed"))
        if c.prefix is None and c.T > 1:
            out.append(("cache", "dense"))
    out.append(("wave", "rows"))
    if c.HD == 256 and c.G in (2, 4):
        out.append(("split", "rows"))
    return out


def _run(c, kernel, how, gpu):
    d = lambda t: t.to(gpu)                                # noqa: E731
    pos, slot_rows, pre = c.rows()
    q, kc, vc = d(c.q), d(c.kc), d(c.vc)
    if how == "dense":
        assert c.prefix is None
        return ops.attention(q, kc, vc, d(pos), d(c.slot), c.B, c.T, c.scale, c.cap, c.window)
    if how == "packed":
        blk = packed_blocks(c.seqs(), 16 // c.G)
        assert blk.shape[1] == (3 if c.prefix is None else 5)
        assert {int(n) for n in blk[:, 1]} >= ({16 // c.G, 1} if c.family.startswith("packed") else set())
        pkv = None if c.prefix is None else (d(c.prefix[0]), d(c.prefix[1]))
        return ops.attention_varlen(q, kc, vc, d(pos), d(slot_rows), d(blk), c.scale, c.cap, c.window, prefix_kv=pkv)
    k = ops._k()
    split = (1 << 20) if kernel == "split" else 0
    old = k.attention_split_rows(-1, True), k.attention_split_rows(-1, False)
    try:
        k.attention_split_rows(split, True)
        k.attention_split_rows(split, False)
        pre_d = None if pre is None else tuple(d(t) for t in pre)
        out = ops.attention(q, kc, vc, d(pos), d(slot_rows), c.M, 1, c.scale, c.cap, c.window, prefix=pre_d)
        torch.cuda.synchronize()
        return out
    finally:
        k.attention_split_rows(old[0], True)
        k.attention_split_rows(old[1], False)


def _check(name, gpu, expect):
    """Run the case through every kernel that takes it; ``expect``: the kernels the family is meant to reach."""
    c = case(name)
    want = case_truth(name)
    pad = (c.pos.reshape(-1) < 0)
    routes = _routes(c)
    assert {kn for kn, _ in routes} >= set(expect), (name, routes)
    msgs = []
    for kernel, how in routes:
        got = _run(c, kernel, how, gpu).float().cpu().view(c.M, -1)
        assert torch.isfinite(got).all(), (name, kernel)
        bad, err = off_count(got, want)
        print(f"ATTN_EDGE gpu {c.family} {name} {kernel} max_err {err:.4g} off {bad}")
        if bad:
            msgs.append(f"{kernel}: {bad} / {got.numel()} elements off; max err {err:.4g}")
        if not (got[pad] == 0).all():
            msgs.append(f"{kernel}: padding rows not exactly zero")
    assert not msgs, f"{name} (HD {c.HD}, G {c.G}, S {c.S}, window {c.window}, cap {c.cap}): " + "; ".join(msgs)


@pytest.mark.parametrize("name", family_names("softcap"))
def test_softcap_saturating(gpu, name):
    """Raw scores at a standard deviation of 12 and 40 against caps of 50 and 5, and cap = 0 (no softcap): a kernel
    without the tanh, with the cap before the scale, or with a cap 10 % off fails here (cache, tail, wave, split)."""
    _check(name, gpu, ("cache", "tail", "wave"))


@pytest.mark.parametrize("name", family_names("prefill"))
def test_prefill_more_than_128_keys(gpu, name):
    """Dense T = 37 rows over up to 300 keys: every wave of attn_cache_kernel runs its 32-key loop up to three times,
    so the online-softmax carry (alpha, l, the accumulator rescale, the V re-staging) decides the result; the same
    rows through the tail and decode kernels."""
    _check(name, gpu, ("cache", "tail", "wave"))


@pytest.mark.parametrize("name", family_names("packed") + family_names("packed_prefix"))
def test_packed_rows_above_512_switch(gpu, name):
    """Packed rows over a cache of 528 positions run the block-table form of attn_cache_kernel (3- and 5-column
    tables, prefix lengths 31 / 32 / 33 / 0 / beyond the block, blocks of 16 / G rows and of one row).  This checks
    numerics against the fp64 truth only: above 512 positions packed rows are not bit-equal to the decode."""
    _check(name, gpu, ("cache", "wave"))


@pytest.mark.parametrize("name", family_names("order"))
def test_score_order(gpu, name):
    """Scores ascending or descending with the key index, or flat with one dominant key at index 0, 31, 32, 127, 128
    or the row's own position: an online softmax that misses a rescale when the maximum rises fails here."""
    _check(name, gpu, ("cache", "tail", "wave"))


@pytest.mark.parametrize("name", family_names("window") + family_names("window_prefix"))
def test_window_edges(gpu, name):
    """Windows 1, 15, 16, 17, 31, 32, 33 and 4096 at positions whose window starts at key 0, 15, 16, 17, 31, 32 and
    33, live ranges of 1, 15, 16 and 17 keys, with and without a shared prefix that the window cuts or excludes."""
    c = case(name)
    _check(name, gpu, ("tail", "wave") if c.prefix is not None else ("cache", "tail", "wave"))


@pytest.mark.parametrize("name", family_names("long"))
def test_long_decode(gpu, name):
    """T = 1 at S = 2064 (attn_decode_kernel) and S = 8208 (attn_cache_kernel), positions 0, S / 2 + 5 and S - 1,
    window 0 and 4096, saturating scores."""
    _check(name, gpu, ("cache",) if case(name).S > 8192 else ("decode",))


@pytest.mark.parametrize("name", family_names("degenerate"))
def test_degenerate_rows(gpu, name):
    """pos = 0 rows, padding rows between valid rows and a sequence of padding rows only: exact zeros for padding."""
    _check(name, gpu, ("cache", "tail", "wave"))
