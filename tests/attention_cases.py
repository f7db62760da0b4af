"""Shared inputs and an fp64 ground truth for the attention edge tests (tests/test_attention_edges_cpu.py and
tests/test_attention_edges_gpu.py).

``truth`` is softcapped GQA attention straight from its definition in float64, with no bf16 rounding of the softmax
weights: it does not go through ``ops.reference.attention`` and so does not share the kernels' rounding choices.

The builders return CPU tensors, seeded per case.  Every case is a dense ``[B, T]`` grid of query rows (row ``b * T +
t`` belongs to sequence ``b``; ``pos == -1`` marks a padding row), which the tests run three ways: as a dense prefill
(``ops.attention`` with ``T > 1``), as packed blocks (``ops.attention_varlen``) and row by row as decode steps
(``ops.attention`` with ``T == 1``).
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import torch

BF = torch.bfloat16
ATOL = RTOL = 2e-2              # the existing attention tests' tolerance (tests/test_kernels_gpu.py)
HKV = 2
GEOMS = ((256, 2), (256, 4), (128, 1), (128, 4))     # (HD, G)


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    HD: int
    G: int
    S: int
    B: int
    T: int
    q: torch.Tensor               # [B * T, Hq, HD] bf16
    kc: torch.Tensor              # [slots, Hkv, S, HD] bf16
    vc: torch.Tensor
    pos: torch.Tensor             # [B, T] int32, -1 = padding row
    slot: torch.Tensor            # [B] int32
    cap: float
    window: int
    prefix: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]] = None   # pk, pv, ps [B], pl [B]

    @property
    def scale(self) -> float:
        return self.HD ** -0.5

    @property
    def M(self) -> int:
        return self.B * self.T

    def rows(self):
        """Per-row view: (pos [M], slot [M], prefix (pk, pv, ps [M], pl [M]) or None)."""
        rep = lambda t: t.repeat_interleave(self.T).contiguous()      # noqa: E731
        pre = None
        if self.prefix is not None:
            pk, pv, ps, pl = self.prefix
            pre = (pk, pv, rep(ps), rep(pl))
        return self.pos.reshape(-1).contiguous(), rep(self.slot), pre

    def seqs(self):
        """(first row, rows, slot[, prefix slot, prefix length]) per sequence, for ``packed_blocks``."""
        out = []
        for b in range(self.B):
            s = (b * self.T, self.T, int(self.slot[b]))
            if self.prefix is not None:
                s += (int(self.prefix[2][b]), int(self.prefix[3][b]))
            out.append(s)
        return out


def truth(q, kc, vc, pos, slot_rows, scale, cap, window, prefix=None) -> torch.Tensor:
    """Attention of packed rows in float64 from the definition.  ``q [M, Hq, HD]``, cache ``[slots, Hkv, S, HD]``,
    ``pos [M]``, ``slot_rows [M]``; ``prefix = (pk, pv, ps [M], pl [M])``: keys ``[0, pl[i])`` of row ``i`` come from
    slot ``ps[i]`` of ``pk / pv``.  Returns ``[M, Hq * HD]`` float64; rows with ``pos < 0`` are zero."""
    Hkv, S, HD = kc.shape[1], kc.shape[2], kc.shape[3]
    M = pos.numel()
    Hq = q.numel() // (M * HD)
    G = Hq // Hkv
    out = torch.zeros(M, Hq, HD, dtype=torch.float64)
    qd = q.reshape(M, Hq, HD).double()
    for i in range(M):
        p = int(pos[i])
        if p < 0:
            continue
        n = p + 1
        K = kc[int(slot_rows[i]), :, :n].double()
        V = vc[int(slot_rows[i]), :, :n].double()
        if prefix is not None:
            npre = min(int(prefix[3][i]), n)
            if npre > 0:
                K[:, :npre] = prefix[0][int(prefix[2][i]), :, :npre].double()
                V[:, :npre] = prefix[1][int(prefix[2][i]), :, :npre].double()
        key = torch.arange(n)
        ok = key <= p
        if window > 0:
            ok &= (p - key) < window
        s = torch.einsum("hgd,hnd->hgn", qd[i].view(Hkv, G, HD), K) * scale
        if cap > 0:
            s = cap * torch.tanh(s / cap)
        s = s.masked_fill(~ok, float("-inf"))
        w = torch.softmax(s, dim=-1)
        out[i] = torch.einsum("hgn,hnd->hgd", w, V).reshape(Hq, HD)
    return out.view(M, Hq * HD)


def off_count(a: torch.Tensor, b: torch.Tensor, atol: float = ATOL, rtol: float = RTOL):
    """(elements of ``a`` outside ``atol + rtol * |b|`` of ``b``, max abs error)."""
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    err = (a - b).abs()
    return int((err > atol + rtol * b.abs()).sum()), float(err.max()) if err.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------
# builders

def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _randn(g, *shape, mul=1.0):
    return (torch.randn(*shape, generator=g) * mul).to(BF)


def _grid(bases, T):
    return (torch.tensor(bases, dtype=torch.int32)[:, None] + torch.arange(T, dtype=torch.int32)[None, :]).contiguous()


def _random_case(name, family, geom, S, pos, qmul, cap, window, plens=None, spike=0.0) -> Case:
    """Random K / V, ``q = randn * qmul``.  ``plens``: per-sequence shared-prefix lengths.  ``spike > 0`` makes the two
    keys at each prefix boundary (the prefix slot's key ``plen - 1`` and the own slot's key ``plen``) stand out by
    about ``spike`` in score for every query, so that reading either from the wrong cache changes the output."""
    HD, G = geom
    g = _gen(name)
    B, T = pos.shape
    Hq = HKV * G
    kc = _randn(g, B + 1, HKV, S, HD)
    vc = _randn(g, B + 1, HKV, S, HD)
    slot = torch.randperm(B + 1, generator=g)[:B].to(torch.int32)
    q = torch.randn(B * T, Hq, HD, generator=g) * qmul
    prefix = None
    if plens is not None:
        pk = _randn(g, 3, HKV, S, HD)
        pv = _randn(g, 3, HKV, S, HD)
        ps = torch.randint(0, 3, (B,), generator=g, dtype=torch.int32)
        pl = torch.tensor(plens, dtype=torch.int32)
        if spike > 0:
            u = torch.randn(HD, generator=g)
            u /= u.norm()
            c = (spike / HD ** -0.5) ** 0.5            # (c u) . (c u) * scale = spike
            q = q + c * u
            for b in range(B):
                n = int(pl[b])
                if 0 < n <= S:
                    pk[int(ps[b]), :, n - 1] = (pk[int(ps[b]), :, n - 1].float() + c * u).to(BF)
                if n < S:
                    kc[int(slot[b]), :, n] = (kc[int(slot[b]), :, n].float() + c * u).to(BF)
        prefix = (pk, pv, ps, pl)
    return Case(name, family, HD, G, S, B, T, q.to(BF), kc, vc, pos.contiguous(), slot, cap, window, prefix)


def _order_case(name: str, family: str, mode: str, geom) -> Case:
    """Keys along one direction ``u``: ``q . k * scale`` is a prescribed function of the key index (plus a jitter of
    about 0.3): ascending or descending from -20 to 20 over the cache, or flat with one key 12 above the rest."""
    HD, G = geom
    g = _gen(name)
    S, B, T = 272, 2, 8
    Hq = HKV * G
    pos = _grid((140, S - T), T)
    u = torch.randn(HD, generator=g)
    u /= u.norm()
    key = torch.arange(S, dtype=torch.float32)
    if mode == "asc":
        t = -20 + 40 * key / (S - 1)
    elif mode == "desc":
        t = 20 - 40 * key / (S - 1)
    else:
        t = torch.zeros(S)
        if mode == "dompos":
            t[pos.reshape(-1).long()] = 12.0
        else:
            t[int(mode[3:])] = 12.0
    c = HD ** 0.5                                          # (c u) . (t u) * scale = t
    kc = (t[None, None, :, None] * u + 0.25 * torch.randn(B + 1, HKV, S, HD, generator=g)).to(BF)
    vc = _randn(g, B + 1, HKV, S, HD)
    q = (c * u + 0.25 * torch.randn(B * T, Hq, HD, generator=g)).to(BF)
    slot = torch.tensor([2, 0], dtype=torch.int32)
    return Case(name, family, HD, G, S, B, T, q, kc, vc, pos, slot, 50.0, 0)


# ---------------------------------------------------------------------------------------------------------------
# the case table: name -> (family, builder); nothing is built until a test asks for the case

_REG: Dict[str, Tuple[str, Callable[[], Case]]] = {}


def _reg(fn, name, family, *args):
    assert name not in _REG
    _REG[name] = (family, functools.partial(fn, name, family, *args))


# Saturating softcap: q * 12 and q * 40 put raw scores at a standard deviation of 12 and 40; cap 0 = no softcap.
for _i, (_qmul, _cap) in enumerate(((12, 50.0), (40, 50.0), (12, 5.0), (12, 0.0), (2, 0.0))):
    _pos = _grid((0, 30, 96 - 8), 8)
    _pos[1, 3] = -1
    _reg(_random_case, f"softcap_q{_qmul}_cap{_cap:g}", "softcap", GEOMS[_i % 4], 96, _pos, _qmul, _cap, 0)

# More than 128 keys under multi-row blocks: each wave of the prefill kernel runs its K loop more than once.
for _i, (_qmul, _w) in enumerate(((2, 0), (12, 33), (12, 0), (2, 33))):
    _pos = _grid((0, 131, 300 - 37), 37)
    _pos[0, -2:] = -1
    _pos[2, 5] = -1
    _reg(_random_case, f"prefill_s300_q{_qmul}_w{_w}", "prefill", GEOMS[_i], 300, _pos, _qmul, 50.0, _w)

# Packed rows over a cache of 528 positions, the smallest multiple of 16 above the 512 switch.  T = 33 rows per
# sequence gives blocks of the full 16 / G rows and a last block of one row for every G.  Prefix lengths 31 / 32 / 33
# sit around the 32-key block edge; 0 is no prefix, 528 lies beyond every position.
_pos = _grid((0, 131, 528 - 33), 33)
_reg(_random_case, "packed_s528_plain", "packed", GEOMS[0], 528, _pos, 12, 50.0, 0)
_reg(_random_case, "packed_s528_plain_w33", "packed", GEOMS[3], 528, _pos, 2, 50.0, 33)
_reg(_random_case, "packed_s528_prefix_a", "packed_prefix", GEOMS[1], 528, _pos, 2, 50.0, 0, (31, 32, 33), 8.0)
_reg(_random_case, "packed_s528_prefix_b", "packed_prefix", GEOMS[2], 528, _pos, 2, 50.0, 0, (0, 528, 505), 8.0)
_reg(_random_case, "packed_s528_prefix_w33", "packed_prefix", GEOMS[0], 528, _pos, 2, 50.0, 33, (33, 150, 500), 8.0)

# Score order: ascending, descending, flat with one dominant key.
ORDERS = ("asc", "desc", "dom0", "dom31", "dom32", "dom127", "dom128", "dompos")
for _i, _m in enumerate(ORDERS):
    _reg(_order_case, f"order_{_m}", "order", _m, GEOMS[_i % 4])

# Window edges.  Sequence 0: one row per window start pos - window + 1 in KMINS, and a padding row; sequence 1:
# consecutive positions across the point where the window fills (live ranges of fewer than window keys, then window);
# sequence 2: the last positions of the cache.  Windows 1, 15, 16 and 17 give live ranges of exactly that many keys.
# The prefix variants give sequence 0 a prefix of 20 keys (cut in the middle by the windows that start at 0 to 17,
# excluded entirely by those that start at 31 to 33), sequence 1 one that ends inside its rows, and sequence 2 one that
# covers all but the last 4 positions.
WINDOWS = (1, 15, 16, 17, 31, 32, 33, 4096)
KMINS = (0, 15, 16, 17, 31, 32, 33)
for _i, _w in enumerate(WINDOWS):
    _S = 300 if _w == 4096 else 96
    _edge = [0, 15, 16, 17, 131, 160, 255] if _w == 4096 else [_w - 1 + _k for _k in KMINS]
    _pos = torch.stack([torch.tensor(_edge + [-1], dtype=torch.int32),
                        _grid((max(0, min(_w, _S - 8) - 4),), 8)[0], _grid((_S - 8,), 8)[0]])
    _reg(_random_case, f"window_w{_w}", "window", GEOMS[_i % 4], _S, _pos, 2, 50.0, _w)
    _reg(_random_case, f"window_w{_w}_prefix", "window_prefix", GEOMS[(_i + 1) % 4], _S, _pos, 2, 50.0, _w,
         (20, int(_pos[1, 3]), _S - 4), 4.0)

# Long decode, T = 1: S = 2064 (2048 < S <= 8192: attn_decode_kernel) and S = 8208 (> 8192: attn_cache_kernel with
# one row per block), positions {0, S / 2 + 5, S - 1}.
for _S, _geom, _w, _pl in ((2064, GEOMS[1], 0, None), (2064, GEOMS[2], 4096, None), (2064, GEOMS[0], 0, (0, 517, 3000)),
                           (8208, GEOMS[3], 0, None), (8208, GEOMS[0], 4096, None)):
    _pos = torch.tensor([[0], [_S // 2 + 5], [_S - 1]], dtype=torch.int32)
    _reg(_random_case, f"long_s{_S}_w{_w}" + ("_prefix" if _pl else ""), "long", _geom, _S, _pos, 12, 50.0, _w, _pl,
         8.0 if _pl else 0.0)

# Degenerate rows: pos = 0, padding rows between valid rows, a sequence made only of padding rows.
for _i, _geom in enumerate(GEOMS):
    _pos = torch.tensor([[0, -1, 2, 3, -1, -1, 6, 7], [-1] * 8, [0, 1, 2, -1, 4, 5, 6, 47], [0] * 7 + [-1]],
                        dtype=torch.int32)
    _reg(_random_case, f"degenerate_{_geom[0]}x{_geom[1]}", "degenerate", _geom, 48, _pos, 2, 50.0, (0, 16, 0, 3)[_i])

CASE_NAMES = tuple(_REG)
FAMILIES = tuple(dict.fromkeys(f for f, _ in _REG.values()))


def family_names(family: str) -> Tuple[str, ...]:
    return tuple(n for n, (f, _) in _REG.items() if f == family)


@functools.lru_cache(maxsize=8)
def case(name: str) -> Case:
    return _REG[name][1]()


@functools.lru_cache(maxsize=None)
def case_truth(name: str) -> torch.Tensor:
    """``truth`` of a case's rows, computed once per process; callers must not modify it."""
    c = case(name)
    pos, slot_rows, pre = c.rows()
    return truth(c.q, c.kc, c.vc, pos, slot_rows, c.scale, c.cap, c.window, pre)
