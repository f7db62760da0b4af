"""Per-shape GEMM selection between the in-tree MFMA kernels (four-wave, ring) and hipBLASLt.

Every projection of the Gemma-2 forward (QKV, o, gate|up, down, lm_head / lens unembedding, the SAE encode, and their
two-source LoRA forms) goes through ``taboo_brittleness_amd.ops.gemm``, which asks :func:`plan` for its launches: the
table's choice (:func:`choose`), the per-epilogue rules (written down once, in :func:`plan`'s docstring) and the
``"gs"`` row split.  Only :func:`parse_choice` reads choice strings.  Pure Python: no torch, no extension.  A choice is

* ``"g256"`` / ``"g128"`` — ``csrc/gemm4.hip``'s four-wave kernel (128x128 wave tiles) with 256- or 128-row output
  tiles (the 128-row tile doubles the workgroup count for the N = 3584 projections at moderate M), bit-identical; ``"gs"`` — the four-wave kernel with its tile height(s) from a rounds model
  of the persistent grid (:func:`split_rows`: 256-row tiles, 128-row tiles, or both as two launches split by rows);
* ``"k256"`` / ``"k128"`` — the four-wave kernel split over K (``tb_gemm4_splitk``: as many K ranges as fill the
  CUs, fp32 partials, ordered reduction) for thin grids (o_proj / down at N = 3584, every projection at decode M);
  deterministic but not bit-identical to the unsplit kernels, so ``auto`` only;
* ``"r<bm>x<bn>"`` / ``"r<bm>x<bn>b"`` / ``"r<bm>x<bn>c"`` — ``csrc/gemm_ring.hip``'s narrow-tile ring GEMM (bm x bn
  output tiles, a 64 KB or 144 KB LDS-DMA ring; ``c``: deeper stages for the small tiles): fills the chip at decode / mid row counts WITHOUT splitting K, bit-identical to the
  four-wave kernel at every M (batch-invariant);
* ``"blas"`` — ``torch.matmul`` (hipBLASLt, with the TunableOp solution table the bench loads).

Modes (``TB_GEMM``):

* ``tb`` (default) — in-tree batch-invariant kernels only (``g*``, ``gs``, ``r*``; never split-K or hipBLASLt), per row count the fastest of them as measured (the table's ``tb_shapes``; without one the fill
  heuristic).  All of them accumulate every output element over K in the same order with the same MFMA, so a row's
  result does not depend on M or on the tile choice: the whole forward is batch-invariant, which is what makes the
  sweep's reuse levels (shared prefixes, layer resume, ride-along baselines, trie decode) exact -- every cell's
  records equal a from-scratch generation of that cell (the GPU equivalence tests require bit-equal records).
* ``auto`` — the fastest of in-tree / split-K / hipBLASLt per ``(N, K, epilogue, M)`` as measured on an MI355X by
  ``tools/ring_bench.py`` / ``tools/gemm_dispatch_tune.py`` (``configs/gemm_dispatch/<arch>.json``); shapes the
  table does not cover use hipBLASLt.  NOT batch-invariant: a row's bf16 projections depend on the batch's row
  count, so reused and from-scratch results can differ in the last bits and then in greedy tokens
  (``tests/test_drift_gpu.py`` measures how often).
* ``blas`` — hipBLASLt only (the round-2 path).
"""
from __future__ import annotations

import bisect
import functools
import json
import os
from typing import Dict, List, NamedTuple, Optional, Tuple, Union

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TABLE_DIR = os.path.join(REPO, "configs", "gemm_dispatch")
NUM_CU = 256

Choice = Union[int, str]

_state = {"mode": os.environ.get("TB_GEMM", "tb"), "table": None, "tb_table": None, "table_path": None,
          "loaded": False}


def set_mode(mode: str) -> None:
    assert mode in ("auto", "tb", "blas"), mode
    _state["mode"] = mode


def mode() -> str:
    return _state["mode"]


def load_table(path: Optional[str] = None, arch: str = "gemma2-9b") -> Optional[str]:
    """Load the measured dispatch table (``None``: ``TB_GEMM_TABLE`` or ``configs/gemm_dispatch/<arch>.json``)."""
    path = path or os.environ.get("TB_GEMM_TABLE") or os.path.join(TABLE_DIR, f"{arch}.json")
    if not os.path.exists(path):
        _state["table"], _state["table_path"] = None, None
        return None
    raw = json.load(open(path))

    def parse(sec):
        tab: Dict[Tuple[int, int, int], Tuple[List[int], List[Choice]]] = {}
        for key, rows in raw.get(sec, {}).items():
            n, k, e = (int(v) for v in key.split(","))
            rows = sorted(rows, key=lambda r: r[0])
            tab[(n, k, e)] = ([int(r[0]) for r in rows], [r[1] if isinstance(r[1], str) else int(r[1]) for r in rows])
        return tab
    _state["table"], _state["tb_table"], _state["table_path"] = parse("shapes"), parse("tb_shapes") or None, path
    _state["loaded"] = True
    return path


def fill_choice(M: int, N: int) -> Choice:
    """Four-wave kernel tile rows without a measured entry: 256 unless the grid fills less than half the CUs (the
    128-row tile runs its MFMAs at ~0.78x the 256-row tile's rate, profiles/r4/gemm4/pmc_counted_waits_gate_up_4096.txt,
    so it only pays where it doubles a very thin grid)."""
    return "g128" if (N // 256) * (-(-M // 256)) < NUM_CU // 2 else "g256"


def choose(M: int, N: int, K: int, epi: int = 0) -> Choice:
    """``"g256"`` | ``"g128"`` | ``"gs"`` | ``"r<bm>x<bn>[b]"`` | ``"k256"`` | ``"k128"`` | ``"k64"`` | ``"blas"`` for
    ``C[M, N] = A[M, K] @ W[N, K]^T`` (epi 3: gate|up + GeGLU, 4: QKV + RoPE, 5: o / down + residual norm)."""
    m = _state["mode"]
    if m == "blas":
        return "blas"
    if not _state["loaded"]:
        load_table()          # keyed by (N, K, epilogue): shapes of other models simply miss it
    ent = _tb_entry(N, K, epi) if m == "tb" else (_state["table"] or {}).get((N, K, epi))
    if ent is not None:
        ms, cs = ent
        return cs[min(bisect.bisect_left(ms, M), len(cs) - 1)]
    return fill_choice(M, N) if m == "tb" else "blas"


@functools.lru_cache(maxsize=1024)
def _tb_entry_cached(table_id: int, N: int, K: int, epi: int):
    tab = _state["tb_table"]
    if tab is None:
        return None
    for e in ((epi, 0) if epi in (4, 5) else (epi,)):
        if (N, K, e) in tab:
            return tab[(N, K, e)]
    # a LoRA-augmented projection (models/lora.py: the bank's up-projections appended to K) runs the base shape's
    # choices: the largest measured K below it with the same N (its extra K tiles are < 4 % of the work)
    for e in ((epi, 0) if epi in (4, 5) else (epi,)):
        ks = [k for (n, k, ee) in tab if n == N and ee == e and k < K]
        if ks:
            return tab[(N, max(ks), e)]
    return None


def _tb_entry(N: int, K: int, epi: int):
    return _tb_entry_cached(id(_state["tb_table"]), N, K, epi)


def has_entry(N: int, K: int, epi: int, M: Optional[int] = None) -> bool:
    """Whether the loaded dispatch table measured ``(N, K, epi)`` (auto mode), up to row count ``M`` if given."""
    if _state["mode"] != "auto":
        return False
    if not _state["loaded"]:
        load_table()
    tab = _state["table"]
    if tab is None or (N, K, epi) not in tab:
        return False
    return M is None or M <= tab[(N, K, epi)][0][-1]


# time of a 128-row four-wave tile relative to a 256-row one (half the MFMAs at 0.538 vs 0.694 MFMA utilisation,
# profiles/r4/gemm4/pmc_counted_waits_gate_up_4096.txt)
G128_COST = 0.64


@functools.lru_cache(maxsize=4096)
def split_rows(M: int, N: int) -> int:
    """Row split of the ``"gs"`` choice: rows ``[0, M1)`` on 256-row tiles, the rest on 128-row tiles (two launches of
    the persistent four-wave kernel).  A persistent grid runs in rounds of one tile per CU, so a grid that does not
    divide into the CUs leaves its last round part-empty (e.g. o_proj at M = 6144: 14 x 24 = 336 tiles on 256 CUs);
    ``M1`` minimises the rounds-based cost ``ceil(tiles256 / CUs) + G128_COST * ceil(tiles128 / CUs)`` over the
    multiples of 256 (ties: more 256-row rows).  ``M1 = M``: plain 256-row tiles, ``0``: plain 128-row tiles.  The
    model picks the fastest of the three at 213 of 222 measured (shape, M) points above 2048 rows and is within 3 % at
    the rest (profiles/r5/gemm_dispatch/gs.jsonl).  Every tile height accumulates the same K chain, so the split keeps
    the GEMM batch-invariant."""
    nbn = max(1, N // 256)

    def cost(m1):
        c = -(-nbn * -(-m1 // 256) // NUM_CU) if m1 > 0 else 0
        return c + (G128_COST * -(-nbn * -(-(M - m1) // 128) // NUM_CU) if m1 < M else 0.0)
    cands = [min(256 * k, M) for k in range(-(-M // 256) + 1)]
    return min(cands, key=lambda m1: (cost(m1), -m1))


class Parsed(NamedTuple):
    """A choice, decoded: kind ``"g"`` / ``"k"`` (tile: tile rows), ``"r"`` (tile: ``(bm, bn, variant)``), ``"gs"``,
    ``"blas"``."""
    kind: str
    tile: Union[None, int, Tuple[int, int, int]] = None


class Launch(NamedTuple):
    """One launch over rows ``[r0, r1)``: family ``"g4"`` / ``"splitk"`` (tile: tile rows), ``"ring"`` (tile:
    ``(bm, bn, variant)``) or ``"blas"``."""
    family: str
    r0: int
    r1: int
    tile: Union[None, int, Tuple[int, int, int]] = None


@functools.lru_cache(maxsize=512, typed=True)
def parse_choice(c) -> Parsed:
    """Every accepted spelling of a choice as one :class:`Parsed` value (the only place choice strings are read):
    ``"g256"`` / ``"g128"``, ``"gs"``, ``"k64"`` / ``"k128"`` / ``"k256"``, ``"r<bm>x<bn>"`` (variant 0, 64 KB ring) /
    ``"r<bm>x<bn>b"`` (1, 144 KB ring) / ``"r<bm>x<bn>c"`` (2, 144 KB ring of 4-8 K tiles per stage), ``"blas"``, a bare
    table int ``256`` / ``128`` (= ``g<int>``); a :class:`Parsed` passes through."""
    if isinstance(c, Parsed):
        return c
    if isinstance(c, int) and not isinstance(c, bool):
        return Parsed("g", c)
    if isinstance(c, str):
        if c in ("gs", "blas"):
            return Parsed(c)
        head, body = c[:1], c[1:]
        if head in ("g", "k") and body.isdigit():
            return Parsed(head, int(body))
        if head == "r":
            var = {"b": 1, "c": 2}.get(body[-1:], 0)
            bm, _, bn = (body[:-1] if var else body).partition("x")
            if bm.isdigit() and bn.isdigit():
                return Parsed("r", (int(bm), int(bn), var))
    raise ValueError(f"unknown GEMM choice {c!r}")


def is_invariant(choice: Choice) -> bool:
    """Whether a choice accumulates every output over K in the one order of the in-tree kernels (no split-K, no
    hipBLASLt): rows then get bit-identical results in any batch."""
    return isinstance(choice, str) and parse_choice(choice).kind in ("g", "gs", "r")


def ring_tile(choice: Choice) -> Optional[Tuple[int, int, int]]:
    """``(bm, bn, variant)`` of a ring-GEMM choice (see :func:`parse_choice`), else None."""
    p = parse_choice(choice) if isinstance(choice, str) else None
    return p.tile if p is not None and p.kind == "r" else None


def resolve(M: int, N: int, K: int, epi: int = 0, two_source: bool = False, ring_ok=None) -> Parsed:
    """The choice one GEMM runs, by the rules of :func:`plan`."""
    if two_source:
        c = choose(M, N, K, epi)
        p = parse_choice(c) if isinstance(c, str) else None
        if p is not None and p.kind == "r":
            bm, bn, _ = p.tile
            p = Parsed("r", (bm, bn, 1)) if ring_ok(epi if epi in (3, 4) else 0, bm, bn, 1) else None
        return parse_choice(fill_choice(M, N)) if p is None or p.kind in ("blas", "k") else p
    if epi in (4, 5) and not (has_entry(N, K, epi, M) or _state["mode"] == "tb"):
        p = parse_choice(choose(M, N, K, 0))
    else:
        p = parse_choice(choose(M, N, K, epi))
    if epi == 3 and p.kind == "blas":
        return parse_choice(fill_choice(M, N))
    if epi == 4 and p.kind == "r" and not ring_ok(4, *p.tile):
        return Parsed("g", 128)
    return p


@functools.lru_cache(maxsize=4096)
def _launches(p: Parsed, M: int, N: int) -> Tuple[Launch, ...]:
    if p.kind == "gs":                # full rounds of 256-row tiles, the rest on 128-row tiles
        M1 = split_rows(M, N)
        return tuple(Launch("g4", r0, r1, rows) for r0, r1, rows in ((0, M1, 256), (M1, M, 128)) if r1 > r0)
    return (Launch({"g": "g4", "k": "splitk", "r": "ring", "blas": "blas"}[p.kind], 0, M, p.tile),)


def plan(M: int, N: int, K: int, epi: int = 0, two_source: bool = False, ring_ok=None,
         choice: Optional[Choice] = None) -> Tuple[Launch, ...]:
    """The launches of ``C[M, N] = A[M, K] @ W[N, K]^T`` under table key ``epi`` (0 plain, 3 gate|up + GeGLU,
    4 QKV + RoPE, 5 o / down + residual norm), in order.  ``two_source``: A is ``[x | a2]`` (the LoRA-augmented
    operand, ``K`` its whole width).  ``ring_ok(epi, bm, bn, variant)`` tells whether the ring GEMM is built with a
    tile for this shape.  ``choice`` forces a choice in place of the rules (``ops.tb_gemm`` / ``ops.gemm_l2a``,
    ``ops.linear``'s override).  The rules:

    * epilogue 0 and 3: ``choose(M, N, K, epi)``.  For 3 that is also what ``ops.fused_geglu_wins`` tests
      (``!= "blas"``); ``ops.gate_up_geglu``, once called, runs ``"blas"`` as ``fill_choice(M, N)``.
    * epilogues 4 and 5: their own table entry where ``has_entry(N, K, epi, M)`` or the mode is ``tb``, else the
      epilogue-0 entry.
    * QKV (4), one source: a ring tile the kernel does not have (``ring_ok``) becomes the four-wave kernel with 128-row
      tiles; ``"splitk"`` means fp32 partials summed by ``rope_qkv_cache_part``, ``"blas"`` the plain projection (its
      own epilogue-0 dispatch) then ``rope_qkv_cache``.  For epilogue 5 ``"splitk"`` means partials summed by
      ``add_rmsnorm2_part``.
    * two sources: ``choose(M, N, K, epi)`` directly, without the epilogue-0 fallback; ``"blas"``, ``k*`` and bare-int
      entries become ``fill_choice(M, N)`` (one K order, never hipBLASLt); a ring tile always takes variant 1 (the
      only one built with two sources) and is checked with ``ring_ok`` -- epilogue 5 against ring epilogue 0 -- else
      ``fill_choice(M, N)``.
    * ``"gs"`` is two launches split at ``split_rows(M, N)``, empty row ranges dropped.
    * a plain projection (0, 3, 5) with a ring choice does not ask ``ring_ok``: the binding checks the tile.
    * ``ops.gemm_nt`` on four-wave-eligible shapes forces ``fill_choice(max(M, 4096), N)``."""
    p = resolve(M, N, K, epi, two_source, ring_ok) if choice is None else parse_choice(choice)
    return _launches(p, M, N)


def describe() -> dict:
    return {"mode": _state["mode"],
            "table": os.path.relpath(_state["table_path"], REPO) if _state["table_path"] else None}
