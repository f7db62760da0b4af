"""Residual-stream interventions at the hooked layer (EP:112-152).

An :class:`EditPlan` describes, per batch row (= sweep cell), *where* to edit
(absolute spike positions) and *what* to remove:

* ``sae`` cells — error-preserving latent ablation ``x <- x - alpha * sum_{j in S} a_j(x) W_dec[j]``
  (only the ablated latents are encoded: ``a_j = JumpReLU(<x - b_dec?, W_enc[:, j]> + b_enc[j])``).
* ``proj`` cells — projection-out ``x <- x - U U^T x`` with an orthonormal basis ``U`` per cell.

Both are the same row-local low-rank update, so one HIP kernel
(``ops.lowrank_edit``) serves a whole mixed batch; the hook only computes the
per-row "is this a spike position" mask on the device, which keeps the decode
step graph-capturable.

``EditPlan.mode = "reconstruct"`` is the literal reading of EP:126 for the ``sae``
cells: *encode, zero the selected latents, decode back and continue*,
``x <- bf16(b_dec + sum_j s_j a_j(x) W_dec[j])`` with ``s_j = 1 - alpha`` on the
ablated latents and 1 elsewhere.  The SAE's reconstruction error leaves the
stream, so no flagged row is ever a no-op and a cell with nothing ablated
(``cnt = 0``) is the *pure splice* control.  The hook encodes the flagged rows
(``sae.encode``, one kernel family at every row count) and splices them with
``ops.sae_splice_edit``; both are pure per-row functions with a fixed summation
order, so a row gives the same bits alone, inside a decode bucket, or taken from
a table of activations encoded earlier (:meth:`EditHook.use_table`).  Everything
is static-shape and free of host syncs (``ops.flag_compact`` lists the flagged
rows of a prefill on the device), so the hook sits inside the decode hipGraphs
like the error-preserving one.  Projection cells are unchanged.

``EditPlan.mode = "clamp"`` and ``"steer"`` *push* the selected latents of the ``sae``
cells towards per-row targets ``EditPlan.values`` (``c``, one per selected latent)
instead of removing them (``ops.latent_affine_edit``, the sibling of the
error-preserving kernel):

* ``clamp`` -- ``a'_j = (1 - alpha) a_j + alpha c_j``: at ``alpha = 1`` the latent is held
  at ``c_j`` whether or not it fires; ``c = 0`` is exactly the error-preserving ablation.
* ``steer`` -- ``a'_j = a_j + c_j``: the feature is added regardless of the input.  The
  plan's ``alpha`` is ignored in this mode.

An inactive latent is edited too, so a flagged row is a no-op only where
``alpha a_j == alpha c_j`` for every selected latent.  Same static shapes, no host
sync; projection cells are unchanged.

``sae_noise`` (kind 3) and ``proj_noise`` (kind 4) rows are the *norm-matched controls* of ``sae`` and ``proj``
rows (``ops.matched_noise_edit``): at the same positions, the residual moves exactly as far as the targeted edit
would move it (``|sum_j c_j D_j|_2``, the coefficients computed by the same device code), but along a Gaussian
direction drawn from ``(EditPlan.seeds[row], absolute position)``.  A position therefore gets the same edit in a
prefill, a teacher-forced tail and a decode step, and a row where the targeted edit is an exact no-op is one for
the control too.  ``reconstruct`` replaces the residual instead of adding a delta to it, so it has no such control.

``sae_swap`` (kind 5) and ``proj_swap`` (kind 6) rows are *interchange interventions* (``ops.interchange_edit``): at
the row's spike positions the selected latents (kind 5) or the coordinates in the span of the row's basis rows
(kind 6) are set to the values they have in a *donor* residual, and everything else -- the SAE error, every other
latent, the orthogonal complement -- stays.  Where the other kinds test necessity (does the readout drop when these
coordinates go?), these test sufficiency and specificity (do they carry *which* secret it is?).  The donor rows
live in ``EditPlan.donor [R, D]``; the donor of plan row ``b`` at its ``k``-th spike is ``donor[donor_base[b] + k]``
(``donor_base < 0``: that row is left alone), which the hook resolves on the device as it does the activation table
of the reconstruct mode, so the path stays static-shape and free of host syncs.  For ``sae_swap`` rows ``alpha``
interpolates between the row's own activations (0) and the donor's (1); ``proj_swap`` rows take the donor's
coordinates outright, as ``proj`` rows are projected out outright.  A row that equals its donor row is an exact
no-op.  A swap row needs a donor per spike, so it cannot edit at ``ALL_POSITIONS``, and ``sae_swap`` is defined for
the error-preserving mode only.  A plan without swap rows runs exactly the calls it ran before these kinds existed.

:class:`TraceHook` edits nothing: listed at the hooked layer behind the edit hook and at every later block of a packed
pass, it reads out the capped lens logit of each row's tracked tokens (``ops.lens_track``), the layer trace of the
sweep (``intervention.layer_trace``).

:class:`ComponentHook` edits nothing either: it splits the lens logit of selected rows into the direct term at the
hooked layer and one term per attention head and per MLP of every later block (``ops.seg_dots``), the direct logit
attribution behind an edit.  It is listed at the hooked layer behind the edit hook, as a sub-hook
(``forward_packed(sub_hooks=)``) at every later block, and at the last block.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import ops


@dataclass
class EditPlan:
    """Device tensors, one row per sequence in the batch."""

    spikes: torch.Tensor                 # [B, K] int32 absolute positions, -1 = unused
    kind: torch.Tensor                   # [B] int8: 0 none, 1 sae, 2 proj, 3 sae_noise, 4 proj_noise, 5 sae_swap,
                                         # 6 proj_swap
    idx: torch.Tensor                    # [B, mmax] int32 (latent ids, or rows of the basis table)
    cnt: torch.Tensor                    # [B] int32
    alpha: float = 1.0
    basis: Optional[torch.Tensor] = None   # [n_rows, D] fp32 table of orthonormal basis rows (proj cells)
    mode: str = "error_preserving"         # sae cells: or "reconstruct" (splice the SAE reconstruction in)
    any_position: bool = False             # some row edits at ALL_POSITIONS (bounds the flagged rows of a forward)
    values: Optional[torch.Tensor] = None  # [B, mmax] fp32 targets c of the selected latents (clamp / steer modes)
    seeds: Optional[torch.Tensor] = None   # [B] int64 noise streams of the sae_noise / proj_noise rows
    has_noise: tuple = (False, False)      # host-known: some row has kind 3 / kind 4 (set by build)
    donor: Optional[torch.Tensor] = None   # [R, D] donor residuals of the sae_swap / proj_swap rows (model dtype)
    # [B] int32: row b's k-th spike reads donor[donor_base[b] + k]; < 0: no donor
    donor_base: Optional[torch.Tensor] = None
    has_swap: tuple = (False, False)       # host-known: some row has kind 5 / kind 6 (set by build)

    def __post_init__(self):
        check_mode(self.mode)
        if any(self.has_swap):
            if self.donor is None or self.donor_base is None:
                raise ValueError("EditPlan: sae_swap / proj_swap rows need donor ([R, D]) and donor_base ([B] int32)")
            if self.any_position and bool(((self.kind >= 5).view(-1, 1) & (self.spikes == ALL_POSITIONS)).any()):
                raise ValueError("EditPlan: sae_swap / proj_swap rows cannot be combined with ALL_POSITIONS spikes "
                                 "(a donor row exists per spike only)")
            if self.has_swap[0] and self.mode != "error_preserving":
                raise ValueError(f"EditPlan: sae_swap is defined for ablation_mode = error_preserving only, not "
                                 f"{self.mode!r}")
        if self.donor is not None and self.donor.dim() != 2:
            raise ValueError("EditPlan.donor must be [R, D]")
        if self.donor_base is not None and (self.donor_base.dtype != torch.int32
                                            or self.donor_base.numel() != self.kind.numel()):
            raise ValueError("EditPlan.donor_base must be [B] int32")
        if any(self.has_noise):
            if self.seeds is None:
                raise ValueError("EditPlan: sae_noise / proj_noise rows need seeds ([B] int64)")
            if self.has_noise[0] and self.mode == "reconstruct":
                raise ValueError("EditPlan: sae_noise has no meaning under ablation_mode = reconstruct (the splice "
                                 "replaces the residual: there is no added delta whose norm could be matched)")
        if self.seeds is not None and (self.seeds.dtype != torch.int64 or self.seeds.numel() != self.kind.numel()):
            raise ValueError("EditPlan.seeds must be [B] int64")
        if self.mode in AFFINE_MODES and self.values is None:
            self.values = torch.zeros(self.idx.shape, dtype=torch.float32, device=self.idx.device)
        if self.values is not None and tuple(self.values.shape) != tuple(self.idx.shape):
            raise ValueError(f"EditPlan.values must be [B, mmax] like idx {tuple(self.idx.shape)}, "
                             f"not {tuple(self.values.shape)}")

    @property
    def B(self) -> int:
        return int(self.spikes.shape[0])

    @staticmethod
    def build(device, spikes: Sequence[Sequence[int]], kinds: Sequence[str], sel: Sequence[Sequence[int]],
              alpha: float = 1.0, basis: Optional[torch.Tensor] = None, kmax: Optional[int] = None,
              mmax: Optional[int] = None, mode: str = "error_preserving", values=None, seeds=None,
              noise: Optional[tuple] = None, donor: Optional[torch.Tensor] = None, donor_base=None,
              swap: Optional[tuple] = None) -> "EditPlan":
        """``values`` (clamp / steer modes): the targets of the selected latents, one scalar for all of them or a
        per-row list of lists aligned with ``sel``.  ``seeds``: one int per row, required with ``sae_noise`` /
        ``proj_noise`` rows (taken mod 2^64).  ``noise``: which noise paths (``sae_noise``, ``proj_noise``) the hook
        keeps, for a plan that is refilled in place; default: those of ``kinds``.  ``donor [R, D]`` / ``donor_base``
        (one int per row, < 0: no donor): the donor residuals of the ``sae_swap`` / ``proj_swap`` rows; ``swap``: which
        swap paths the hook keeps, as ``noise``."""
        B = len(spikes)
        kmax = kmax or max(1, max((len(s) for s in spikes), default=1))
        mmax = mmax or max(1, max((len(s) for s in sel), default=1))
        sp = np.full((B, kmax), -1, dtype=np.int32)
        ix = np.zeros((B, mmax), dtype=np.int32)
        cn = np.zeros((B,), dtype=np.int32)
        kd = np.asarray([KIND_CODES[k] for k in kinds], dtype=np.int8)
        for b in range(B):
            s = spikes[b]
            if len(s):
                s = list(s)[:kmax]
                sp[b, : len(s)] = s
            m = sel[b]
            if len(m):
                m = list(m)[:mmax]
                ix[b, : len(m)] = m
                cn[b] = len(m)
        t = lambda a: torch.from_numpy(a).to(device)   # noqa: E731
        vals = None
        if values is not None:
            va = np.zeros((B, mmax), dtype=np.float32)
            if isinstance(values, (int, float, np.number)):
                va[:] = float(values)
            else:
                if len(values) != B:
                    raise ValueError(f"EditPlan.build: values has {len(values)} rows, sel has {B}")
                for b in range(B):
                    if len(values[b]) != len(sel[b]):
                        raise ValueError(f"EditPlan.build: values[{b}] has {len(values[b])} entries, "
                                         f"sel[{b}] has {len(sel[b])}")
                    n = min(len(values[b]), mmax)
                    va[b, :n] = np.asarray(list(values[b])[:n], dtype=np.float32)
            vals = t(va)
        sd = None
        if seeds is not None:
            if len(seeds) != B:
                raise ValueError(f"EditPlan.build: seeds has {len(seeds)} rows, sel has {B}")
            sd = t(seeds_to_int64(seeds))
        db = None
        if donor_base is not None:
            if len(donor_base) != B:
                raise ValueError(f"EditPlan.build: donor_base has {len(donor_base)} rows, sel has {B}")
            db = t(np.asarray([int(v) for v in donor_base], dtype=np.int32))
        return EditPlan(t(sp), t(kd), t(ix), t(cn), alpha, basis.to(device) if basis is not None else None, mode,
                        bool((sp == ALL_POSITIONS).any()), vals, sd,
                        tuple(noise) if noise is not None else (bool((kd == 3).any()), bool((kd == 4).any())),
                        donor.to(device) if donor is not None else None, db,
                        tuple(swap) if swap is not None else (bool((kd == 5).any()), bool((kd == 6).any())))


KIND_CODES = {"none": 0, "sae": 1, "proj": 2, "sae_noise": 3, "proj_noise": 4, "sae_swap": 5, "proj_swap": 6}


def seeds_to_int64(seeds) -> np.ndarray:
    """Python ints (any size) as the int64 array whose bits are the seeds mod 2^64 (the kernel reads them unsigned)."""
    return np.asarray([int(s) & ((1 << 64) - 1) for s in seeds], dtype=np.uint64).view(np.int64)


ALL_POSITIONS = -2   # spike value that matches every (non-padding) position: position-agnostic edits
ABLATION_MODES = ("error_preserving", "reconstruct", "clamp", "steer")
AFFINE_MODES = ("clamp", "steer")      # sae cells pushed towards EditPlan.values (ops.latent_affine_edit)


def check_mode(mode: str, clamp_value: Optional[float] = None) -> str:
    """The mode, validated; with ``clamp_value`` (the pipelines pass ``intervention.clamp_value``) also that a
    ``steer`` run adds something."""
    if mode not in ABLATION_MODES:
        raise ValueError(f"intervention.ablation_mode must be one of {', '.join(ABLATION_MODES)}, not {mode!r}")
    if mode == "steer" and clamp_value is not None and float(clamp_value) == 0.0:
        raise ValueError("intervention.ablation_mode = steer needs a non-zero intervention.clamp_value "
                         "(adding 0 leaves every cell at its baseline)")
    return mode


def spike_mask(pos: torch.Tensor, spikes: torch.Tensor, B: int, T: int) -> torch.Tensor:
    """[B*T] bool: row position is one of its sequence's spike positions (``ALL_POSITIONS`` = any)."""
    p = pos.view(B, T, 1)
    sp = spikes.view(B, 1, -1)
    hit = ((p == sp) | (sp == ALL_POSITIONS)) & (p >= 0)
    return hit.any(-1).view(B * T)


class EditHook:
    """Layer hook applying an :class:`EditPlan` (both SAE and projection cells) in place."""

    def __init__(self, plan: EditPlan, sae=None):
        self.plan = plan
        self.sae = sae
        self._bufs = {}
        self._table = None
        if plan.mode == "reconstruct" and sae is not None and sae.d_in % 8:
            raise ValueError("reconstruct mode needs a residual width that is a multiple of 8")

    def use_table(self, acts: Optional[torch.Tensor], base: Optional[torch.Tensor] = None) -> None:
        """Reconstruct mode: take the flagged rows' activations from ``acts [R, d_sae]`` (encoded earlier from
        the very residuals this forward is fed, e.g. a pair's baseline residuals at its spikes) instead of
        encoding them: the row of plan row ``b`` at its ``k``-th spike is ``acts[base[b] + k]`` (``base [B]``
        int32, < 0: that plan row is left unedited).  ``use_table(None)`` returns to fresh encodes."""
        self._table = None if acts is None else (acts, base)

    def _rows(self, B: int, T: int, device):
        # per stream: the sweep runs the ride-along decode and the teacher-forced tail concurrently
        sid = torch.cuda.current_stream(device).stream_id if device.type == "cuda" else 0
        key = (B, T, sid)
        b = self._bufs.get(key)
        if b is None:
            mmax = self.plan.idx.shape[1]
            b = {
                "idx": torch.empty(B * T, mmax, dtype=torch.int32, device=device),
                "cnt": torch.empty(B * T, dtype=torch.int32, device=device),
                "apply_sae": torch.empty(B * T, dtype=torch.uint8, device=device),
                "apply_proj": torch.empty(B * T, dtype=torch.uint8, device=device),
                "coef": torch.zeros(B * T, mmax, dtype=torch.float32, device=device),
            }
            if self.plan.mode in AFFINE_MODES:
                b["val"] = torch.empty(B * T, mmax, dtype=torch.float32, device=device)
            if any(self.plan.has_noise):
                b["apply_noise"] = torch.empty(B * T, dtype=torch.uint8, device=device)
                b["seeds"] = torch.empty(B * T, dtype=torch.int64, device=device)
            if any(self.plan.has_swap):
                b["apply_swap"] = torch.empty(B * T, dtype=torch.uint8, device=device)
                b["donor_src"] = torch.empty(B * T, dtype=torch.int32, device=device)
            if self.plan.mode == "reconstruct" and self.sae is not None:
                b["src"] = torch.empty(B * T, dtype=torch.int32, device=device)
                cap = self._capacity(B, T)
                if cap < B * T:
                    b["rows"] = torch.empty(cap, dtype=torch.int32, device=device)
            self._bufs[key] = b
        return b

    def __call__(self, h: torch.Tensor, x: torch.Tensor, ctx) -> None:
        """Rows are matched to plan rows through their cache slot (``ctx.slot``), so a forward over
        any subset of the batch (e.g. a prefill of a few rows) applies the right per-row edit."""
        B, T = ctx.B, ctx.T
        pl = self.plan
        r = self._rows(B, T, h.device)
        sl = ctx.slot.long()
        spikes = pl.spikes.index_select(0, sl)
        hit = spike_mask(ctx.pos, spikes, B, T)
        kind = pl.kind.index_select(0, sl).view(B, 1).expand(B, T).reshape(B * T)
        r["apply_sae"].copy_(hit & (kind == 1))
        r["apply_proj"].copy_(hit & (kind == 2))
        r["idx"].view(B, T, -1).copy_(pl.idx.index_select(0, sl).view(B, 1, -1).expand(B, T, -1))
        r["cnt"].view(B, T).copy_(pl.cnt.index_select(0, sl).view(B, 1).expand(B, T))
        if self.sae is not None and pl.mode == "reconstruct":
            self._splice(h, x, ctx, r, spikes)
        elif self.sae is not None and pl.mode in AFFINE_MODES:
            # clamp: alpha and val = fl32(alpha * c); steer: alpha = 0 and val = c (the plan's alpha is ignored)
            s = self.sae
            c = pl.values.index_select(0, sl)
            alpha = pl.alpha if pl.mode == "clamp" else 0.0
            r["val"].view(B, T, -1).copy_((c * alpha if pl.mode == "clamp" else c).view(B, 1, -1).expand(B, T, -1))
            ops.latent_affine_edit(h, r["apply_sae"], r["idx"], r["cnt"], r["val"], s.W_encT, s.W_dec, s.b_enc,
                                   s.threshold, s.b_dec if s.apply_b_dec_to_input else None, alpha, ctx.w_next,
                                   ctx.eps, x, r["coef"])
        elif self.sae is not None:
            s = self.sae
            ops.lowrank_edit(h, r["apply_sae"], r["idx"], r["cnt"], s.W_encT, s.W_dec, s.b_enc, s.threshold,
                             s.b_dec if s.apply_b_dec_to_input else None, pl.alpha, ctx.w_next, ctx.eps, x,
                             r["coef"])
        if pl.basis is not None:
            ops.lowrank_edit(h, r["apply_proj"], r["idx"], r["cnt"], pl.basis, pl.basis, None, None, None, 1.0,
                             ctx.w_next, ctx.eps, x, None)
        if any(pl.has_noise):
            self._noise(h, x, ctx, r, hit, kind, sl)
        if any(pl.has_swap):
            self._swap(h, x, ctx, r, hit, kind, sl, spikes)

    def _swap(self, h, x, ctx, r, hit, kind, sl, spikes) -> None:
        """The interchange rows: kind 5 with the SAE tables, kind 6 with the plan's basis.  ``src`` is the donor row
        of the first matching spike (as :meth:`_splice` reads its table), -1 where the row is no flagged swap row."""
        B, T = ctx.B, ctx.T
        pl = self.plan
        swap = hit & (kind >= 5)
        k = (ctx.pos.view(B, T, 1) == spikes.view(B, 1, -1)).to(torch.int32).argmax(-1)          # first matching spike
        b0 = pl.donor_base.index_select(0, sl).view(B, 1)
        src = torch.where(b0 >= 0, b0 + k, torch.full_like(k, -1)).view(B * T)
        r["donor_src"].copy_(torch.where(swap, src, torch.full_like(src, -1)))
        if pl.has_swap[0]:
            if self.sae is None:
                raise ValueError("EditPlan has sae_swap rows but the hook has no SAE")
            s = self.sae
            r["apply_swap"].copy_(hit & (kind == 5))
            ops.interchange_edit(h, r["apply_swap"], r["idx"], r["cnt"], s.W_encT, s.W_dec, pl.donor, r["donor_src"],
                                 s.b_enc, s.threshold, s.b_dec if s.apply_b_dec_to_input else None, pl.alpha,
                                 ctx.w_next, ctx.eps, x, r["coef"])
        if pl.has_swap[1]:
            if pl.basis is None:
                raise ValueError("EditPlan has proj_swap rows but no basis")
            r["apply_swap"].copy_(hit & (kind == 6))
            ops.interchange_edit(h, r["apply_swap"], r["idx"], r["cnt"], pl.basis, pl.basis, pl.donor,
                                 r["donor_src"], None, None, None, 1.0, ctx.w_next, ctx.eps, x)

    def _noise(self, h, x, ctx, r, hit, kind, sl) -> None:
        """The norm-matched controls: kind-3 rows with the SAE tables (and the clamp / steer targets, built as for
        the targeted rows), kind-4 rows with the plan's basis.  A row is flagged by one kind only, so the order of
        the calls does not matter."""
        B, T = ctx.B, ctx.T
        pl = self.plan
        r["seeds"].view(B, T).copy_(pl.seeds.index_select(0, sl).view(B, 1).expand(B, T))
        pos = ctx.pos.view(B * T)
        if pl.has_noise[0]:
            if self.sae is None:
                raise ValueError("EditPlan has sae_noise rows but the hook has no SAE")
            s = self.sae
            r["apply_noise"].copy_(hit & (kind == 3))
            affine = pl.mode in AFFINE_MODES          # r["val"] was filled above, as for the targeted rows
            alpha = 0.0 if pl.mode == "steer" else pl.alpha
            ops.matched_noise_edit(h, r["apply_noise"], r["idx"], r["cnt"], s.W_encT, s.W_dec, r["seeds"], pos,
                                   r["val"] if affine else None, s.b_enc, s.threshold,
                                   s.b_dec if s.apply_b_dec_to_input else None, alpha, ctx.w_next, ctx.eps, x,
                                   r["coef"])
        if pl.has_noise[1]:
            if pl.basis is None:
                raise ValueError("EditPlan has proj_noise rows but no basis")
            r["apply_noise"].copy_(hit & (kind == 4))
            ops.matched_noise_edit(h, r["apply_noise"], r["idx"], r["cnt"], pl.basis, pl.basis, r["seeds"], pos,
                                   None, None, None, None, 1.0, ctx.w_next, ctx.eps, x)

    def _capacity(self, B: int, T: int) -> int:
        """Host-known bound on the flagged rows of a ``[B, T]`` forward: a sequence is edited at no more than its
        plan row's K spike positions, or anywhere under ``ALL_POSITIONS``."""
        K = int(self.plan.spikes.shape[1])
        return B * T if self.plan.any_position else min(B * T, B * K)

    def _splice(self, h, x, ctx, r, spikes) -> None:
        """Reconstruct mode for the flagged ``sae`` rows: activations from the table set by :meth:`use_table`,
        else encoded here -- the whole bucket when every row can be flagged (decode steps, ``ALL_POSITIONS``),
        otherwise only the rows ``ops.flag_compact`` lists (a prefill of ``B * T`` rows edits at most ``B * K``)."""
        B, T = ctx.B, ctx.T
        pl, s = self.plan, self.sae
        M = B * T
        hv = h.view(M, -1)
        src = r["src"]
        if self._table is not None:
            acts, base = self._table
            k = (ctx.pos.view(B, T, 1) == spikes.view(B, 1, -1)).to(torch.int32).argmax(-1)      # first matching spike
            b0 = base.index_select(0, ctx.slot.long()).view(B, 1)
            r["src"].view(B, T).copy_(torch.where(b0 >= 0, b0 + k, torch.full_like(k, -1)))
        elif "rows" in r:
            ops.flag_compact(r["apply_sae"], r["rows"].numel(), rows=r["rows"], inv=r["src"])
            acts = s.encode(hv.index_select(0, r["rows"].clamp_min(0).long()))
        else:
            acts, src = s.encode(hv), None            # row i of the bucket reads acts[i]
        ops.sae_splice_edit(hv, r["apply_sae"], acts, r["idx"], r["cnt"], s.W_dec, s.b_dec, pl.alpha, ctx.w_next,
                            ctx.eps, x.view(M, -1), src)

    def ablated_activation(self) -> Optional[torch.Tensor]:
        """Per-row activations of the ablated latents from the last call (diagnostics)."""
        for v in self._bufs.values():
            return v["coef"]
        return None


class CaptureHook:
    """Copies ``h`` rows into ``store[slot, pos]`` (device scatter; graph-capturable).

    ``store`` is ``[slots, S + 1, D]``: positions ``0..S-1`` are real, index ``S``
    of each slot is a scratch row that absorbs padding rows, so the scatter
    needs no data-dependent shapes.
    """

    def __init__(self, store: torch.Tensor):
        self.store = store

    def __call__(self, h: torch.Tensor, x: torch.Tensor, ctx) -> None:
        ops.capture_rows(self.store, h, ctx.pos, ctx.slot, ctx.B, ctx.T)


class TraceHook:
    """Layer trace: the tracked tokens' capped lens logits of the residual rows at every block from ``first`` on
    (``ops.lens_track``).  Holds the launch's table ``V [U, T, D]`` fp32 (one block of lens directions per pair), the
    row map ``rows [M]`` int32 (the table block of every row of the launch) and the output ``out [Lt, M, T]`` fp32,
    ``Lt`` blocks from ``first``; one instance is listed at each of those blocks, at block ``first`` after the edit
    hook, so it sees the edited rows.  A call at block ``l`` reads the rows of the current window into slab
    ``l - first``.

    A packed forward runs one chunk of the launch's rows, padded to whole GEMM tiles: :meth:`use_rows` sets the
    chunk's window ``[r0, r1)`` before each forward (as :meth:`EditHook.use_table` sets the splice table), and builds
    the chunk's map -- its rows' table blocks, -1 on the padding rows, which the kernel skips.  Shapes are static
    per chunk and nothing syncs with the host."""

    def __init__(self, V: torch.Tensor, rows: torch.Tensor, out: torch.Tensor, first: int, eps: float, cap: float):
        if V.dim() != 3 or out.dim() != 3 or out.shape[1] != rows.shape[0] or out.shape[2] != V.shape[1]:
            raise ValueError(f"TraceHook: V [U, T, D], rows [M] and out [Lt, M, T] do not fit: {tuple(V.shape)}, "
                             f"{tuple(rows.shape)}, {tuple(out.shape)}")
        if rows.dtype != torch.int32:
            raise ValueError("TraceHook: rows must be int32")
        self.V, self.rows, self.out = V, rows, out
        self.first, self.eps, self.cap = int(first), float(eps), float(cap)
        self.calls = 0
        self.use_rows(0, rows.shape[0])

    @property
    def layers(self) -> range:
        return range(self.first, self.first + self.out.shape[0])

    def use_rows(self, r0: int, r1: int, padded: Optional[int] = None) -> None:
        """The next forwards run rows ``[r0, r1)`` of the launch, followed by padding rows up to ``padded`` rows."""
        n = r1 - r0
        padded = n if padded is None else int(padded)
        if not 0 <= r0 <= r1 <= self.rows.shape[0] or padded < n:
            raise ValueError(f"TraceHook.use_rows: window [{r0}, {r1}) padded to {padded} does not fit "
                             f"{self.rows.shape[0]} rows")
        self._win = (r0, r1)
        if padded == n:
            self._map, self._tmp = self.rows[r0:r1], None
        else:
            self._map = torch.full((padded,), -1, dtype=torch.int32, device=self.rows.device)
            self._map[:n].copy_(self.rows[r0:r1])
            self._tmp = torch.empty(padded, self.out.shape[2], dtype=torch.float32, device=self.rows.device)

    def __call__(self, h: torch.Tensor, x: torch.Tensor, ctx) -> None:
        k = ctx.layer - self.first
        if not 0 <= k < self.out.shape[0]:
            raise ValueError(f"TraceHook: called at block {ctx.layer}, traces blocks {self.first}.."
                             f"{self.first + self.out.shape[0] - 1}")
        r0, r1 = self._win
        hv = h.view(-1, h.shape[-1])
        if hv.shape[0] != self._map.shape[0]:
            raise ValueError(f"TraceHook: the forward has {hv.shape[0]} rows, the window set by use_rows "
                             f"{self._map.shape[0]}")
        self.calls += 1
        if self._tmp is None:
            ops.lens_track(hv, self.V, self._map, self.eps, self.cap, out=self.out[k, r0:r1])
        else:
            ops.lens_track(hv, self.V, self._map, self.eps, self.cap, out=self._tmp)
            self.out[k, r0:r1].copy_(self._tmp[: r1 - r0])


def component_tables(model, first: int, ids: Sequence[Optional[int]], T: int = 2):
    """The component trace's tables of one pair, blocks ``first + 1 .. layers - 1``: ``A [Lc, T, heads * head_dim]``
    with ``A_b = ((1 + ln_post_attn_b) * v) @ W_o,b``, ``F [Lc, T, D]`` with ``F_b = (1 + ln_post_ffn_b) * v`` and the
    lens directions ``Vd [T, D]`` (``v`` of ``lens_direction``), column ``j`` for ``ids[j]``; a missing or
    out-of-vocabulary id leaves a zero column.  Built in fp64 and rounded once to fp32."""
    from .gradient import lens_direction

    w, s = model.w, model.spec
    ids = list(ids)
    if not 1 <= len(ids) <= T:
        raise ValueError(f"component_tables: 1 to {T} ids, not {len(ids)}")
    if not 0 <= first < s.layers - 1:
        raise ValueError(f"component_tables: no block behind block {first} of {s.layers}")
    dev = w.lm_head.device
    v = torch.zeros(T, s.hidden, dtype=torch.float64, device=dev)
    for j, t in enumerate(ids):
        if t is not None and 0 <= int(t) < w.lm_head.shape[0]:
            v[j] = lens_direction(model, [int(t)]).double()
    A, F = [], []
    for l in range(first + 1, s.layers):
        L = w.layers[l]
        A.append(((1.0 + L.ln_post_attn.double()) * v) @ L.wo.double())
        F.append((1.0 + L.ln_post_ffn.double()) * v)
    return torch.stack(A).float().contiguous(), torch.stack(F).float().contiguous(), v.float().contiguous()


class ComponentHook:
    """Component trace: per-head and per-MLP direct contributions to the lens logit of selected rows
    (``ops.seg_dots``).  Holds the launch's tables ``A [Lc, U, T, heads * head_dim]``, ``F [Lc, U, T, D]`` and
    ``Vd [U, T, D]`` fp32 (:func:`component_tables`, one block per pair), the selected rows ``sel [Ms]`` of the launch
    (int32, ascending) with their table blocks ``sblk [Ms]``, and the outputs, all numerators over the sublayer's own
    RMS but not yet over ``rho_f``:

    * ``direct [Ms, T]``: ``h_l . v`` at the hooked layer ``first`` (listed there behind the edit hook);
    * ``comp [Lc, Ms, T, heads + 1]``: heads ``0 .. heads - 1``, then the MLP, of blocks ``first + 1 .. layers - 1``
      (:meth:`sub` listed as a sub-hook at each of them);
    * ``total [Ms, T]`` and ``rho_f [Ms]``: ``(h_last . v) / rho_f`` and ``rho_f = rho(h_last)`` (listed at the last
      block).

    A packed forward runs one chunk of the launch's rows: :meth:`use_rows` sets the chunk's window before each
    forward, as :meth:`TraceHook.use_rows` does.  The selection is sorted, so a window's selected rows are a slice
    known on the host: the kernel launches over that slice alone, shapes are static per chunk and nothing syncs with
    the host (pass ``sel_host`` with a device ``sel``)."""

    def __init__(self, A: torch.Tensor, F: torch.Tensor, Vd: torch.Tensor, sel: torch.Tensor, sblk: torch.Tensor,
                 first: int, heads: int, eps: float, out: Optional[torch.Tensor] = None,
                 sel_host: Optional[Sequence[int]] = None):
        if (A.dim() != 4 or F.dim() != 4 or Vd.dim() != 3 or A.shape[:3] != F.shape[:3] or A.shape[0] < 1
                or tuple(A.shape[1:3]) != tuple(Vd.shape[:2]) or F.shape[3] != Vd.shape[2] or A.shape[3] % heads):
            raise ValueError(f"ComponentHook: A [Lc, U, T, heads * head_dim], F [Lc, U, T, D] and Vd [U, T, D] do not "
                             f"fit: {tuple(A.shape)}, {tuple(F.shape)}, {tuple(Vd.shape)}")
        if sel.dtype != torch.int32 or sblk.dtype != torch.int32 or sel.dim() != 1 or sblk.shape != sel.shape:
            raise ValueError("ComponentHook: sel and sblk must be [Ms] int32")
        T, D = Vd.shape[1], Vd.shape[2]
        ops.seg_dots_check(A.shape[3], heads, T, D, "ComponentHook")
        ops.seg_dots_check(D, 1, T, D, "ComponentHook")
        # the host's copy of the selection (``sel_host``: the caller's, so a device ``sel`` is not read back)
        self._sel = [int(r) for r in (sel.tolist() if sel_host is None else sel_host)]
        if len(self._sel) != sel.shape[0]:
            raise ValueError("ComponentHook: sel_host must list the rows of sel")
        if any(b <= a for a, b in zip(self._sel, self._sel[1:])) or (self._sel and self._sel[0] < 0):
            raise ValueError("ComponentHook: the selected rows must be ascending launch rows")
        self.A, self.F, self.Vd, self.sel, self.sblk = A, F, Vd, sel, sblk
        self.first, self.heads, self.eps = int(first), int(heads), float(eps)
        Lc, Ms, dev = A.shape[0], sel.shape[0], A.device
        # the four outputs are views of one flat fp32 buffer (``out``: the caller's, so they can ride in its one
        # device-to-host copy; :meth:`split` cuts the host copy the same way)
        n = self.out_numel(Lc, Ms, T, heads)
        if out is None:
            out = torch.zeros(n, dtype=torch.float32, device=dev)
        elif out.shape != (n,) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise ValueError(f"ComponentHook: out must be a contiguous [{n}] float32 on the tables' device")
        else:
            out.zero_()
        self.out = out
        self.comp, self.direct, self.total, self.rho_f = self.split(out, Lc, Ms, T, heads)
        self.calls = 0
        self.use_rows(0, (self._sel[-1] + 1) if self._sel else 0)

    @staticmethod
    def out_numel(Lc: int, Ms: int, T: int, heads: int) -> int:
        return Ms * (T * (Lc * (heads + 1) + 2) + 1)

    @staticmethod
    def split(flat, Lc: int, Ms: int, T: int, heads: int):
        """``(comp [Lc, Ms, T, heads + 1], direct [Ms, T], total [Ms, T], rho_f [Ms])`` as views of a flat buffer."""
        a = Lc * Ms * T * (heads + 1)
        b = a + Ms * T
        c = b + Ms * T
        return (flat[:a].reshape(Lc, Ms, T, heads + 1), flat[a:b].reshape(Ms, T), flat[b:c].reshape(Ms, T),
                flat[c:c + Ms])

    @property
    def layers(self) -> range:
        """The blocks whose sublayers are read."""
        return range(self.first + 1, self.first + 1 + self.A.shape[0])

    @property
    def last(self) -> int:
        return self.first + self.A.shape[0]

    def use_rows(self, r0: int, r1: int, padded: Optional[int] = None) -> None:
        """The next forwards run rows ``[r0, r1)`` of the launch, followed by padding rows up to ``padded`` rows."""
        import bisect

        n = r1 - r0
        padded = n if padded is None else int(padded)
        if not 0 <= r0 <= r1 or padded < n:
            raise ValueError(f"ComponentHook.use_rows: window [{r0}, {r1}) padded to {padded}")
        i0, i1 = bisect.bisect_left(self._sel, r0), bisect.bisect_left(self._sel, r1)
        self._sl, self._n = (i0, i1), padded
        k, T, dev = i1 - i0, self.Vd.shape[1], self.sel.device
        self._rows = self.sel[i0:i1] - r0
        self._blk = self.sblk[i0:i1].contiguous()
        self._th = torch.empty(k, T, self.heads, dtype=torch.float32, device=dev)
        self._t1 = torch.empty(k, T, 1, dtype=torch.float32, device=dev)
        self._rms = torch.empty(k, dtype=torch.float32, device=dev)

    def _rows_of(self, t: torch.Tensor, what: str) -> torch.Tensor:
        v = t.view(-1, t.shape[-1])
        if v.shape[0] != self._n:
            raise ValueError(f"ComponentHook: the forward has {v.shape[0]} {what} rows, the window set by use_rows "
                             f"{self._n}")
        return v

    def __call__(self, h: torch.Tensor, x: torch.Tensor, ctx) -> None:
        if ctx.layer not in (self.first, self.last):
            raise ValueError(f"ComponentHook: called at block {ctx.layer}, listed at blocks {self.first} and "
                             f"{self.last}")
        hv = self._rows_of(h, "residual")
        i0, i1 = self._sl
        if i0 == i1:
            return
        self.calls += 1
        if ctx.layer == self.first:
            ops.seg_dots(hv, self.Vd, self._rows, self._blk, 1, None, self.eps, out=self._t1, rms=self._rms)
            self.direct[i0:i1].copy_(self._t1[:, :, 0])
        else:
            ops.seg_dots(hv, self.Vd, self._rows, self._blk, 1, hv, self.eps, out=self._t1, rms=self._rms)
            self.total[i0:i1].copy_(self._t1[:, :, 0])
            self.rho_f[i0:i1].copy_(self._rms)

    def sub(self, kind: str, inp: torch.Tensor, o: torch.Tensor, ctx) -> None:
        """The sub-hook: ``("attn", ws.attn, ws.o)`` and ``("ffn", ws.act, ws.o)`` of a block in :attr:`layers`."""
        k = ctx.layer - self.first - 1
        if not 0 <= k < self.A.shape[0] or kind not in ("attn", "ffn"):
            raise ValueError(f"ComponentHook.sub: {kind!r} at block {ctx.layer}, reads attn / ffn of blocks "
                             f"{self.first + 1}..{self.last}")
        ov = self._rows_of(o, "sublayer")
        i0, i1 = self._sl
        if i0 == i1:
            return
        self.calls += 1
        if kind == "attn":
            ops.seg_dots(self._rows_of(inp, "attention"), self.A[k], self._rows, self._blk, self.heads, ov, self.eps,
                         out=self._th, rms=self._rms)
            self.comp[k, i0:i1, :, : self.heads].copy_(self._th)
        else:
            ops.seg_dots(ov, self.F[k], self._rows, self._blk, 1, ov, self.eps, out=self._t1, rms=self._rms)
            self.comp[k, i0:i1, :, self.heads].copy_(self._t1[:, :, 0])
