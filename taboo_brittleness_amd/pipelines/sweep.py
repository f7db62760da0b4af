"""Targeted-vs-random intervention sweep (EP:112-152).

Per (word, prompt) *pair* a baseline hint is generated and read out; per
*cell* — (pair, method ∈ {sae_targeted, sae_random, proj_targeted,
proj_random}, budget m or rank r, trial) — the hint is regenerated with the
edit applied at the pair's spike positions of the hooked layer, then read out:

* content: logit-lens secret probability at the hooked layer over the
  response (mean / final / max) and the LL-Top-k guesses (EP:132);
* fluency: ΔNLL of the *unedited* hint under the edited vs the original model
  (teacher forced, edit at the same positions; EP:136);
* leak: the regenerated hint literally contains the secret (EP:136).

Execution is batched: every batch of cells shares one :class:`Generator`
(one KV cache, hipGraph-captured decode step replayed across batches) and one
persistent edit plan whose tensors are refreshed in place, so capture happens
once per sweep.  Cells are enumerated deterministically and seeded per cell
(SURVEY 7.3.14); data-parallel ranks own whole (word, prompt) pairs -- contiguous
blocks of pairs, every cell of a pair on its pair's rank
(``pipelines.run_sweep.pair_owners``).

Prefix sharing (``runtime.prefix_share``, exact): an edited cell computes
exactly what its pair's baseline computed up to the first edited position f
(same prompt, same greedy tokens, no edit yet).  The baseline's KV cache and
hooked-layer residuals for positions < f are therefore copied (device copies)
instead of recomputed: the cell resumes decoding at f, and the teacher-forced
ΔNLL pass only runs positions ≥ f, adding the baseline's per-token NLLs for
the earlier targets.  Baselines of the *next* pairs ride along in the same
decode batch, so their cost hides behind the cells'.

Layer resume (``_run_batch_resume``) adds three more exact reuse levels that rest on one fact: blocks
``0..l`` (l = hooked layer) see only tokens, the edit only touches the residual after block ``l``.

* prefix-trie decode — diverged cells of a pair with equal tokens since their divergence run blocks
  ``0..l`` once per group (``Generator.decode(share_keys=)``, keys from :meth:`SweepRunner._trie_keys`);
* lens row dedup — their hooked-layer residuals at unedited positions are identical, so those lens rows are
  unembedded once (:meth:`SweepRunner._lens_row_keys`, ``lens_packed(row_key=)``);
* no-op spike skip — a spike where none of a cell's ablated latents fires is an exact no-op edit, decided by
  the edit kernel itself on the baseline's residuals (:meth:`SweepRunner._spike_activity`), so the cell's
  teacher-forced tail starts at its first effective spike (``plan["f"]``).

``intervention.ablation_mode = reconstruct`` (the literal EP:126 reading: the residual at a spike is replaced by
the SAE's reconstruction with the ablated latents scaled) keeps every level but the last: no spliced row is a
no-op, so every ``sae`` cell's tail starts at its pair's first spike.  The tail's hooked-layer rows are the
baseline's own residuals, so their SAE activations are encoded once per pair (``Pair.splice_acts``, K rows) and the
tail splices from that table without encoding; only the decode steps of diverged cells encode fresh rows.  The mode
adds one ``sae_splice`` cell per pair (budget 0, nothing ablated): the pure-splice control.

``intervention.ablation_mode = clamp | steer`` push the selected latents towards ``intervention.clamp_value``
(interp/edits.py) with the error-preserving run's cells, latent selection and seeds.  An inactive latent is edited
too, so the no-op spike skip is off (every cell's tail starts at its pair's first spike and the activity table is
not built); every other level stays on and exact, the edit being a pure per-row function of the very rows the tail
feeds.

The swap methods (``SWAP_METHODS``: ``sae_swap``, ``sae_swap_random``, ``proj_swap``, ``proj_swap_random``; opt-in) are
*interchange interventions* (interp/edits.py, ``ops.interchange_edit``): at the pair's spikes the selected latents or
subspace coordinates take the values they have in a *donor* pair's residuals -- the next word's pair with the same
prompt, or the same word's next prompt (``intervention.swap_donor``).  The donor rows of a batch live in a
``[B * K, D]`` table of the edit plan, refilled on the device from the donor pairs' kept residuals.  A swap edit is
almost never a no-op, so the no-op spike skip is off for these cells; every other reuse level stays on and exact (the
edit is a pure per-row function of the tail's rows and of constant donor rows).  Their records also report the donor's
secret (``p_donor_*``, ``donor_leak``, ``donor_in_topk``); for that, every pair of a run with swap methods tracks the
other words' secret ids after its decoys (:meth:`SweepRunner.build_pairs`).  With one weight set for all words (the
offline random-init default) two words with the same prompt generate the same hint, so a ``next_word`` donor row can
coincide with the target's row where their spikes coincide: that spike is an exact no-op of the kernel.

``intervention.latent_score = effect_lens | attr_model`` changes only how ``Pair.targeted`` is ranked
(:meth:`SweepRunner._causal_scores`: the effect of ablating each active latent alone at the spikes on the secret's
lens logit, or its first-order attribution to the model's own logit); cells, seeds, random pools and every reuse
level are those of the default ``corr``.

``intervention.component_trace`` (opt-in) says which component behind the edit moved the secret: at every cell's edited
spike rows and the rows right behind them, the same two passes carry a :class:`~..interp.edits.ComponentHook` that
splits the uncapped lens logit of the last block's residual into the direct term at block ``l`` and one term per
attention head and per MLP of blocks ``l+1 ..`` (``ops.seg_dots``); the records' ``comp_*`` fields are the differences
edited minus baseline, each run over its own final RMS.

``intervention.layer_trace`` (opt-in) reads the blocks between the edit and the output: the teacher-forced tail and the
pairs' unedited pass of blocks ``l+1..`` carry a :class:`~..interp.edits.TraceHook` at blocks ``l .. layers - 1`` that
writes the capped lens logit of every row's tracked ids (``ops.lens_track``); the records' ``trace_*`` fields are the
per-block differences edited minus baseline at the spikes and over the response, and ``trace_recovery``, the share of
the direct effect that the later blocks undo.  Teacher-forced rows only: the decode rows of diverged cells are not
traced, and the decode hipGraphs never see the hook.

Module layout: this module holds the runner's driver (construction, baselines, ``run_cells``) and the
summaries; its methods are grouped by phase into mixins -- :mod:`.sweep_plan` (pair scoring, cells, edit bases
and plans, prefetch), :mod:`.sweep_decode` (one batch through the decode: layer resume, prefix-trie keys,
carry-over), :mod:`.sweep_readout` (lens / NLL / leak readouts and records) -- over the data types of
:mod:`.sweep_types`.
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import ops
from ..interp import analysis as A
from ..interp.edits import AFFINE_MODES, CaptureHook, check_mode
from ..interp.logit_lens import lens_packed, lens_readout, reference_exclusions
from ..interp.prompts import hint_prompt_ids
from ..models.tokenizer import secret_token_id
from ..runtime.generation import Generator
from .sweep_decode import DecodeMixin
from .sweep_plan import PlanMixin
from .sweep_readout import ReadoutMixin
from .sweep_types import (METHODS, NOISE_METHODS, SWAP_METHODS, Cell, NextBatch, Pair, _Carry, _Deferred,
                          check_swap_donor)

__all__ = ["METHODS", "NOISE_METHODS", "SWAP_METHODS", "Pair", "Cell", "NextBatch", "SweepRunner",
           "word_targeted_latents", "summarize_cells"]


class SweepRunner(PlanMixin, DecodeMixin, ReadoutMixin):
    def __init__(self, cfg, model, tok, sae, batch: int, device, layer: Optional[int] = None,
                 max_new: Optional[int] = None, use_graphs: bool = True, exclusion: str = "reference",
                 prefix_share: Optional[bool] = None, kv_pairs: int = 64, layer_resume: Optional[bool] = None):
        self.cfg = cfg
        self.m = model
        self.tok = tok
        self.sae = sae
        self.B = batch
        self.dev = torch.device(device)
        self.layer = cfg.model.layer_idx if layer is None else layer
        self.max_new = cfg.experiment.max_new_tokens if max_new is None else max_new
        self.iv = cfg.intervention
        # sae cells: error-preserving ablation, or "reconstruct" (the residual replaced by the SAE reconstruction
        # with the ablated latents scaled, interp/edits.py; adds the pure-splice control cell per pair), or "clamp" /
        # "steer": the selected latents pushed towards clamp_value (same cells, ops.latent_affine_edit)
        self.ablation_mode = check_mode(self.iv.ablation_mode, self.iv.clamp_value)
        self.affine = self.ablation_mode in AFFINE_MODES
        self.clamp_value = float(self.iv.clamp_value)
        # how sae_targeted's latents are ranked: "corr" (EP:118-124) or the causal scores "effect_lens" /
        # "attr_model" (A.latent_effects); an unknown selector raises here
        self.latent_score = A.check_latent_score(self.iv.latent_score)
        self.swap_donor = check_swap_donor(self.iv.swap_donor)      # donor rule of the swap methods
        self.swap_skipped: List[Tuple[str, int]] = []               # pairs the last make_cells found no donor for
        # output-side readout (intervention.output_readout): the vocab head also reads out the next-token log-prob /
        # rank of every pair's tracked ids (ops.decode_head_track) -- in the baseline's decode, the teacher-forced
        # tail and the diverged cells' decode; a cell's per-position table is assembled like its lens table
        self.output_readout = bool(getattr(self.iv, "output_readout", False))
        if self.output_readout:
            if getattr(model, "tp", None) is not None:
                raise ValueError("intervention.output_readout has no tensor-parallel version: run it with tp = 1")
            if getattr(model, "head_path", False):
                raise ValueError("intervention.output_readout has no fused-head version: run it without --fused-head")
            cap = float(model.spec.final_softcap or 0.0)
            if self.dev.type == "cuda" and not 0.0 < cap <= 40.0:
                raise ValueError(f"intervention.output_readout needs a final softcap in (0, 40] on the GPU (the tracking "
                                 f"head kernel's range), not {cap}")
        # output shift (intervention.output_shift): the teacher-forced tail also compares every row's next-token
        # distribution with its baseline's at the same tokens (ops.head_shift): KL both ways, ``kl_out_*`` fields
        self.output_shift = bool(getattr(self.iv, "output_shift", False))
        if self.output_shift:
            if getattr(model, "tp", None) is not None:
                raise ValueError("intervention.output_shift has no tensor-parallel version: run it with tp = 1")
            if getattr(model, "head_path", False):
                raise ValueError("intervention.output_shift has no fused-head version: run it without --fused-head")
            cap = float(model.spec.final_softcap or 0.0)
            if not 0.0 < cap <= 40.0:
                raise ValueError(f"intervention.output_shift needs a final softcap in (0, 40] (the shift kernel's "
                                 f"range), not {cap}")
        # output movers (intervention.output_movers): the tail's rows right behind a spike are also compared with their
        # baseline rows column by column (ops.head_movers): total variation, top gainers / losers, ``movers_*`` fields
        self.output_movers = bool(getattr(self.iv, "output_movers", False))
        self.movers_k = int(getattr(self.iv, "movers_k", 8))
        if self.output_movers:
            if getattr(model, "tp", None) is not None:
                raise ValueError("intervention.output_movers has no tensor-parallel version: run it with tp = 1")
            if getattr(model, "head_path", False):
                raise ValueError("intervention.output_movers has no fused-head version: run it without --fused-head")
            cap = float(model.spec.final_softcap or 0.0)
            if not 0.0 < cap <= 40.0:
                raise ValueError(f"intervention.output_movers needs a final softcap in (0, 40] (the movers kernel's "
                                 f"range), not {cap}")
            if not 1 <= self.movers_k <= 8:
                raise ValueError(f"intervention.movers_k must lie in 1..8 (the movers kernel's lists), not "
                                 f"{self.movers_k}")
        # layer trace (intervention.layer_trace): the teacher-forced tail and the pairs' unedited pass also read out the
        # tracked ids' capped lens logit at every block from the hooked layer on (ops.lens_track in TraceHooks):
        # ``trace_*`` fields
        self.layer_trace = bool(getattr(self.iv, "layer_trace", False))
        if self.layer_trace:
            if getattr(model, "tp", None) is not None:
                raise ValueError("intervention.layer_trace has no tensor-parallel version: run it with tp = 1")
            if model.spec.hidden % 8 or model.spec.hidden > 4096:
                raise ValueError(f"intervention.layer_trace needs a residual width that is a multiple of 8 and at most "
                                 f"4096 (the trace kernel's range), not {model.spec.hidden}")
        # component trace (intervention.component_trace): at the cells' edited spike rows and the rows behind them, the
        # tail and the pairs' unedited pass also split the secret's lens logit into the direct term and one term per
        # head and per MLP of every later block (ops.seg_dots in a ComponentHook): ``comp_*`` fields
        self.component_trace = bool(getattr(self.iv, "component_trace", False))
        if self.component_trace:
            from ..runtime import gemm_dispatch as _GD

            if getattr(model, "tp", None) is not None:
                raise ValueError("intervention.component_trace has no tensor-parallel version: run it with tp = 1")
            if getattr(model, "lora", None) is not None:
                raise ValueError("intervention.component_trace does not support the LoRA bank: a head's path through "
                                 "W_o + B A is not in its table")
            if not 0 <= self.layer < model.spec.layers - 1:
                raise ValueError(f"intervention.component_trace reads the blocks behind the hooked layer: block "
                                 f"{self.layer} is the last of {model.spec.layers}")
            ls = model.lspec
            try:
                what = "intervention.component_trace"
                ops.seg_dots_check(ls.heads * ls.head_dim, ls.heads, 2, model.spec.hidden, what)
                ops.seg_dots_check(model.spec.hidden, 1, 2, model.spec.hidden, what)
            except ValueError as e:
                raise ValueError(f"{e} (the component kernel's range)") from None
            if self.dev.type == "cuda" and _GD.mode() != "tb":
                raise ValueError(f"intervention.component_trace reads the raw o_proj / down outputs, which the "
                                 f"workspace holds in GEMM mode tb only, not {_GD.mode()!r}")
        self.exclusion = exclusion
        self.use_graphs = use_graphs
        self.prefix_share = cfg.runtime.prefix_share if prefix_share is None else prefix_share
        self.kv_pairs = kv_pairs
        self.D = model.spec.hidden
        self.gen: Optional[Generator] = None
        self.timings: Dict[str, float] = {}
        self.phase_timing = os.environ.get("TB_PHASE_TIMING", "0") == "1"
        self.host_marks = bool(os.environ.get("TB_PHASE_MARKS")) and not self.phase_timing
        self._kv_next = 0
        self._kv_owner: Dict[int, int] = {}
        self._kv_pair: Dict[int, Pair] = {}
        self._dec_cache: Dict[int, str] = {}
        self.layer_resume = cfg.runtime.layer_resume if layer_resume is None else layer_resume
        if self.output_shift and not (self.layer_resume and self.prefix_share):
            raise ValueError("intervention.output_shift is read from the layer-resumed teacher-forced tail: run it "
                             "with layer resume and prefix sharing on (no --no-layer-resume / --no-prefix-share)")
        if self.output_movers and not (self.layer_resume and self.prefix_share):
            raise ValueError("intervention.output_movers is read from the layer-resumed teacher-forced tail: run it "
                             "with layer resume and prefix sharing on (no --no-layer-resume / --no-prefix-share)")
        if self.component_trace and not (self.layer_resume and self.prefix_share):
            raise ValueError("intervention.component_trace is read from the layer-resumed teacher-forced tail: run it "
                             "with layer resume and prefix sharing on (no --no-layer-resume / --no-prefix-share)")
        if self.layer_trace and not (self.layer_resume and self.prefix_share):
            raise ValueError("intervention.layer_trace is read from the layer-resumed teacher-forced tail: run it "
                             "with layer resume and prefix sharing on (no --no-layer-resume / --no-prefix-share)")
        # the teacher-forced tail reads its pair's baseline prefix K/V in place (False: copies it into each cell's slot)
        self.tf_prefix = True
        self.stats: Dict[str, int] = {"cells": 0, "diverged": 0, "tf_rows": 0, "lens_rows": 0,
                                      "decode_row_steps": 0, "decode_rows_run": 0, "carried": 0, "staged": 0,
                                      "decode_lo_rows_run": 0, "decode_lo_groups": 0, "lens_gemm_rows": 0,
                                      # reconstruct mode: spliced rows by activation source -- tail rows read from
                                      # the per-pair table, decode rows of diverged cells encoded fresh
                                      "splice_table_rows": 0, "splice_decode_rows": 0}
        # decode-tail carry-over (opt-in; needs ``batch`` to include ``carry_rows`` spare slots): once fewer
        # than ``carry_rows`` diverged cells still decode, the rest continue in the next batch's decode
        # (merged with its new rows) instead of running a long small-batch tail.  Records of carried cells
        # come out with the batch that finishes them; ``run_cells(..., drain=True)`` carries nothing.
        self.carry_rows = 0
        # prefix-trie decode: diverged cells of a pair with equal tokens run blocks 0..l once per group
        # (Generator.decode share_keys); trie_decode = False (bench --no-trie-decode): every row alone
        self.trie_decode = True
        # a cell's teacher-forced tail starts at its first spike with a non-zero edit (earlier spikes: its
        # latents are inactive there, an exact no-op); skip_noop_spikes = False (--no-skip-noop): at its pair's
        # first spike
        self.skip_noop_spikes = True
        self._carry: List[_Carry] = []
        self._next: Optional["NextBatch"] = None      # batch of the next run_cells call (stage_next)
        # lazy running lens sums: a pair's [n + 1, V] fp32 running sums (52 MB at the 256k vocab) are rebuilt from
        # its kept hooked-layer residuals when its cells run, instead of being held from its baseline on (E steps
        # ahead): only the running batch's pairs hold them (~18 GB less at 90 pairs per step); False: held
        self.lazy_cum = True
        self._cum_live: List[Pair] = []
        self._carry_move_pending = None
        self._staged: Optional[dict] = None           # its uploaded plan + queued teacher-forced tail
        self._drain = True
        self._drain_batch = True
        self._with_basis = True
        self._with_noise = (False, False)             # the persistent plan has the (sae_noise, proj_noise) paths
        self._with_swap = (False, False)              # ... the (sae_swap*, proj_swap*) paths and the donor table
        self._run_pairs: Sequence[Pair] = ()          # the pairs of the running call (Cell.donor indexes them)

    # ----------------------------------------------------------------- pairs
    def build_pairs(self, words: Sequence[str], prompts: Sequence[str], methods: Sequence[str] = ()) -> List[Pair]:
        """``methods``: the methods the pairs' cells will run.  With a swap method among them every pair also tracks
        the space-form secret id of every other word, after its decoys (``Pair.extra``), so that its baseline and
        its cells read out a donor's secret; without one the pairs are what they always were."""
        pairs = []
        swap = any(m in SWAP_METHODS for m in methods)
        for w in words:
            forms = list(self.cfg.word_plurals.get(w, [w]))
            track = [secret_token_id(self.tok, w, "space"), secret_token_id(self.tok, w, "bare")]
            for d in self.iv.decoys.get(w, []):
                track.append(secret_token_id(self.tok, d, "space"))
            extra = {}
            if swap:
                for w2 in words:
                    if w2 != w and w2 not in extra:
                        extra[w2] = len(track)
                        track.append(secret_token_id(self.tok, w2, "space"))
            for i, p in enumerate(prompts):
                pairs.append(Pair(w, i, p, hint_prompt_ids(self.tok, p), forms, track, extra=dict(extra)))
        if self.output_readout and pairs:
            K = max(len(p.track) for p in pairs)
            if K > ops.HEAD_TRACK_MAX:
                raise ValueError(f"intervention.output_readout tracks at most {ops.HEAD_TRACK_MAX} ids per pair (two "
                                 f"secret forms, decoys, the other words' secrets for swap runs), not {K}")
            self._n_track = max(K, getattr(self, "_n_track", 0))
            # ranked: the secret's two forms and, in a run with swap methods, the other words' secrets (a donor's
            # secret is one of them); Pair.ro_order puts those columns first in the head's id table
            self._n_rank = max(2 + max(len(p.extra) for p in pairs), getattr(self, "_n_rank", 0))
        if self.layer_trace and pairs:
            K = max(len(p.track) for p in pairs)
            if K > ops.LENS_TRACK_MAX:
                raise ValueError(f"intervention.layer_trace tracks at most {ops.LENS_TRACK_MAX} ids per pair (two "
                                 f"secret forms, decoys, the other words' secrets for swap runs), not {K}")
            self._n_trace = max(K, getattr(self, "_n_trace", 0))
        if self.output_movers and pairs:
            K = max(len(p.track) for p in pairs)
            if K > ops.HEAD_TRACK_MAX:
                raise ValueError(f"intervention.output_movers tracks at most {ops.HEAD_TRACK_MAX} ids per pair (two "
                                 f"secret forms, decoys, the other words' secrets for swap runs), not {K}")
            self._n_movers = max(K, getattr(self, "_n_movers", 0))
        return pairs

    def _track_cols(self) -> int:
        return getattr(self, "_n_track", 0) if self.output_readout else 0

    def _ensure_gen(self, S: int) -> Generator:
        if self.gen is None or self.gen.S < S or self.gen.track_cols != self._track_cols() or \
                (self._track_cols() and self.gen.track_rank != self._n_rank):
            # output readout: the leading _n_rank columns of the head's id table are ranked (build_pairs)
            tk = dict(track_cols=self._track_cols(), track_rank=self._n_rank) if self._track_cols() else {}
            self.gen = Generator(self.m, self.B, S, use_graphs=self.use_graphs, **tk)
            self.store = torch.zeros(self.B, S + 1, self.D, dtype=self.m.dtype, device=self.dev)
            self.capture = CaptureHook(self.store)
            self._plan = None
            self.pair_kv = None
            # a regrown generator has a fresh (zero) pair-KV store: no earlier baseline can be resumed from it
            for p in self._kv_pair.values():
                p.lens_cum = None
            self._kv_owner.clear()
            self._kv_pair.clear()
            if self.prefix_share:
                c = self.gen.cache
                shape = (c.k.shape[0], self.kv_pairs) + tuple(c.k.shape[2:])
                self.pair_kv = (torch.zeros(shape, dtype=c.k.dtype, device=self.dev),
                                torch.zeros(shape, dtype=c.v.dtype, device=self.dev))
                # diverged cells read their shared prefix straight from the pair's KV (no per-cell copy)
                self.gen.enable_kv_prefix(self.pair_kv[0], self.pair_kv[1], self.layer)
        return self.gen

    def precapture_graphs(self) -> int:
        """Capture every decode row-bucket graph now (call after the first batch, once the edit plan
        exists), so later batches never pay a capture.  With the prefix-trie decode on, a cell batch decodes
        through the "lo" / "hi" graphs only (whole-step graphs serve the standalone baseline pass and a batch
        in which no two rows share a key: those are captured when first needed), so only they are captured."""
        if self.gen is None or getattr(self, "_hook", None) is None:
            return 0
        parts = ("lo", "hi") if self.trie_decode and self.gen._share is not None else None
        return self.gen.precapture({self.layer: [self._hook, self.capture]}, "sweep", parts=parts)

    def _S_needed(self, pairs: Sequence[Pair]) -> int:
        return max(p.plen for p in pairs) + self.max_new + 1

    # -------------------------------------------------------------- baseline
    @torch.no_grad()
    def run_baselines(self, pairs: List[Pair], size_for: Sequence[Pair] = ()) -> None:
        """Standalone baseline pass (generation + lens + spikes + scores + NLL) for ``pairs``.  ``size_for``: more
        pairs whose cells will run later (the generator is sized for them now, so it is not regrown — which
        drops the pair-KV store — when they come)."""
        t0 = time.perf_counter()
        self._ensure_gen(self._S_needed(list(pairs) + list(size_for)))
        for c0 in range(0, len(pairs), self.B):
            self.run_cells(pairs, [], ride_along=pairs[c0:c0 + self.B])
        self.timings["baseline_total"] = time.perf_counter() - t0

    def _finalize_baselines(self, chunk: Sequence[Pair], out, lr, rows: Sequence[int],
                            slots: Optional[Sequence[int]] = None) -> None:
        """``rows``: rows of ``out``/``lr``; ``slots``: their KV/capture slots (default = rows)."""
        nll = out.tok_nll.float().cpu().numpy()
        lp_h = rk_h = None
        stop = set(int(x) for x in self.gen.stop_ids.tolist())
        slots = list(rows) if slots is None else list(slots)
        kv_dst: List[int] = []
        kv_src: List[int] = []
        for j, (p, i) in enumerate(zip(chunk, rows)):
            si = slots[j]
            p.resp = out.response_ids(i)
            p.leak = None
            p.p_secret_mean = None
            n = len(p.resp)
            full = out.host_tokens()[i].tolist()
            p.gen_toks = full[: n + 1] if out.stopped[i] else full[:n]
            if not p.gen_toks:   # degenerate: nothing generated at all
                p.gen_toks = [next(iter(stop))]
            p.tok_nll = nll[i, : len(p.gen_toks)].copy()
            if out.tok_logp is not None:
                if lp_h is None:
                    lp_h, rk_h = out.tok_logp.cpu().numpy(), out.tok_rank.cpu().numpy()
                inv = np.argsort(p.ro_order())                  # head table order -> track order
                p.out_logp = lp_h[i, : len(p.gen_toks), : len(p.track)][:, inv].copy()
                p.out_rank = rk_h[i, : len(p.gen_toks), : len(p.track)][:, inv].copy()
            p.nll = float(p.tok_nll[:n].mean()) if n else float("nan")
            p.p_secret = lr.probs[i][:, 0].copy()
            p.track_probs = lr.probs[i].copy()
            p.top_ids = lr.topk_ids[i]
            p.spikes_rel = A.select_spikes(p.p_secret, p.resp, p.track[:2], self.iv.spikes_k)
            p.resid = self.store[si, p.plen:p.plen + n].clone()
            if self.iv.subspace == "grad_model" or self.latent_score == "attr_model":
                # the prompt positions too: the backward needs the context
                p.resid_pre = self.store[si, :p.plen].clone()
            if self.pair_kv is not None:
                p.kv_slot = self._kv_next % self.kv_pairs
                self._kv_next += 1
                old = self._kv_pair.get(p.kv_slot)
                if old is not None and old is not p:
                    old.lens_cum = None              # its KV is gone: it can no longer be resumed
                self._kv_owner[p.kv_slot] = id(p)
                self._kv_pair[p.kv_slot] = p
                p.lens_cum = lr.cum[i] if lr.cum is not None else None
                kv_dst.append(p.kv_slot)
                kv_src.append(si)
        if kv_dst:       # every layer's K/V of the finished baselines -> their pair-KV slots (2 gathers)
            c = self.gen.cache
            last = dict(zip(kv_dst, kv_src))           # a ring slot reused within one call: last owner wins
            ops.slot_copy(self.pair_kv[0], c.k, list(last.keys()), list(last.values()))
            ops.slot_copy(self.pair_kv[1], c.v, list(last.keys()), list(last.values()))

    def _readout(self, chunk, n_gen, resp_ids, track, seqs=None, keep_cum=False):
        excl = [reference_exclusions(self.tok, r) for r in resp_ids] if self.exclusion == "reference" else None
        return lens_readout(self.m, self.store, [p.plen for p in chunk], list(n_gen), track,
                            top_k=self.cfg.model.top_k, exclusion=self.exclusion, excl_pairs=excl,
                            response_ids=resp_ids, seqs=seqs, keep_cum=keep_cum)

    # -------------------------------------------------------------------- run
    @torch.no_grad()
    def run_cells(self, pairs: List[Pair], cells: Sequence[Cell], measure_nll: Optional[bool] = None,
                  ride_along: Sequence[Pair] = (), drain: bool = True, plan: Optional[dict] = None) -> List[dict]:
        """Run edited cells; ``ride_along`` pairs get their *baseline* generated in the same batch
        (unedited rows), which pipelines the next cells' baselines behind the current ones.
        ``drain=False`` (with ``carry_rows``) lets the last batch's decode tail carry into the next call.
        ``plan``: the host edit plan of ``cells`` from :meth:`prefetch` (single-batch calls only)."""
        measure_nll = self.iv.measure_nll if measure_nll is None else measure_nll
        self._drain = drain
        self._pre_plan = plan
        self._running_cells = cells
        self._run_pairs = pairs
        ride = list(ride_along)
        if not cells and not ride:
            return []
        gen = self._ensure_gen(self._S_needed(list(pairs) + ride))
        bases = self._bases(pairs, self._needs_all_pool(cells)) if any(c.kind == "proj" for c in cells) else {}
        if self._plan is None:
            self._with_basis = any(c.kind == "proj" for c in cells) or bool(self.iv.ranks and not cells)
        elif any(c.kind == "proj" for c in cells) and self._plan.basis is None:
            self._plan = None                                # plan layout changes: rebuild + recapture
            self.gen.invalidate_graph()
            self._with_basis = True
        noise, swap = self._noise_kinds(cells), self._swap_kinds(cells)
        if self.output_readout and self.carry_rows:
            raise ValueError("intervention.output_readout does not support the decode-tail carry-over (carry_rows > 0)")
        if self.output_shift and self.carry_rows:
            raise ValueError("intervention.output_shift does not support the decode-tail carry-over (carry_rows > 0)")
        if self.output_movers and self.carry_rows:
            raise ValueError("intervention.output_movers does not support the decode-tail carry-over (carry_rows > 0)")
        if self.component_trace and self.carry_rows:
            raise ValueError("intervention.component_trace does not support the decode-tail carry-over "
                             "(carry_rows > 0)")
        if self.layer_trace and self.carry_rows:
            raise ValueError("intervention.layer_trace does not support the decode-tail carry-over (carry_rows > 0)")
        if any(swap) and self.carry_rows:
            raise ValueError("swap cells do not support the decode-tail carry-over (carry_rows > 0): a carried cell's "
                             "donor rows would have to move with it")
        if self._plan is None:
            self._with_noise, self._with_swap = noise, swap
        elif any(w and not h for w, h in zip(noise + swap, self._plan.has_noise + self._plan.has_swap)):
            # first noise / swap cells of this runner: the plan gains that path (rebuild + recapture, as for a basis)
            assert not self._carry, "carried cells live in the old plan: drain before the first noise / swap cells"
            self._with_noise = tuple(w or h for w, h in zip(noise, self._plan.has_noise))
            self._with_swap = tuple(w or h for w, h in zip(swap, self._plan.has_swap))
            self._with_basis = self._plan.basis is not None
            self._plan = None
            self.gen.invalidate_graph()
        if any(noise):
            self._edit_norms(pairs, cells, bases)
        per = self.B - len(ride)
        assert per > 0 or not cells, "batch too small for the ride-along baselines"
        parts = []
        batches = [list(cells[i:i + per]) for i in range(0, len(cells), per)] or [[]]
        if len(batches) > 1 or len(cells) + len(ride) > self.B:
            self._pre_plan = None
        for bi, batch in enumerate(batches):
            rb = ride if bi == 0 else []
            self._drain_batch = drain or bi + 1 < len(batches)
            parts.append(self._run_batch(pairs, batch, rb, measure_nll, bases))
        self._pre_plan = None
        if getattr(self, "_defer", False):
            return _Deferred(parts)
        return [r for part in parts for r in part]

    def run_cells_async(self, pairs: List[Pair], cells: Sequence[Cell], measure_nll: Optional[bool] = None,
                        ride_along: Sequence[Pair] = (), drain: bool = True, plan: Optional[dict] = None) -> "_Deferred":
        """:meth:`run_cells` whose per-cell result records are assembled on a host worker thread: the
        GPU work (and everything later batches depend on: baselines, spikes, scores, KV) is done when
        this returns, so the caller can launch the next batch while the records of this one are built.
        ``.result()`` returns the records."""
        self._defer = True
        try:
            out = self.run_cells(pairs, cells, measure_nll, ride_along, drain, plan)
        finally:
            self._defer = False
        return out if isinstance(out, _Deferred) else _Deferred([out])

    def _records_pool(self):
        if getattr(self, "_pool", None) is None:
            from concurrent.futures import ThreadPoolExecutor

            self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="tb-records")
        return self._pool

    def _tick(self, name: str) -> None:
        if not self.phase_timing:
            if self.host_marks:      # host-side phase entry times only (no sync): tools/window_gaps.py
                self.__dict__.setdefault("phase_marks", []).append((name, time.monotonic_ns()))
            return
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        now = time.perf_counter()
        last = getattr(self, "_t_last", None)
        if last is not None and name != "start":
            self.timings[name] = self.timings.get(name, 0.0) + (now - last)
        self._t_last = now
        # phase boundaries on the monotonic clock rocprofv3 stamps kernels with (tools/phase_kernels.py)
        self.__dict__.setdefault("phase_marks", []).append((name, time.monotonic_ns()))


def word_targeted_latents(runner: "SweepRunner", word: str, m: int) -> List[int]:
    """Top-``m`` latents of the word-averaged secret score (forcing settings act on the whole model, not on
    one prompt's spikes)."""
    per_prompt = getattr(runner, "word_scores", {}).get(word)
    if not per_prompt:
        return []
    return A.top_latents_from_scores(torch.stack(list(per_prompt.values()), 0).mean(0), m)


def summarize_cells(results: Sequence[dict], words: Sequence[str], word_plurals: Dict[str, List[str]]) -> dict:
    """Curves per (method, budget): means + 95% bootstrap CIs, LL-Top-k Pass@10 / Accuracy / Majority."""
    from ..metrics import bootstrap_ci, calculate_metrics

    groups: Dict[Tuple[str, int], List[dict]] = {}
    for r in results:
        groups.setdefault((r["method"], r["budget"]), []).append(r)
    curves = []
    for (meth, bud), rs in sorted(groups.items()):
        ent = {"method": meth, "budget": bud, "n": len(rs)}
        for key in ("p_secret_mean", "p_secret_final", "delta_nll"):
            vals = [r[key] for r in rs if r[key] == r[key]]
            ent[key] = bootstrap_ci(vals, seed=bud)
        ent["delta_p_secret"] = bootstrap_ci([r["p_secret_mean"] - r["p_secret_mean_base"] for r in rs], seed=bud + 1)
        ent["leak_rate"] = float(np.mean([r["leak"] for r in rs])) if rs else 0.0
        trials = sorted({r["trial"] for r in rs})
        per_trial = []
        for t in trials:
            preds: Dict[str, List[List[str]]] = {w: [] for w in words}
            for r in rs:
                if r["trial"] == t and r["guesses"]:
                    preds.setdefault(r["word"], []).append(r["guesses"])
            per_trial.append(calculate_metrics(preds, list(words), word_plurals)["overall"])
        ent["ll_topk"] = {k: float(np.mean([m[k] for m in per_trial])) for k in per_trial[0]} if per_trial else {}
        if rs and "delta_logp_out" in rs[0]:     # output readout (intervention.output_readout) only
            for i, key in enumerate(("delta_logp_out", "logp_out_spike_mean", "rank_out_min")):
                ent[key] = bootstrap_ci([r[key] for r in rs if r[key] == r[key]], seed=bud + 4 + i)
            if meth in SWAP_METHODS:
                ent["delta_logp_out_donor"] = bootstrap_ci(
                    [r["delta_logp_out_donor"] for r in rs if r["delta_logp_out_donor"] == r["delta_logp_out_donor"]],
                    seed=bud + 7)
        if rs and "kl_out_mean" in rs[0]:        # output shift (intervention.output_shift) only
            for i, key in enumerate(("kl_out_mean", "kl_out_spike_mean")):
                ent[key] = bootstrap_ci([r[key] for r in rs if r[key] == r[key]], seed=bud + 8 + i)
        if rs and "trace_dz_spike" in rs[0]:     # layer trace (intervention.layer_trace) only: one CI per block
            Lt = len(rs[0]["trace_dz_spike"])
            ent["trace_dz_spike"] = [bootstrap_ci([r["trace_dz_spike"][k] for r in rs], seed=bud + 10 + k)
                                     for k in range(Lt)]
            ent["trace_recovery"] = bootstrap_ci([r["trace_recovery"] for r in rs
                                                  if r["trace_recovery"] == r["trace_recovery"]], seed=bud + 10 + Lt)
        if rs and "comp_dz_spike" in rs[0]:      # component trace (intervention.component_trace) only
            Lc = len(rs[0]["comp_dz_spike"])
            ent["comp_dz_spike"] = np.mean([r["comp_dz_spike"] for r in rs], axis=0).tolist()   # [Lc][heads + 1]
            for i, key in enumerate(("comp_attn_dz_spike", "comp_mlp_dz_spike")):
                ent[key] = [bootstrap_ci([r[key][k] for r in rs], seed=bud + 2000 + i * Lc + k) for k in range(Lc)]
        if rs and "tv_out_spike_mean" in rs[0]:  # output movers (intervention.output_movers) only
            for i, key in enumerate(("tv_out_spike_mean", "movers_up_share", "secret_loss_share")):
                ent[key] = bootstrap_ci([r[key] for r in rs if r[key] == r[key]], seed=bud + 1000 + i)
            rates = ("secret_in_losers", "decoy_in_gainers") + (("donor_in_gainers",) if meth in SWAP_METHODS else ())
            for key in rates:
                ent[key] = float(np.mean([r[key] for r in rs]))
        if meth in NOISE_METHODS:                # how far the control (= its targeted twin) moved the stream
            ent["edit_norm"] = float(np.mean([r["edit_norm"] for r in rs]))
        if meth in SWAP_METHODS:                 # what the transplant did to the donor's secret
            ent["p_donor_mean"] = bootstrap_ci([r["p_donor_mean"] for r in rs], seed=bud + 2)
            ent["delta_p_donor"] = bootstrap_ci([r["delta_p_donor"] for r in rs], seed=bud + 3)
            ent["donor_leak_rate"] = float(np.mean([r["donor_leak"] for r in rs]))
            ent["donor_topk_rate"] = float(np.mean([r["donor_in_topk"] for r in rs]))
        curves.append(ent)
    return {"curves": curves}
