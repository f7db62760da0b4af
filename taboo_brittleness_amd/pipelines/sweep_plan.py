"""Sweep planning (part of :class:`~.sweep.SweepRunner`): pair scoring (latent secret scores, spike selection,
SAE activity), the cells of a pair (methods x budgets x trials), the edit bases (SAE decoder rows, PCA /
gradient subspaces, random controls) and the per-batch edit plan, its host -> device staging and the
next-batch prefetch (plans built on the host while the GPU runs the current batch).
"""
from __future__ import annotations

import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import ops
from ..interp import analysis as A
from ..interp.edits import EditHook, EditPlan
from .sweep_types import METHODS, NOISE_METHODS, SPLICE_METHOD, SWAP_METHODS, Cell, NextBatch, Pair, _h2d


class PlanMixin:
    """Methods of :class:`~.sweep.SweepRunner` (state lives on the runner; see its docstring)."""

    @torch.no_grad()
    def _score_pairs(self, pairs: List[Pair]) -> None:
        """Latent secret scores per prompt (EP:118-124) → targeted latent lists; activation-matched random pools."""
        if self.sae is None:
            return
        mmax = max(self.iv.budgets) if self.iv.budgets else 1
        rows, seg, p_all, sp = [], [0], [], []
        live = [p for p in pairs if len(p.resp) > 0]
        for p in live:
            rows.append(p.resid)
            p_all.append(torch.from_numpy(np.asarray(p.p_secret, dtype=np.float32)))
            seg.append(seg[-1] + len(p.resp))
            sp.append(p.spikes_rel)
        if not live:
            return
        R = torch.cat(rows, 0)
        sel, acts = self.latent_score, None
        if sel == "corr":
            scores = A.latent_scores(self.sae, R, torch.cat(p_all), sp, seg)       # [G, L]
        else:
            # causal ranking: one encode serves the scores, the correlational comparison and the activity below
            acts = self.sae.encode(R)
            scores = self._causal_scores(live, R, acts, seg, torch.cat(p_all), sel, mmax)
        # word -> {prompt index: latest scores}: a re-scored pair (e.g. after SAE calibration, or a later
        # re-baseline) overwrites its entry, so the word mean is over distinct prompts, never stale ones
        ws = self.__dict__.setdefault("word_scores", {})
        for g, p in enumerate(live):
            ws.setdefault(p.word, {})[p.pidx] = scores[g].clone()
        if self.iv.score_over == "word":
            by_word: Dict[str, List[int]] = {}
            for g, p in enumerate(live):
                by_word.setdefault(p.word, []).append(g)
            for w, gs in by_word.items():
                s = scores[gs].mean(0)
                tl = A.top_latents_from_scores(s, mmax)
                for g in gs:
                    live[g].targeted = tl
        else:
            for p, tl in zip(live, A.top_latents_batch(scores, mmax)):
                p.targeted = tl
        if sel != "corr":
            # the values the ranking used (the word mean under score_over = word), in the order of ``targeted``
            used = scores
            if self.iv.score_over == "word":
                used = torch.stack([scores[[h for h, q in enumerate(live) if q.word == p.word]].mean(0) for p in live])
            vals = used.gather(1, torch.tensor([p.targeted for p in live], dtype=torch.long, device=used.device)).cpu()
            for p, v in zip(live, vals.tolist()):
                p.targeted_scores = v
        if acts is None:
            acts = self.sae.encode(R)
        sp_rows = torch.tensor([seg[g] + i for g, p in enumerate(live) for i in p.spikes_rel], device=acts.device)
        sp_grp = torch.tensor([g for g, p in enumerate(live) for _ in p.spikes_rel], device=acts.device)
        active = torch.zeros(len(live), acts.shape[1], dtype=torch.float32, device=acts.device)
        if sp_rows.numel():
            active.index_add_(0, sp_grp, (acts.index_select(0, sp_rows) > 0).float())
        g_idx, l_idx = torch.nonzero(active > 0, as_tuple=True)
        g_h, l_h = g_idx.cpu().numpy(), l_idx.cpu().numpy()
        bounds = np.searchsorted(g_h, np.arange(len(live) + 1))
        for g, p in enumerate(live):
            p.active_pool = l_h[bounds[g]:bounds[g + 1]].astype(np.int64)
        if self.ablation_mode == "reconstruct":
            # the rows the teacher-forced tail splices are these very residuals at the spikes: keep their
            # activations per pair (K rows), so the tail never encodes (no row is a no-op in this mode, so the
            # activity table of the no-op spike skip is not needed either)
            key, K, n0 = self._sae_key(), self.iv.spikes_k, 0
            for g, p in enumerate(live):
                k = len(p.spikes_rel[:K])
                p.splice_acts = acts.index_select(0, sp_rows[n0:n0 + k]) if k else acts[:0]
                p.splice_key = key
                n0 += len(p.spikes_rel)
            return
        if self.affine:
            return                              # clamp / steer edit inactive latents too: no spike is skipped
        self._spike_activity(live)

    @torch.no_grad()
    def _causal_scores(self, live: Sequence[Pair], R: torch.Tensor, acts: torch.Tensor, seg: Sequence[int],
                       p_all: torch.Tensor, sel: str, mmax: int) -> torch.Tensor:
        """``intervention.latent_score = effect_lens | attr_model``: ``[G, L]`` scores of the pairs from their spike
        rows of ``acts`` (``A.latent_effects``; pairs that share a secret token share a launch).  Also ranks the
        same pairs by the correlational score once (``Pair.targeted_corr``, reported as ``corr_overlap``)."""
        dev = acts.device
        spike = torch.zeros(acts.shape[0], dtype=torch.uint8)
        for g, p in enumerate(live):
            for i in p.spikes_rel:
                spike[seg[g] + i] = 1
        corr, _, _ = ops.latent_score(acts.contiguous(), p_all.to(dev).float().contiguous(), spike.to(dev),
                                      torch.tensor(list(seg), dtype=torch.int32, device=dev))
        for p, tl in zip(live, A.top_latents_batch(corr, mmax)):
            p.targeted_corr = tl
        scores = torch.zeros(len(live), acts.shape[1], dtype=torch.float32, device=dev)
        groups: Dict[tuple, List[int]] = {}
        for g, p in enumerate(live):
            groups.setdefault(tuple(p.track[:1]), []).append(g)
        for ids, gs in groups.items():
            ridx = torch.tensor([seg[g] + i for g in gs for i in live[g].spikes_rel], dtype=torch.long, device=dev)
            sseg = np.cumsum([0] + [len(live[g].spikes_rel) for g in gs]).tolist()
            grads = torch.cat([self._score_grads(live[g]) for g in gs], 0) if sel == "attr_model" else None
            sc = A.latent_effects(self.sae, self.m, R.index_select(0, ridx.to(R.device)), acts.index_select(0, ridx),
                                  sseg, list(ids), self.iv.alpha, sel, grads)
            scores[torch.tensor(gs, dtype=torch.long, device=dev)] = sc
        return scores

    def _score_grads(self, p: Pair) -> torch.Tensor:
        """``attr_model``: the pair's spike rows of ``GR.model_gradients`` (``[len(spikes_rel), D]``), kept with the
        baseline they came from: a pair is back-propagated once per baseline, however often it is re-scored."""
        from ..interp import gradient as GR

        pre = getattr(p, "resid_pre", None)
        assert pre is not None, "latent_score = attr_model needs the baselines run with latent_score = attr_model"
        assert getattr(self.m, "tp", None) is None and getattr(self.m, "lora", None) is None, \
            "attr_model needs unsharded, merged weights"
        spikes = tuple(p.spikes_rel)
        c = p.score_grads
        if c is not None and c[0] is p.resid and c[1] == spikes:
            return c[2]
        g = GR.model_gradients(self.m, torch.cat([pre, p.resid], 0), self.layer, [p.plen + t for t in spikes],
                               p.track[:1])
        p.score_grads = (p.resid, spikes, g)
        return g

    @torch.no_grad()
    def _splice_table(self, upairs: Sequence[Pair]):
        """Reconstruct mode: the per-step activation table of the teacher-forced tail -- each pair's activations at
        its spikes (``Pair.splice_acts``, re-encoded here if the SAE changed since they were taken), concatenated;
        returns ``(table [R, d_sae], first row per pair)``."""
        key, K = self._sae_key(), self.iv.spikes_k
        offs, parts, n = [], [], 0
        for p in upairs:
            k = len(p.spikes_rel[:K])
            if p.splice_key != key or p.splice_acts is None or p.splice_acts.shape[0] != k:
                rows = torch.tensor([min(max(t, 0), p.resid.shape[0] - 1) for t in p.spikes_rel[:K]],
                                    dtype=torch.long, device=self.dev)
                p.splice_acts = self.sae.encode(p.resid.index_select(0, rows)) if k else \
                    torch.zeros(0, self.sae.d_sae, dtype=torch.float32, device=self.dev)
                p.splice_key = key
            offs.append(n)
            parts.append(p.splice_acts)
            n += k
        tab = torch.cat(parts, 0) if len(parts) > 1 else parts[0]
        if tab.shape[0] == 0:
            tab = torch.zeros(1, self.sae.d_sae, dtype=torch.float32, device=self.dev)
        return tab.contiguous(), offs

    @torch.no_grad()
    def _spike_activity(self, live: Sequence[Pair]) -> None:
        """Where each candidate latent's ablation is a non-zero edit: the latents active at the spikes plus the
        targeted ones, evaluated by the edit kernel itself (``ops.lowrank_edit`` coefficients on copies of the
        baseline's hooked-layer residuals at the spikes — the exact rows and arithmetic the teacher-forced tail
        edits, since blocks ``0..l`` are the baseline's there).  A cell whose latents are all inactive at its
        pair's first spikes leaves those positions bit-identical to the baseline (all-zero edits are no-ops), so
        its tail starts at its first *effective* spike (``_plan_for`` -> ``plan["f"]``)."""
        s, K = self.sae, self.iv.spikes_k
        rows, owner = [], []
        key = self._sae_key()
        for g, p in enumerate(live):
            cand = np.union1d(p.active_pool, np.asarray(p.targeted, np.int64)).astype(np.int64)
            p.act_ids, p.act_mask, p.act_key = cand, np.zeros(cand.size, np.int64), key
            if s is None or p.resid is None or not cand.size:
                continue
            for k, t in enumerate(p.spikes_rel[:K]):
                if 0 <= t < p.resid.shape[0]:
                    for c0 in range(0, cand.size, 256):
                        rows.append((g, t))
                        owner.append((g, k, c0, min(256, cand.size - c0)))
        if not rows or self.iv.alpha == 0:
            return
        n = len(rows)
        idx = np.zeros((n, 256), np.int32)
        cnt = np.zeros(n, np.int32)
        for i, (g, k, c0, m) in enumerate(owner):
            idx[i, :m] = live[g].act_ids[c0:c0 + m]
            cnt[i] = m
        dev = self.dev
        h = torch.stack([live[g].resid[t] for g, t in rows]).contiguous()
        coef = torch.zeros(n, 256, dtype=torch.float32, device=dev)
        ops.lowrank_edit(h, torch.ones(n, dtype=torch.uint8, device=dev), torch.from_numpy(idx).to(dev),
                         torch.from_numpy(cnt).to(dev), s.W_encT, s.W_dec, s.b_enc, s.threshold,
                         s.b_dec if s.apply_b_dec_to_input else None, self.iv.alpha, None, 1e-6, None, coef)
        nz = (coef != 0).cpu().numpy()
        for i, (g, k, c0, m) in enumerate(owner):
            live[g].act_mask[c0:c0 + m] |= nz[i, :m].astype(np.int64) << k

    @staticmethod
    def _noise_kinds(cells: Sequence[Cell]) -> Tuple[bool, bool]:
        ms = {c.method for c in cells}
        return ("sae_noise" in ms, "proj_noise" in ms)

    @staticmethod
    def _swap_kinds(cells: Sequence[Cell]) -> Tuple[bool, bool]:
        ms = {c.method for c in cells}
        return (bool(ms & {"sae_swap", "sae_swap_random"}), bool(ms & {"proj_swap", "proj_swap_random"}))

    def _needs_all_pool(self, cells: Sequence[Cell]) -> bool:
        """``proj_swap`` reads the basis pooled over all pairs, whatever ``pca_pool`` says: between-word directions
        are what a swap must carry."""
        return self.iv.pca_pool == "word" and any(c.method == "proj_swap" for c in cells)

    @staticmethod
    def _donor_eligible(q: Pair) -> bool:
        return q.resid is not None and q.resid.shape[0] > 0 and bool(q.spikes_rel)

    def swap_donors(self, pairs: Sequence[Pair]) -> List[int]:
        """Per pair, the index of its donor among ``pairs`` (-1: none) under ``intervention.swap_donor``:
        ``next_word`` -- the pair of the next word in ``cfg.words`` order (cyclic, own word skipped) with the same
        prompt index; ``next_prompt`` -- the same word's next prompt index (cyclic).  A candidate without a baseline
        or without spikes is skipped and the next one is tried."""
        at: Dict[tuple, int] = {}
        for i, q in enumerate(pairs):
            at.setdefault((q.word, q.pidx, q.rep), i)
            at.setdefault((q.word, q.pidx), i)
        words = list(self.cfg.words) + sorted({q.word for q in pairs} - set(self.cfg.words))
        out = []
        for p in pairs:
            if self.swap_donor == "next_word":
                w0 = words.index(p.word)
                cand = [(words[(w0 + k) % len(words)], p.pidx) for k in range(1, len(words))]
            else:
                idxs = sorted({q.pidx for q in pairs if q.word == p.word})
                i0 = idxs.index(p.pidx)
                cand = [(p.word, idxs[(i0 + k) % len(idxs)]) for k in range(1, len(idxs))]
            d = -1
            for w, i in cand:
                j = at.get((w, i, p.rep), at.get((w, i), -1))
                if j >= 0 and pairs[j] is not p and self._donor_eligible(pairs[j]):
                    d = j
                    break
            out.append(d)
        return out

    @torch.no_grad()
    def _edit_norms(self, pairs: Sequence[Pair], cells: Sequence[Cell], bases: Dict[str, torch.Tensor]) -> None:
        """How far the norm-matched controls move the stream: per (pair, noise method, budget), the mean over the
        pair's spikes of ``|targeted delta|_2 / |h|_2``, measured by the control's own kernel
        (``ops.matched_noise_edit``'s ``norm_out``) on copies of the baseline's hooked-layer residuals at the spikes
        -- the rows the teacher-forced tail edits.  Kept on the pair (``Pair.edit_norm``) until it is re-baselined;
        result records of noise cells carry it as ``edit_norm``."""
        K, s, dev = self.iv.spikes_k, self.sae, self.dev
        rows: Dict[str, list] = {"sae_noise": [], "proj_noise": []}       # (pair, budget, latent ids | basis rows)
        for c in cells:
            if c.method not in NOISE_METHODS:
                continue
            p = pairs[c.pair]
            if p.edit_norm is None or p.edit_norm[0] is not p.resid:
                p.edit_norm = (p.resid, {})
            if (c.method, c.budget) in p.edit_norm[1]:
                continue
            p.edit_norm[1][(c.method, c.budget)] = 0.0
            if p.resid is None or not [t for t in p.spikes_rel[:K] if 0 <= t < p.resid.shape[0]]:
                continue
            if c.method == "sae_noise":
                rows[c.method].append((p, c.budget, list(p.targeted[: c.budget]), None))
            else:
                bk = p.word if self.iv.pca_pool == "word" else "__all__"
                rows[c.method].append((p, c.budget, None, bases[bk][: c.budget]))
        for meth, ent in rows.items():
            if not ent:
                continue
            hs, ix, own, tabs, off = [], [], [], [], 0
            for p, bud, lat, U in ent:
                if U is not None:                    # this entry's basis rows, appended to the call's table
                    lat = list(range(off, off + int(U.shape[0])))
                    tabs.append(U.float().to(dev))
                    off += int(U.shape[0])
                for t in p.spikes_rel[:K]:
                    if 0 <= t < p.resid.shape[0]:
                        hs.append(p.resid[t])
                        ix.append(lat)
                        own.append((p, bud))
            n, mmax = len(hs), max(1, max(len(l) for l in ix))
            idx = np.zeros((n, mmax), np.int32)
            for i, l in enumerate(ix):
                idx[i, :len(l)] = l
            h = torch.stack(hs).contiguous()
            hn = torch.linalg.vector_norm(h.float(), dim=1)
            # the norm does not depend on the draw: any stream will do
            seeds = torch.zeros(n, dtype=torch.int64, device=dev)
            pos = torch.zeros(n, dtype=torch.int32, device=dev)
            norm = torch.zeros(n, dtype=torch.float32, device=dev)
            ap = torch.ones(n, dtype=torch.uint8, device=dev)
            idx_d = torch.from_numpy(idx).to(dev)
            cnt_d = torch.tensor([len(l) for l in ix], dtype=torch.int32, device=dev)
            if meth == "sae_noise":
                # the coefficients of the sweep's own edit: clamp -> val = alpha c, steer -> val = c at alpha 0
                val, alpha = None, self.iv.alpha
                if self.affine:
                    alpha = self.iv.alpha if self.ablation_mode == "clamp" else 0.0
                    val = torch.full((n, mmax), self.clamp_value, dtype=torch.float32, device=dev)
                    val = val * alpha if self.ablation_mode == "clamp" else val
                ops.matched_noise_edit(h, ap, idx_d, cnt_d, s.W_encT, s.W_dec, seeds, pos, val,
                                       s.b_enc, s.threshold, s.b_dec if s.apply_b_dec_to_input else None, alpha,
                                       norm_out=norm)
            else:
                tab = torch.cat(tabs, 0).contiguous()
                ops.matched_noise_edit(h, ap, idx_d, cnt_d, tab, tab, seeds, pos, norm_out=norm)
            rel = (norm / hn.clamp_min(1e-30)).cpu().numpy()
            acc: Dict[tuple, list] = {}
            for i, (p, bud) in enumerate(own):
                acc.setdefault((id(p), bud), [p]).append(float(rel[i]))
            for (_, bud), v in acc.items():
                v[0].edit_norm[1][(meth, bud)] = float(np.mean(v[1:]))

    # ----------------------------------------------------------------- cells
    def make_cells(self, pairs: Sequence[Pair], methods: Sequence[str] = METHODS) -> List[Cell]:
        cells: List[Cell] = []
        base = self.cfg.experiment.seed
        if "sae_noise" in methods and self.ablation_mode == "reconstruct":
            raise ValueError("sae_noise has no meaning under ablation_mode = reconstruct: the splice replaces the "
                             "residual, so there is no added delta whose norm could be matched")
        swap = [m for m in methods if m in SWAP_METHODS]
        donors: List[int] = []
        if swap:
            if any(m.startswith("sae") for m in swap) and self.ablation_mode != "error_preserving":
                raise ValueError(f"sae_swap / sae_swap_random are defined for ablation_mode = error_preserving only, "
                                 f"not {self.ablation_mode!r}")
            if any(p.extra is None or not all(q.word == p.word or q.word in p.extra for q in pairs) for p in pairs):
                raise ValueError("swap methods need pairs that track the other words' secrets: "
                                 "build_pairs(words, prompts, methods)")
            donors = self.swap_donors(pairs)
            if getattr(self, "component_trace", False):     # the donor column of the pairs' component tables
                self._pair_donor = {id(p): pairs[d].word for p, d in zip(pairs, donors) if d >= 0}
            self.swap_skipped = [(p.word, p.pidx) for p, d in zip(pairs, donors) if d < 0]
        for pi, p in enumerate(pairs):
            for meth in methods:
                if meth == SPLICE_METHOD:
                    continue                         # added below, once per pair, in reconstruct mode only
                if meth in SWAP_METHODS and donors[pi] < 0:
                    continue                         # no eligible donor: no swap cells (swap_skipped)
                if meth.startswith("sae"):
                    if self.sae is None:
                        continue
                    budgets = self.iv.budgets
                    trials = 1 if meth in ("sae_targeted", "sae_swap") else self.iv.random_trials
                else:
                    budgets = self.iv.ranks
                    trials = 1 if meth in ("proj_targeted", "proj_swap") else self.iv.proj_random_trials
                if meth in NOISE_METHODS:
                    trials = self.iv.noise_trials
                for bud in budgets:
                    for t in range(trials):
                        # replicate 0 keeps the plain key, so sweeps seeded before replicates existed reproduce;
                        # a replicate > 0 (the bench's repeated pairs) draws its own random latent sets / subspaces
                        key = (base, p.word, p.pidx, meth, bud, t) + ((p.rep,) if p.rep else ())
                        cells.append(Cell(pi, meth, int(bud), t, A.cell_seed(*key),
                                          donors[pi] if meth in SWAP_METHODS else -1))
            if self.ablation_mode == "reconstruct" and self.sae is not None and \
                    any(meth.startswith("sae") for meth in methods):
                key = (base, p.word, p.pidx, SPLICE_METHOD, 0, 0) + ((p.rep,) if p.rep else ())
                cells.append(Cell(pi, SPLICE_METHOD, 0, 0, A.cell_seed(*key)))      # the pure-splice control
        return cells

    def _bases(self, pairs: Sequence[Pair], with_all: bool = False) -> Dict[str, torch.Tensor]:
        """Targeted secret subspaces pooled per word (or across all pairs): PCA of the spike residuals
        (EP:144-146) or, with ``intervention.subspace = grad_lens | grad_model``, the top singular directions of
        the secret-logit gradients at the spikes (EP:146's alternative; interp/gradient.py).  ``with_all``: under
        ``pca_pool = word`` also the ``__all__`` pool (``proj_swap``)."""
        from ..interp import gradient as GR

        rmax = max(self.iv.ranks) if self.iv.ranks else 1
        mode = self.iv.subspace
        if mode not in ("pca", "grad_lens", "grad_model"):
            raise ValueError(f"intervention.subspace must be pca, grad_lens or grad_model, not {mode!r}")
        # the bases depend only on the pairs' kept baseline residuals (identity-keyed: a re-run baseline makes a
        # new tensor) and the subspace settings; run_sweep passes every pair on every chunk and the staged plan
        # asks again, so the gradient forward/backward passes run once per pair set
        ckey = (mode, self.iv.pca_pool, bool(with_all), rmax,
                tuple((id(p), id(p.resid), tuple(p.spikes_rel or ())) for p in pairs))
        cache = getattr(self, "_bases_cache", None)
        if cache is not None and cache[0] == ckey:
            return cache[1]
        out = self._bases_compute(pairs, mode, rmax, with_all)
        self._bases_cache = (ckey, out, [p.resid for p in pairs])   # refs held: the ids cannot be reused
        return out

    def _bases_compute(self, pairs: Sequence[Pair], mode: str, rmax: int,
                       with_all: bool = False) -> Dict[str, torch.Tensor]:
        from ..interp import gradient as GR

        groups: Dict[str, List[torch.Tensor]] = {}
        for p in pairs:
            if p.resid is None or not p.spikes_rel:
                continue
            key = p.word if self.iv.pca_pool == "word" else "__all__"
            if mode == "pca":
                groups.setdefault(key, []).append(p.resid[p.spikes_rel].float())
            elif mode == "grad_lens":
                groups.setdefault(key, []).append(GR.lens_gradients(self.m, p.resid[p.spikes_rel], p.track[:1]))
            else:
                pre = getattr(p, "resid_pre", None)
                assert pre is not None, "grad_model subspaces need the baselines run with subspace=grad_model"
                assert getattr(self.m, "tp", None) is None and getattr(self.m, "lora", None) is None, \
                    "grad_model needs unsharded, merged weights"
                seq = torch.cat([pre, p.resid], 0)
                sp = [p.plen + t for t in p.spikes_rel]
                groups.setdefault(key, []).append(GR.model_gradients(self.m, seq, self.layer, sp, p.track[:1]))
            if with_all and key != "__all__":
                groups.setdefault("__all__", []).append(groups[key][-1])
        if mode == "pca":
            return {k: A.secret_subspace(torch.cat(v, 0), rmax) for k, v in groups.items()}
        return {k: GR.gradient_subspace(torch.cat(v, 0), rmax, seed=A.cell_seed("grad", k, rmax))
                for k, v in groups.items()}

    def _plan_for(self, cells: Sequence[Cell], pairs: Sequence[Pair], bases: Dict[str, torch.Tensor],
                  with_carry: bool = True):
        """Host-side plan of a batch: int arrays (one row per cell, cell ``i`` = row/slot ``i``) plus the
        projection basis rows to upload (row ``i * rmax + j`` = j-th direction of proj cell ``i``)."""
        K = self.iv.spikes_k
        mmax = max([max(self.iv.budgets or [1]), max(self.iv.ranks or [1])])
        if self._with_swap[0] or self._swap_kinds(cells)[0]:
            mmax = max(mmax, 2 * max(self.iv.budgets or [1]))      # sae_swap: the target's and the donor's latents
        rmax = max(self.iv.ranks) if self.iv.ranks else 1
        B = self.B
        sp = np.full((B, K), -1, dtype=np.int32)
        ix = np.zeros((B, mmax), dtype=np.int32)
        cn = np.zeros(B, dtype=np.int32)
        kd = np.zeros(B, dtype=np.int8)
        sd = np.zeros(B, dtype=np.int64)                   # noise streams of the sae_noise / proj_noise rows
        db = np.full(B, -1, dtype=np.int32)                # first donor-table row of the swap rows (row b * K + k)
        dn_dst: List[int] = []                             # donor table: rows to fill, and (donor pair, response
        dn_src: List[Tuple[int, int]] = []                 # index) of the residual that goes there
        tgt: Dict[str, Tuple[List[int], List[int]]] = {}   # pooled basis -> (table rows, its rows)
        rproj: Tuple[List[int], List[int], List[int]] = ([], [], [])   # random controls: (first row, rank, seed)
        by_pair: Dict[int, List[int]] = {}
        for ci, c in enumerate(cells):
            by_pair.setdefault(c.pair, []).append(ci)
        for pi, cis in by_pair.items():
            p = pairs[pi]
            s_abs = p.spikes_abs[:K]
            ca = np.asarray(cis)
            if s_abs:
                sp[ca, : len(s_abs)] = s_abs
            rnd = [ci for ci in cis if cells[ci].kind == "sae" and
                   cells[ci].method not in ("sae_targeted", "sae_noise", SPLICE_METHOD) + SWAP_METHODS]
            if rnd:
                got = A.random_latents_batch(self.sae.d_sae, [cells[ci].budget for ci in rnd],
                                             [cells[ci].seed for ci in rnd],
                                             [p.targeted[: cells[ci].budget] for ci in rnd], pool=p.active_pool)
                for ci, g in zip(rnd, got):
                    ix[ci, : len(g)] = g
                    cn[ci] = len(g)
                kd[rnd] = 1
            tg = np.asarray(p.targeted[:mmax], dtype=np.int32)
            self._plan_swap_rows(cells, cis, p, pairs, K, rmax, bases, ix, cn, kd, db, dn_dst, dn_src, tgt, rproj)
            for ci in cis:
                c = cells[ci]
                if c.method in SWAP_METHODS:
                    continue
                if c.kind == "sae":
                    if c.method in ("sae_targeted", "sae_noise"):     # the control takes the targeted cell's latents
                        n = min(c.budget, tg.size)
                        ix[ci, :n] = tg[:n]
                        cn[ci] = n
                        if c.method == "sae_targeted":
                            kd[ci] = 1
                        else:
                            kd[ci], sd[ci] = 3, c.seed
                    elif c.method == SPLICE_METHOD:
                        kd[ci] = 1                   # nothing ablated (cnt 0): the row is spliced as it is
                else:
                    if c.method in ("proj_targeted", "proj_noise"):   # ... and the targeted cell's basis rows
                        bk = p.word if self.iv.pca_pool == "word" else "__all__"
                        r = min(c.budget, int(bases[bk].shape[0]))
                        dst, src = tgt.setdefault(bk, ([], []))
                        dst.extend(range(ci * rmax, ci * rmax + r))
                        src.extend(range(r))
                    else:
                        r = c.budget
                        rproj[0].append(ci * rmax)
                        rproj[1].append(r)
                        rproj[2].append(c.seed)
                    ix[ci, :r] = np.arange(ci * rmax, ci * rmax + r)
                    cn[ci] = r
                    kd[ci] = 2
                    if c.method == "proj_noise":
                        kd[ci], sd[ci] = 4, c.seed
        basis = None
        # largest rank first (a basis costs ~r^2 block reductions; the workgroups are dispatched in order)
        lpt = np.argsort(-np.asarray(rproj[1], np.int64), kind="stable")
        if tgt or rproj[0]:       # filled on the device by _load_plan: gathers of the pooled bases + random_basis
            basis = {"tgt": {k: (np.asarray(d, np.int64), np.asarray(sr, np.int64)) for k, (d, sr) in tgt.items()},
                     "bases": {k: bases[k] for k in tgt},
                     "rnd": tuple(np.asarray(v, t)[lpt] for v, t in zip(rproj, (np.int64, np.int32, np.int64)))}
        plan = {"spikes": sp, "kind": kd, "idx": ix, "cnt": cn, "seeds": sd, "basis": basis, "rows": B * rmax,
                "rmax": rmax, "donor_base": db,
                "donor": (np.asarray(dn_dst, np.int64), dn_src, pairs) if dn_dst else None,
                "f": self._effective_first_edit(cells, pairs, by_pair, kd, ix, cn)}
        return self._plan_add_carry(plan) if with_carry else plan

    def _plan_swap_rows(self, cells, cis, p, pairs, K, rmax, bases, ix, cn, kd, db, dn_dst, dn_src, tgt, rproj) -> None:
        """The swap cells of pair ``p`` (plan rows ``cis``): their selected sets, kinds 5 / 6, and the donor rows of
        their spikes -- plan row ``ci`` reads donor-table rows ``ci * K + k``, the donor's residual at its
        ``k mod n``-th spike (``n`` = the donor's spike count)."""
        for ci in cis:
            c = cells[ci]
            if c.method not in SWAP_METHODS:
                continue
            q = pairs[c.donor]
            qs = [t for t in q.spikes_rel if 0 <= t < q.resid.shape[0]]
            assert qs, "swap cell whose donor has no spikes (make_cells skips those pairs)"
            db[ci] = ci * K
            for k in range(len(p.spikes_abs[:K])):
                dn_dst.append(ci * K + k)
                dn_src.append((c.donor, qs[k % len(qs)]))
            if c.method == "sae_swap":
                lat = list(dict.fromkeys(list(p.targeted[: c.budget]) + list(q.targeted[: c.budget])))
            elif c.method == "sae_swap_random":
                excl = list(dict.fromkeys(list(p.targeted[: c.budget]) + list(q.targeted[: c.budget])))
                own = A.random_latents(self.sae.d_sae, c.budget, c.seed, exclude=excl, pool=p.active_pool)
                oth = A.random_latents(self.sae.d_sae, c.budget, A.cell_seed(c.seed, "donor"), exclude=excl,
                                       pool=q.active_pool)
                lat = list(dict.fromkeys(list(own) + list(oth)))
            if c.kind == "sae":
                lat = lat[: ix.shape[1]]
                ix[ci, : len(lat)] = lat
                cn[ci] = len(lat)
                kd[ci] = 5
                continue
            if c.method == "proj_swap":
                r = min(c.budget, int(bases["__all__"].shape[0]))
                dst, src = tgt.setdefault("__all__", ([], []))
                dst.extend(range(ci * rmax, ci * rmax + r))
                src.extend(range(r))
            else:
                r = c.budget
                rproj[0].append(ci * rmax)
                rproj[1].append(r)
                rproj[2].append(c.seed)
            ix[ci, :r] = np.arange(ci * rmax, ci * rmax + r)
            cn[ci] = r
            kd[ci] = 6

    def _sae_key(self) -> Optional[tuple]:
        """Identity + in-place version of the SAE tensors an edit's coefficients depend on: an activity table
        built under other parameters (e.g. before ``calibrate()``) is never used."""
        s = self.sae
        if s is None:
            return None
        ts = [s.W_encT, s.b_enc, s.threshold] + ([s.b_dec] if s.apply_b_dec_to_input else [])
        return tuple((id(t), t._version) for t in ts) + (getattr(s, "param_version", 0), float(self.iv.alpha))

    def _effective_first_edit(self, cells, pairs, by_pair, kd, ix, cn) -> np.ndarray:
        """Per cell (plan row): response index of its first spike where the edit is non-zero (the pair's spike
        order), ``len(resp)`` if it never is (the cell is its baseline), -1 = the pair's first spike (projection
        cells, or no activity table).  Latents outside a pair's activity table count as active everywhere.  A
        ``sae_noise`` row (kind 3) is zero exactly where its targeted twin is."""
        K = self.iv.spikes_k
        f = np.full(self.B, -1, np.int64)
        if not self.skip_noop_spikes or self.ablation_mode == "reconstruct" or self.affine:
            # reconstruct: R(h) != h at every spike, no cell is its baseline; clamp / steer: inactive latents move too
            return f
        key = self._sae_key()
        for pi, cis in by_pair.items():
            p = pairs[pi]
            ids, msk = p.act_ids, p.act_mask
            if p.act_key != key:
                continue                        # stale or missing table: every cell edits from the first spike
            sp = np.asarray(p.spikes_rel[:K], np.int64)
            ca = np.asarray([ci for ci in cis if kd[ci] == 1 or kd[ci] == 3], np.int64)
            if ids is None or not ca.size or not sp.size:
                continue
            lat = ix[ca].astype(np.int64)
            j = np.minimum(np.searchsorted(ids, lat), max(ids.size - 1, 0))
            found = (ids[j] == lat) if ids.size else np.zeros(lat.shape, bool)
            allk = (1 << sp.size) - 1
            bits = np.where(found, msk[j] if ids.size else 0, allk)
            bits = np.where(np.arange(lat.shape[1])[None, :] < cn[ca][:, None], bits, 0)
            cell_bits = np.bitwise_or.reduce(bits, axis=1)
            on = (cell_bits[:, None] >> np.arange(sp.size)[None, :]) & 1
            f[ca] = np.where(on.astype(bool), sp[None, :], len(p.resp)).min(1)
        return f

    def _plan_add_carry(self, plan: dict) -> dict:
        for cr in self._carry:                  # carried cells keep editing at their carry-region slots
            cs_, ck_, ci_, cc_, sd_ = cr.plan_row
            plan["spikes"][cr.slot] = cs_
            plan["kind"][cr.slot] = ck_
            plan["idx"][cr.slot] = ci_
            plan["cnt"][cr.slot] = cc_
            plan["seeds"][cr.slot] = sd_
        return plan

    def prefetch(self, pairs: Sequence[Pair], methods: Sequence[str] = METHODS):
        """Build a future step's cells and host edit plan on a helper thread (pure host work: cell
        enumeration, seeded random latent sets, plan arrays) while the GPU runs the current step.
        Needs the pairs' baselines (spikes, targeted latents) to be final.  Pass the result to
        :meth:`run_cells` / :meth:`run_cells_async` as ``prefetched``; ``None`` if it cannot apply."""
        if not pairs or any(p.resid is None for p in pairs):
            return None
        if any(not m.startswith("sae") or m in SWAP_METHODS for m in methods):
            # projection cells: their plan needs the pooled PCA bases (device work, main thread); the cells are
            # enumerated here (the random-control bases are drawn on the device when the plan loads).  Swap cells
            # likewise: their plan reads the donor pairs' residuals
            if getattr(self, "_prefetch_pool", None) is None:
                from concurrent.futures import ThreadPoolExecutor

                self._prefetch_pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="tb-prefetch")
            return self._prefetch_pool.submit(lambda: (self.make_cells(pairs, methods), None))
        if getattr(self, "_prefetch_pool", None) is None:
            from concurrent.futures import ThreadPoolExecutor

            self._prefetch_pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="tb-prefetch")

        def work():
            t0 = time.perf_counter()
            cells = self.make_cells(pairs, methods)
            t1 = time.perf_counter()
            out = (cells, None) if len(cells) > self.B else (cells, self._plan_for(cells, pairs, {}, with_carry=False))
            t2 = time.perf_counter()
            self.timings["prefetch_cells"] = self.timings.get("prefetch_cells", 0.0) + t1 - t0
            self.timings["prefetch_plan"] = self.timings.get("prefetch_plan", 0.0) + t2 - t1
            return out
        return self._prefetch_pool.submit(work)

    def _load_plan(self, plan: dict) -> EditHook:
        """Upload into the persistent plan (fixed tensors, so a captured decode graph stays valid)."""
        dev = self.dev
        if self._plan is None:
            t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
            basis = torch.zeros(plan["rows"], self.D, dtype=torch.float32, device=dev) if self._with_basis else None
            # clamp / steer: every selected latent has the same target, so the plan's values never change
            values = torch.full(plan["idx"].shape, self.clamp_value, dtype=torch.float32, device=dev) \
                if self.affine else None
            # the noise paths exist only in a plan built for a call with noise cells (self._with_noise): every other
            # sweep runs the kernels it ran before
            noise = tuple(self._with_noise)
            # likewise the swap paths and their donor table ([B * K, D], model dtype): only in a plan built for a call
            # with swap cells
            swap = tuple(self._with_swap)
            donor = torch.zeros(plan["spikes"].shape[0] * plan["spikes"].shape[1], self.D, dtype=self.m.dtype,
                                device=dev) if any(swap) else None
            self._plan = EditPlan(t(plan["spikes"]), t(plan["kind"]), t(plan["idx"]), t(plan["cnt"]), self.iv.alpha,
                                  basis, self.ablation_mode, values=values,
                                  seeds=t(plan["seeds"]) if any(noise) else None, has_noise=noise, donor=donor,
                                  donor_base=t(plan["donor_base"]) if any(swap) else None, has_swap=swap)
            self._hook = EditHook(self._plan, self.sae)
        else:
            for f in ("spikes", "kind", "idx", "cnt") + (("seeds",) if self._plan.seeds is not None else ()) + \
                    (("donor_base",) if self._plan.donor_base is not None else ()):
                getattr(self._plan, f).copy_(_h2d(plan[f], dev), non_blocking=True)
        if plan.get("donor") is not None:
            # the donor rows of this batch's swap cells, gathered on the device from the donor pairs' kept residuals
            assert self._plan.donor is not None, "swap cells need a plan built with a donor table"
            dst, src, prs = plan["donor"]
            up = lambda a: _h2d(a, dev).to(dev, non_blocking=True)   # noqa: E731
            uniq = sorted({j for j, _ in src})
            off, n = {}, 0
            for j in uniq:
                off[j] = n
                n += int(prs[j].resid.shape[0])
            R = torch.cat([prs[j].resid for j in uniq], 0) if len(uniq) > 1 else prs[uniq[0]].resid
            rows = np.asarray([off[j] + t for j, t in src], np.int64)
            self._plan.donor.index_copy_(0, up(dst), R.index_select(0, up(rows)).to(self._plan.donor.dtype))
        if plan["basis"] is not None:
            assert self._plan.basis is not None, "projection cells need a plan built with a basis table"
            pb, tab = plan["basis"], self._plan.basis
            up = lambda a: _h2d(a, dev).to(dev, non_blocking=True)   # noqa: E731
            for bk, (dst, src) in pb["tgt"].items():
                U = pb["bases"][bk]          # pooled bases live on the host (one small upload per basis and batch)
                U = (up(U) if U.device.type == "cpu" else U).float()
                tab.index_copy_(0, up(dst), U.index_select(0, up(src)))
            rows, ranks, seeds = pb["rnd"]
            if rows.size:
                ops.random_basis(up(seeds), up(ranks), up(rows), tab)
        return self._hook

    # ---------------------------------------------------- cross-batch pipeline
    def stage_next(self, nb: "NextBatch") -> None:
        """Announce the batch the next :meth:`run_cells` call will run.  Once this batch's readout is
        queued, its edit plan is uploaded and its teacher-forced tail is queued behind it on the GPU
        (:meth:`_launch_staged_next`), so the device never idles while the host builds this batch's
        records and the next batch's decode rows.  Exact: the tail only writes the next cells' KV slots
        (blocks after the hooked layer) and capture rows, which this batch no longer reads once its lens
        is queued; stream order does the rest."""
        self._next = nb

    def _launch_staged_next(self) -> None:
        nb = getattr(self, "_next", None)
        self._next = None
        if nb is not None and nb.cells is not None and nb.cells is getattr(self, "_running_cells", None):
            nb = None                            # announced batch is the one running now: nothing to stage
        # carried decode rows move out of the cell slots before the next tail writes them (stream order)
        mv = self._carry_move_pending
        self._carry_move_pending = None
        if mv is not None:
            mv()
        if nb is None or not (self.layer_resume and self.prefix_share):
            return
        nb.resolve(self)
        cp = [nb.pairs[c.pair] for c in nb.cells]
        proj = any(c.kind == "proj" for c in nb.cells)
        if not nb.cells or len(nb.cells) > self.B or not self._resumable(cp) or \
                (proj and (self._plan is None or self._plan.basis is None)):
            return
        if self._plan is None or any(w and not h for w, h in zip(self._noise_kinds(nb.cells), self._plan.has_noise)):
            return                               # the plan has no noise path yet: run_cells rebuilds it
        if any(w and not h for w, h in zip(self._swap_kinds(nb.cells), self._plan.has_swap)):
            return                               # likewise the swap paths
        if nb.plan is None:      # bases pooled over the call's pairs, as run_cells computes them
            nb.plan = self._plan_for(nb.cells, nb.pairs,
                                     self._bases(nb.pairs, self._needs_all_pool(nb.cells)) if proj else {},
                                     with_carry=False)
        plan = nb.plan
        nb.plan = plan
        if self._carry:                          # the next decode continues this batch's carried rows
            plan = self._plan_add_carry({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in plan.items()})
        self._set_adapters(cp)
        hook = self._load_plan(plan)
        tf = self._tf_launch(cp, {self.layer: [hook, self.capture]}, plan.get("f"))
        self._staged = {"cells": nb.cells, "plan": plan, "tf": tf, "carry": list(self._carry)}
        self._tick("next_tf_launched")
