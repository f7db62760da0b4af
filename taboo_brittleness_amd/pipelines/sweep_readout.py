"""Sweep readouts (part of :class:`~.sweep.SweepRunner`): the per-cell records after a decode -- logit-lens response
sums reused from the baseline's running sums, top-k guesses, secret probabilities and decoys, the teacher-forced
tail NLL of the edited model on the baseline response (packed rows, fused vocab head) and the leak verdicts.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import ops
from ..interp import analysis as A
from ..interp.edits import ComponentHook, EditHook, TraceHook, component_tables
from ..interp.logit_lens import excl_table, lens_packed, lens_readout, reference_exclusions, vocab_slice, vocab_topk
from ..interp.prompts import contains_secret
from .sweep_types import NOISE_METHODS, SWAP_METHODS, Cell, Pair, _h2d, _nullctx

# bf16 logits per vocab-head GEMM chunk of the teacher-forced tail: 2 GB (4096 rows) measured +0.65 % over 1 GB at the
# same 263 GB peak; 4 GB +0.3 % more but 276 GB peak (profiles/r5/bench/head_chunk/)
HEAD_LOGITS_BYTES = 2 << 30
# teacher-forced tail rows per forward chunk (whole cells; chunks alternate between two streams): 24576 / 49152
# measured within noise of 32768 (profiles/r5/bench/tail_chunk/)
TAIL_CHUNK_ROWS = 32768



class ReadoutMixin:
    """Methods of :class:`~.sweep.SweepRunner` (state lives on the runner; see its docstring)."""

    def _resume_readout(self, entries, out, tf: Optional[dict] = None) -> List[dict]:
        """Lens readout + result records of layer-resumed cells.  The host side is columnar: one set of
        numpy arrays for the whole batch (no per-cell Python work on the launching thread); every
        non-diverged cell of a pair shares the pair's response, spikes and exclusions.

        ``entries``: per cell ``(cell, pair, slot, D or None, nll_edit, self_nll or None, out row or None, f)``
        — ``slot`` holds its capture-store rows, diverged cells read their response from ``out``; spikes before
        the cell's effective first edit ``f`` were no-op edits, their lens is the baseline's.  ``tf`` (output
        readout only): the batch's finished teacher-forced tail, whose tracked rows fill the cells' tables."""
        m = self.m
        S1 = self.store.shape[1]
        E_n = len(entries)
        batch = [e[0] for e in entries]
        cell_pairs = [e[1] for e in entries]
        # ---- per unique pair: response length, prompt length, spikes (kept order), tracked ids, tokens
        uid: Dict[int, int] = {}
        ulist: List[Pair] = []
        u_a = np.empty(E_n, np.int64)
        for i, p in enumerate(cell_pairs):
            u = uid.get(id(p))
            if u is None:
                u = uid[id(p)] = len(ulist)
                ulist.append(p)
            u_a[i] = u
        K = max(len(p.track) for p in ulist)
        Ks = max(1, max(len(p.spikes_rel) for p in ulist))
        U = len(ulist)
        n_u = np.asarray([len(p.resp) for p in ulist], np.int64)
        plen_u = np.asarray([p.plen for p in ulist], np.int64)
        sp_u = np.full((U, Ks), -1, np.int64)
        trk_u = np.full((U, K), -1, np.int64)
        for u, p in enumerate(ulist):
            sp = [x for x in p.spikes_rel if x < len(p.resp)]
            sp_u[u, : len(sp)] = sp
            trk_u[u, : len(p.track)] = p.track
        slot_a = np.asarray([e[2] for e in entries], np.int64)
        dv_a = np.asarray([-1 if e[3] is None else e[3] for e in entries], np.int64)
        j_a = np.asarray([-1 if e[6] is None else e[6] for e in entries], np.int64)
        nll_a = np.asarray([e[4] for e in entries], np.float64)
        f_e = np.asarray([e[7] if len(e) > 7 else 0 for e in entries], np.int64)
        div = dv_a >= 0
        host_tok = out.host_tokens() if (out is not None and div.any()) else None
        ngen_o = np.asarray(out.n_gen, np.int64) if out is not None else np.zeros(0, np.int64)
        ng_a = n_u[u_a].copy()
        d_a = n_u[u_a].copy()
        ng_a[div] = ngen_o[j_a[div]]
        d_a[div] = dv_a[div]
        # self NLL: the teacher-forced value for undiverged cells, the decode's own for diverged ones
        sn_a = np.asarray([np.nan if e[5] is None else e[5] for e in entries], np.float64)
        if div.any():
            tn = out.tok_nll.float().cpu().numpy()[j_a[div]]
            ngd = ng_a[div]
            msk = np.arange(tn.shape[1])[None, :] < ngd[:, None]
            sums = np.where(msk, tn, 0.0).sum(1, dtype=np.float64)
            sn_a[div] = np.where(ngd > 0, sums / np.maximum(ngd, 1), np.nan)
        # ---- rows to evaluate per cell: its spikes before min(D, n_gen) (pair order), then D .. n_gen-1
        lim = np.where(div, np.minimum(d_a, ng_a), n_u[u_a])
        spk = sp_u[u_a]
        keep = (spk >= 0) & (spk < lim[:, None]) & (spk >= f_e[:, None])
        order = np.argsort(~keep, axis=1, kind="stable")
        spk_c = np.take_along_axis(spk, order, 1)
        cnt_s = keep.sum(1)
        cnt_t = np.where(div, np.maximum(ng_a - d_a, 0), 0)
        cnt = cnt_s + cnt_t
        offs = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        R = int(offs[-1])
        cell_of = np.repeat(np.arange(E_n), cnt)
        q = np.arange(R, dtype=np.int64) - offs[cell_of]
        cs = cnt_s[cell_of]
        pos = np.where(q < cs, spk_c[cell_of, np.minimum(q, Ks - 1)], d_a[cell_of] + q - cs)
        rows = slot_a[cell_of] * S1 + plen_u[u_a][cell_of] + pos
        trk = trk_u[u_a][cell_of]
        ex = np.full((R, 2), -1, np.int64)
        if self.exclusion == "reference" and R:
            etab = excl_table(self.tok, m.spec.vocab_size)
            Lm = int(max(1, n_u.max(), ng_a.max() if E_n else 1))
            tok_u = np.zeros((U, Lm), np.int64)
            for u, p in enumerate(ulist):
                tok_u[u, : len(p.resp)] = p.resp
            tokm = tok_u[u_a]
            if div.any():
                w = min(Lm, host_tok.shape[1])
                tokm[np.nonzero(div)[0], :w] = host_tok[j_a[div], :w]
            cur = etab[tokm]
            ex[:, 0] = cur[cell_of, pos]
            ex[:, 1] = np.where(pos > 0, cur[cell_of, np.maximum(pos - 1, 0)], -1)
        row_key = self._lens_row_keys(cell_of, pos, q >= cs, div, j_a, u_a, sp_u, host_tok) if R else None
        row_key, row_check = row_key if row_key is not None else (None, None)
        self._tick("ro_entries")
        self.stats["lens_rows"] += R
        self._ensure_cum(ulist)
        base = self._lens_base(cell_pairs, d_a.tolist(), ng_a.tolist(), f_e)
        self._tick("ro_base")
        acc, pr_d = lens_packed(m, self.store, rows, offs, base, trk, ex, sync=False, row_key=row_key,
                                stats=self.stats, row_check=row_check)
        if self.exclusion == "response":
            lo, Vl = vocab_slice(m)
            for i in range(E_n):
                r_ = cell_pairs[i].resp if dv_a[i] < 0 else host_tok[j_a[i], : ng_a[i]].tolist()
                ids = torch.tensor(sorted(set(r_)), dtype=torch.long, device=self.dev) - lo
                ids = ids[(ids >= 0) & (ids < Vl)]
                if ids.numel():
                    acc[i, ids] = 0.0
        vals, ids = vocab_topk(m, acc, self.cfg.model.top_k)
        # every readout output in one async D2H (pinned), so the next batch's teacher-forced tail can be
        # queued behind this batch's lens before the host waits for it
        vh_d, ih_d = vals.sum(1), ids
        if self.dev.type == "cuda":
            host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (pr_d, vh_d, ih_d)]
            for h, t in zip(host, (pr_d, vh_d, ih_d)):
                h.copy_(t, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.dev))
        else:
            host, ev = [pr_d, vh_d, ih_d], None
        self._tick("lens_launched")
        self._launch_staged_next()
        if ev is not None:
            ev.synchronize()
        pr, vh, ih = (t.numpy() for t in host)
        self._tick("lens")
        cols = {"ng": ng_a, "d": d_a, "div": div, "j": j_a, "sn": sn_a, "nll": nll_a, "pos": pos,
                "cell_of": cell_of, "host_tok": host_tok,
                # swap cells: their donor pairs, resolved now (the records may be built after the next call began)
                "donors": [self._run_pairs[c.donor] if c.donor >= 0 else None for c in batch]}
        if self.output_readout:
            # the pieces of every cell's output-readout table: the tail's rows (row r0 + t - f = index t + 1) and, for
            # diverged cells, the decode's columns (host copies now: the buffers are reused by the next batch)
            cols["ro"] = {"lp": tf.get("logp"), "rk": tf.get("rank"), "r0": tf["r0"][slot_a], "E": tf["E"][slot_a],
                          "f": f_e,
                          "dlp": out.tok_logp.cpu().numpy() if div.any() else None,
                          "drk": out.tok_rank.cpu().numpy() if div.any() else None}
        if self.output_shift:
            # the tail's per-row KLs against the baseline rows; a cell's rows start at r0 (tail row f)
            cols["shift"] = {"kl": tf.get("kl"), "kl_rev": tf.get("kl_rev"), "r0": tf["r0"][slot_a], "f": f_e}
        if self.output_movers:
            # the tail's compact movers outputs: a cell's selected rows (its spikes t >= f, in order) start at m0
            cols["movers"] = {"mv": tf.get("movers"), "m0": tf["mv_m0"][slot_a], "at": tf["mv_at"], "f": f_e}
        if self.component_trace:
            # the tail's component slabs over its selected rows: a cell's rows (response indices ts) start at i0
            cols["comp"] = {"c": tf.get("comp"), "i0": tf["ct_i0"][slot_a], "ts": [tf["ct_ts"][s] for s in slot_a]}
        if self.layer_trace:
            # the tail's [Lt, M, T] lens logits; a cell's rows f .. E start at r0
            cols["trace"] = {"z": tf.get("trace"), "r0": tf["r0"][slot_a], "f": f_e, "E": tf["E"][slot_a]}
        if getattr(self, "_defer", False):
            return self._records_pool().submit(self._resume_records, batch, cell_pairs, cols, pr, vh, ih, K)
        return self._resume_records(batch, cell_pairs, cols, pr, vh, ih, K)

    def _lens_row_keys(self, cell_of, pos, after_d, div, j_a, u_a, sp_u, host_tok) -> Optional[np.ndarray]:
        """Dedup keys of the lens rows (``lens_packed(row_key=)``): the hooked-layer residual of a diverged cell at
        a non-spike position ``t >= D`` is a function of its pair and its tokens ``0..t`` alone (blocks ``0..l``
        see only tokens, and no edit touches it), so cells of one pair with equal tokens up to ``t`` hold the
        same row.  Those rows get a 63-bit hash key of (pair, t, tokens ``0..t``) plus a second independent hash
        as a collision check (``lens_packed(row_check=)``); every other row (spikes, undiverged cells) a unique
        negative key.  Returns ``(keys, checks)``, or None when nothing can repeat."""
        R = len(pos)
        if not self.trie_decode or host_tok is None or not div.any():
            return None
        spike = (sp_u[u_a][cell_of] == pos[:, None]).any(1)
        dd = after_d & div[cell_of] & ~spike
        key = -1 - np.arange(R, dtype=np.int64)
        if not dd.any():
            return None
        # rolling 64-bit hash of every diverged cell's response prefix (wrapping uint64 arithmetic)
        tok = host_tok[j_a[div]].astype(np.uint64) + np.uint64(1)
        h = np.empty(tok.shape, np.uint64)
        h2 = np.empty(tok.shape, np.uint64)
        acc = np.zeros(tok.shape[0], np.uint64)
        acc2 = np.full(tok.shape[0], 0x243F6A8885A308D3, np.uint64)
        mul, mul2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD6E8FEB86659FD93)
        with np.errstate(over="ignore"):
            for t in range(tok.shape[1]):
                acc = (acc ^ tok[:, t]) * mul
                acc ^= acc >> np.uint64(29)
                h[:, t] = acc
                acc2 = (acc2 + tok[:, t] * np.uint64(0x9FB21C651E98DF25)) * mul2
                acc2 ^= acc2 >> np.uint64(31)
                h2[:, t] = acc2
            ci = np.full(len(div), -1, np.int64)
            ci[np.nonzero(div)[0]] = np.arange(int(div.sum()))
            r = np.nonzero(dd)[0]
            c = ci[cell_of[r]]
            t = np.minimum(pos[r], tok.shape[1] - 1)
            k = h[c, t] ^ (u_a[cell_of[r]].astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F))
            k ^= pos[r].astype(np.uint64) * np.uint64(0x165667B19E3779F9)
            k2 = h2[c, t] ^ (u_a[cell_of[r]].astype(np.uint64) * np.uint64(0x85EBCA77C2B2AE63))
        key[r] = (k & np.uint64(0x7FFFFFFFFFFFFFFF)).astype(np.int64)
        chk = np.arange(R, dtype=np.int64)
        chk[r] = k2.view(np.int64)
        return key, chk

    def _resume_records(self, batch, cell_pairs, cols, pr, vh, ih, K) -> List[dict]:
        """Host half of :meth:`_resume_readout`: per-cell readout statistics and result records."""
        nc = len(cell_pairs)
        ng_a, d_a, div, j_a = cols["ng"], cols["d"], cols["div"], cols["j"]
        host_tok = cols["host_tok"]
        # ---- per-cell tracked-id probability tables, vectorised: baseline rows up to D, evaluated rows
        Lmax = int(max(1, ng_a.max() if nc else 1))
        P3 = np.zeros((nc, Lmax, K), dtype=np.float32)
        groups: Dict[int, List[int]] = {}
        for b, p in enumerate(cell_pairs):
            groups.setdefault(id(p), []).append(b)
        for bs in groups.values():
            p = cell_pairs[bs[0]]
            tp = p.track_probs
            if tp is None or not len(p.resp):
                continue
            same = [b for b in bs if d_a[b] >= len(p.resp)]          # undiverged: all baseline rows
            if same:
                P3[np.asarray(same), : tp.shape[0], : tp.shape[1]] = tp[None]
            for b in bs:
                if d_a[b] < len(p.resp):
                    keep = min(int(d_a[b]), int(ng_a[b]), tp.shape[0])
                    P3[b, :keep, : tp.shape[1]] = tp[:keep]
        if cols["pos"].size:
            P3[cols["cell_of"], cols["pos"]] = pr
        valid = np.arange(Lmax)[None, :] < ng_a[:, None]
        p0 = np.where(valid, P3[:, :, 0], 0.0)
        cnt = np.maximum(ng_a, 1)
        ps_mean = p0.sum(1) / cnt
        ps_final = P3[np.arange(nc), np.maximum(ng_a - 1, 0), 0]
        ps_max = np.where(valid, P3[:, :, 0], -np.inf).max(1) if nc else np.zeros(0)
        decoy = (np.where(valid[:, :, None], P3[:, :, 2:], 0.0).sum(1) / cnt[:, None]) if K > 2 else None
        results = []
        ro = cols.get("ro")
        sft = cols.get("shift")
        trc = cols.get("trace")
        mvs = cols.get("movers")
        cmp_ = cols.get("comp")
        for b, (c, p) in enumerate(zip(batch, cell_pairs)):
            ng = int(ng_a[b])
            resp = host_tok[j_a[b], :ng].tolist() if div[b] else p.resp
            rot = None
            if ro is not None:
                rot = self._out_table(p, ng, int(ro["f"][b]), int(ro["E"][b]), int(ro["r0"][b]),
                                      int(d_a[b]) if div[b] else None, ro["lp"], ro["rk"],
                                      (ro["dlp"][j_a[b]], ro["drk"][j_a[b]]) if div[b] else None)
            topk = ih[b].tolist() if ng > 0 and vh[b] > 0 else []
            stats = (float(ps_mean[b]), float(ps_final[b]), float(ps_max[b])) if ng else (0.0, 0.0, 0.0)
            dec = decoy[b, : p.n_decoys].tolist() if (decoy is not None and ng and p.n_decoys > 0) else []
            q = cols["donors"][b]
            results.append(self._cell_record(c, p, ng, resp, stats, dec, topk, float(cols["nll"][b]),
                                             float(cols["sn"][b]), q,
                                             P3[b, :ng, p.extra.get(q.word, 0)] if q is not None else None, ro=rot))
            if sft is not None:                  # output shift only: the other runs keep their keys
                results[-1].update(self._shift_fields(p, int(sft["f"][b]), int(sft["r0"][b]), sft["kl"],
                                                      sft["kl_rev"]))
            if mvs is not None:                  # output movers only: the other runs keep their keys
                results[-1].update(self._movers_fields(p, int(mvs["f"][b]), int(mvs["m0"][b]), mvs["at"], mvs["mv"],
                                                       q if c.method in SWAP_METHODS else None))
            if cmp_ is not None:                 # component trace only: the other runs keep their keys
                results[-1].update(self._comp_fields(p, int(cmp_["i0"][b]), cmp_["ts"][b], cmp_["c"],
                                                     c.method in SWAP_METHODS))
            if trc is not None:                  # layer trace only: the other runs keep their keys
                results[-1].update(self._trace_fields(p, int(trc["f"][b]), int(trc["E"][b]), int(trc["r0"][b]),
                                                      trc["z"], q if c.method in SWAP_METHODS else None))
        return results

    @staticmethod
    def _out_table(p: Pair, ng: int, f: int, E: int, r0: int, D: Optional[int], lp, rk, dec):
        """A layer-resumed cell's output-readout table ``(logp, rank) [ng, K]``, assembled like its lens table ``P3``:
        the baseline's rows for indices ``<= f`` (the distribution choosing token ``i`` comes from position ``i - 1``,
        before the first edit), tail row ``t`` at index ``t + 1`` up to the divergence ``D`` (undiverged: to the
        tail's end), the decode's own columns from ``D + 1`` on."""
        K = len(p.track)
        inv = np.argsort(p.ro_order())                # the head's table order -> track order (the baseline's is)
        LP = np.zeros((ng, K), np.float32)
        RK = np.full((ng, K), -1, np.int32)
        nb = min(f + 1, ng, p.out_logp.shape[0])
        LP[:nb], RK[:nb] = p.out_logp[:nb, :K], p.out_rank[:nb, :K]
        hi = min((E if D is None else min(E, D - 1)) + 2, ng)          # tail indices f + 1 .. hi - 1
        if hi > f + 1 and lp is not None:
            LP[f + 1: hi] = lp[r0: r0 + hi - f - 1, :K][:, inv]
            RK[f + 1: hi] = rk[r0: r0 + hi - f - 1, :K][:, inv]
        if D is not None and dec is not None and ng > D + 1:
            LP[D + 1: ng] = dec[0][D + 1: ng, :K][:, inv]
            RK[D + 1: ng] = dec[1][D + 1: ng, :K][:, inv]
        return LP, RK

    @staticmethod
    def _out_fields(p: Pair, lp: np.ndarray, rk: np.ndarray, donor: Optional[Pair] = None) -> dict:
        """Record fields of the output readout from a per-position table ``(logp, rank) [n, K]`` (one code path for
        every way the table was obtained, so equal tables give equal fields).  Per position ``s_i`` = max log-prob and
        ``r_i`` = min rank over the secret's two forms.  ``logp_out_spike_mean`` runs over the pair's spikes: every
        cell edits all of its pair's spikes (its plan row takes ``Pair.spikes_abs[:spikes_k]``, and ``select_spikes``
        returns at most ``spikes_k``), so these are the cell's edited spikes."""
        n = lp.shape[0]
        nan = float("nan")
        out = {"logp_out_mean": nan, "logp_out_max": nan, "logp_out_final": nan, "logp_out_spike_mean": nan,
               "rank_out_min": -1, "rank_out_median": nan, "decoy_logp_out": []}
        ok = [k for k in (0, 1) if k < len(p.track) and p.track[k] >= 0]
        if n and ok:
            s = lp[:, ok].astype(np.float64).max(1)
            r = rk[:, ok].astype(np.int64)
            r = np.where(r < 0, np.iinfo(np.int64).max, r).min(1)
            sp = [t + 1 for t in p.spikes_rel if t + 1 < n]
            out.update({"logp_out_mean": float(s.mean()), "logp_out_max": float(s.max()), "logp_out_final": float(s[-1]),
                        "logp_out_spike_mean": float(s[sp].mean()) if sp else nan,
                        "rank_out_min": int(r.min()), "rank_out_median": float(np.median(r))})
        if n and p.n_decoys > 0:
            out["decoy_logp_out"] = lp[:, 2: 2 + p.n_decoys].astype(np.float64).mean(0).tolist()
        if donor is not None:
            col = p.extra.get(donor.word, 0)
            out["logp_out_donor_mean"] = float(lp[:, col].astype(np.float64).mean()) if n else nan
            out["rank_out_donor_min"] = int(rk[:, col].min()) if n else -1
        return out

    @torch.no_grad()
    def _ensure_cum(self, pairs: Sequence[Pair]) -> None:
        """Running lens sums of ``pairs`` (lazy mode): recomputed from each pair's hooked-layer residuals with
        the same lens readout its baseline ran; sums rebuilt for earlier batches are released first."""
        need = [p for p in pairs if p.lens_cum is None and p.resid is not None]
        if not need:
            return
        keep = {id(p) for p in pairs}
        for q in self._cum_live:
            if id(q) not in keep:
                q.lens_cum = None
        self._cum_live = [q for q in self._cum_live if id(q) in keep]
        nmax = max(1, max(len(p.resp) for p in need))
        # rows past a response are never read (lens_readout points padding at the last, scratch row): only that
        # row is zeroed, and the residuals go in with one concatenation + one row scatter
        tmp = torch.empty(len(need), nmax + 1, self.D, dtype=self.store.dtype, device=self.dev)
        tmp[:, nmax].zero_()
        parts = [(i, p.resid[: len(p.resp)]) for i, p in enumerate(need) if len(p.resp)]
        if parts:
            dst = np.concatenate([i * (nmax + 1) + np.arange(r.shape[0]) for i, r in parts])
            tmp.view(-1, self.D).index_copy_(0, _h2d(dst, self.dev).to(self.dev, non_blocking=True),
                                             torch.cat([r for _, r in parts], 0))
        resp = [list(p.resp) for p in need]
        excl = [reference_exclusions(self.tok, r) for r in resp] if self.exclusion == "reference" else None
        lr = lens_readout(self.m, tmp, [0] * len(need), [len(r) for r in resp], [p.track for p in need],
                          top_k=self.cfg.model.top_k, exclusion=self.exclusion, excl_pairs=excl,
                          response_ids=resp, keep_cum=True)
        for p, c in zip(need, lr.cum):
            p.lens_cum = c
        self._cum_live += need

    def _lens_base(self, cell_pairs: Sequence[Pair], Dc: Sequence[int], ngen: Sequence[int],
                   f: Optional[np.ndarray] = None) -> torch.Tensor:
        """Reused part of each cell's response lens sum: the baseline's running sum up to the divergence
        ``D`` minus its spike positions from its effective first edit ``f`` on (those are re-evaluated on the
        edited residual; earlier spikes were no-op edits).  Per pair one small matmul of a {0, +-1} coefficient
        matrix over the pair's running sums, written straight into the pair's (contiguous) output rows; every
        coefficient of every pair goes up in one copy."""
        V = vocab_slice(self.m)[1]           # this rank's lens columns under vocab-parallel TP
        base = torch.empty(len(cell_pairs), V, dtype=torch.float32, device=self.dev)
        groups: Dict[int, List[int]] = {}
        for b, p in enumerate(cell_pairs):
            groups.setdefault(id(p), []).append(b)
        coefs: List[np.ndarray] = []
        plan = []
        co = 0
        for bs in groups.values():
            p = cell_pairs[bs[0]]
            n1 = p.lens_cum.shape[0]
            d = np.minimum(np.minimum(np.asarray([Dc[b] for b in bs]), np.asarray([ngen[b] for b in bs])), n1 - 1)
            sp = np.asarray([x for x in p.spikes_rel if x + 1 < n1], dtype=np.int64)
            nb = len(bs)
            # base[b] = C[d_b] - sum_{f_b <= s < d_b} (C[s + 1] - C[s]), as coefficients over the rows of C
            W = np.zeros((nb, n1), np.float32)
            W[np.arange(nb), d] = 1.0
            if sp.size:
                fb = np.asarray([f[b] for b in bs], np.int64) if f is not None else np.zeros(nb, np.int64)
                mk = ((sp[None, :] < d[:, None]) & (sp[None, :] >= fb[:, None])).astype(np.float32)
                np.add.at(W, (slice(None), sp + 1), -mk)
                np.add.at(W, (slice(None), sp), mk)
            coefs.append(W.ravel())
            plan.append((p, bs, n1, co))
            co += W.size
        if self.dev.type == "cuda":
            # one row-combination kernel over every cell: each cell's few non-zero coefficients (its divergence row
            # and its re-evaluated spike terms) in ascending row order -- a fixed per-cell sum, whatever the batch
            # (vectorised per pair: a per-cell host loop cost ~25 ms of GPU idle per step, profiles/r6/prof/head2)
            B = len(cell_pairs)
            basep = np.zeros(B, np.int64)
            bl, pl, cl = [], [], []
            for (p, bs, n1, c), W in zip(plan, coefs):
                W = W.reshape(len(bs), n1)
                assert p.lens_cum.stride(-1) == 1 and p.lens_cum.dtype == torch.float32
                bsa = np.asarray(bs, np.int64)
                basep[bsa] = p.lens_cum.data_ptr()
                r, col = np.nonzero(W)                       # row-major: a cell's terms in ascending row order
                bl.append(bsa[r])
                pl.append(p.lens_cum.data_ptr() + col.astype(np.int64) * (p.lens_cum.stride(0) * 4))
                cl.append(W[r, col])
            b_all = np.concatenate(bl)
            order = np.argsort(b_all, kind="stable")
            b_s = b_all[order]
            cnt = np.bincount(b_s, minlength=B)
            T = max(1, int(cnt.max()) if cnt.size else 1)
            k = np.arange(b_s.size) - (np.cumsum(cnt) - cnt)[b_s]
            ptr = np.repeat(basep[:, None], T, axis=1)      # padding terms: a valid row with coefficient 0
            cf = np.zeros((B, T), np.float32)
            ptr[b_s, k] = np.concatenate(pl)[order]
            cf[b_s, k] = np.concatenate(cl)[order]
            return ops.row_combine(_h2d(ptr, self.dev).to(self.dev, non_blocking=True),
                                   _h2d(cf, self.dev).to(self.dev, non_blocking=True), base)
        dev_w = _h2d(np.concatenate(coefs), self.dev).to(self.dev, non_blocking=True)
        scatter = []
        for p, bs, n1, c in plan:
            w = dev_w[c: c + len(bs) * n1].view(len(bs), n1)
            if bs[-1] - bs[0] + 1 == len(bs):
                torch.mm(w, p.lens_cum, out=base[bs[0]: bs[-1] + 1])
            else:
                scatter.append((bs, w @ p.lens_cum))
        for bs, acc in scatter:              # (cells of a pair are contiguous in the sweep's batches)
            base.index_copy_(0, torch.as_tensor(bs, device=self.dev), acc)
        return base

    @torch.no_grad()
    def _tf_pass(self, cell_pairs: Sequence[Pair], hooks) -> dict:
        """Blocks after the hooked layer over response positions ``f..E`` of every cell (packed rows,
        fed the baseline residuals; edit + capture hooks at the hooked layer).  Returns per-row greedy
        token, its NLL and the NLL of the baseline's next token, and per cell ``(f, E, first row)``."""
        return self._tf_finish(self._tf_launch(cell_pairs, hooks))

    def _tf_finish(self, res: dict) -> dict:
        """Host side of a launched teacher-forced tail: wait for its one D2H copy, split it."""
        pend = res.pop("_pending", None)
        if pend is not None:
            flat, ev, M = pend
            if ev is not None:
                ev.synchronize()
            host = flat[: 3 * M].view(3, M)
            res["nxt"] = host[0, :M].view(torch.int32).numpy()
            res["nll_self"] = host[1, :M].numpy()
            res["nll_tgt"] = host[2, :M].numpy()
            ct = res.pop("_comp", None)
            if ct is not None:               # component trace: the hook's flat output buffer rides at the very end
                n_ct = ComponentHook.out_numel(*ct)
                res["comp"] = tuple(t.numpy() for t in ComponentHook.split(flat[flat.numel() - n_ct:], *ct))
                flat = flat[: flat.numel() - n_ct]
            mv = res.pop("_movers", None)
            if mv is not None:               # output movers: the compact [Ms, ...] outputs ride behind the trace, the
                Ms, Km, Tm = mv              # ids as int32 bits (as the ranks do)
                blk = flat[flat.numel() - Ms * (1 + 4 * Km + Tm):]
                cut = np.cumsum([0, Ms, Ms * Km, Ms * Km, Ms * Km, Ms * Km, Ms * Tm])
                part = [blk[cut[j]: cut[j + 1]] for j in range(6)]
                res["movers"] = {"tv": part[0].numpy(), "up_id": part[1].view(torch.int32).view(Ms, Km).numpy(),
                                 "up_dp": part[2].view(Ms, Km).numpy(),
                                 "dn_id": part[3].view(torch.int32).view(Ms, Km).numpy(),
                                 "dn_dp": part[4].view(Ms, Km).numpy(), "dp_track": part[5].view(Ms, Tm).numpy()}
                flat = flat[: flat.numel() - blk.numel()]
            tr = res.pop("_trace", None)
            if tr is not None:               # layer trace: [Lt, M, T] lens logits ride behind everything else
                res["trace"] = flat[flat.numel() - tr[0] * M * tr[1]:].view(tr[0], M, tr[1]).numpy()
                flat = flat[: flat.numel() - tr[0] * M * tr[1]]
            if res.pop("_shift", False):     # output shift: the rows' two KLs ride at the buffer's end
                res["kl"] = flat[flat.numel() - 2 * M: flat.numel() - M].numpy()
                res["kl_rev"] = flat[flat.numel() - M:].numpy()
                flat = flat[: flat.numel() - 2 * M]
            if flat.numel() > 3 * M:         # output readout: [M, K] log-probs, then [M, K] ranks (int32 bits)
                K = (flat.numel() - 3 * M) // (2 * M)
                res["logp"] = flat[3 * M: 3 * M + M * K].view(M, K).numpy()
                res["rank"] = flat[3 * M + M * K:].view(torch.int32).view(M, K).numpy()
        return res

    @torch.no_grad()
    def _tf_launch(self, cell_pairs: Sequence[Pair], hooks, f_cell: Optional[np.ndarray] = None) -> dict:
        """Enqueue the teacher-forced tail (no host sync): host index arrays, the packed forward, the vocab
        head, and one async D2H copy of its per-row outputs; :meth:`_tf_finish` waits for it.  ``f_cell[b]``:
        cell ``b``'s effective first edit (``_effective_first_edit``; -1 = its pair's first spike)."""
        from ..models.gemma2 import packed_blocks

        m = self.m
        nc = len(cell_pairs)
        uniq: Dict[int, int] = {}
        srcs, ulist = [], []
        off = 0
        f_a = np.zeros(nc, np.int64)
        E_a = np.zeros(nc, np.int64)
        base_a = np.zeros(nc, np.int64)      # row offset of the pair's residuals in the concatenation
        plen_a = np.zeros(nc, np.int64)
        up_a = np.zeros(nc, np.int64)        # unique-pair index
        for b, p in enumerate(cell_pairs):
            n, G = len(p.resp), len(p.gen_toks)
            fc = int(f_cell[b]) if f_cell is not None and b < len(f_cell) else -1
            f_a[b] = min(p.first_edit, max(n - 1, 0)) if fc < 0 else min(fc, n)
            E_a[b] = min(max([G - 2] + list(p.spikes_rel)), n - 1)
            u = uniq.get(id(p))
            if u is None:
                u = uniq[id(p)] = len(ulist)
                ulist.append((p, off))
                srcs.append(p.resid)
                off += p.resid.shape[0]
            up_a[b], base_a[b], plen_a[b] = u, ulist[u][1], p.plen
        Ls = np.maximum(E_a - f_a + 1, 0)
        r0_a = np.concatenate([[0], np.cumsum(Ls)[:-1]]) if nc else np.zeros(0, np.int64)
        seg = [(int(f_a[b]), int(E_a[b]), int(r0_a[b])) for b in range(nc)]
        M = int(Ls.sum())
        rb_ = np.repeat(np.arange(nc), Ls)                      # cell of every row
        t_ = (np.arange(M) - np.repeat(r0_a, Ls)) + np.repeat(f_a, Ls) if M else np.zeros(0, np.int64)
        Gmax = max((len(p.gen_toks) for p, _ in ulist), default=1)
        gtab = np.full((max(1, len(ulist)), Gmax + 1), -1, np.int64)
        for u, (p, _) in enumerate(ulist):
            gtab[u, : len(p.gen_toks)] = p.gen_toks
        pos = (plen_a[rb_] + t_).astype(np.int32)
        slot = rb_.astype(np.int32)
        tgt = gtab[up_a[rb_], t_ + 1].astype(np.int32)
        src = base_a[rb_] + t_
        self.stats["tf_rows"] += M
        self._tick("tf_host_prep")
        res = {"seg": seg, "nxt": np.zeros(0, np.int32), "nll_self": np.zeros(0, np.float32),
               "nll_tgt": np.zeros(0, np.float32), "row_cell": rb_, "row_t": t_, "tgt": tgt,
               "f": f_a, "E": E_a, "r0": r0_a, "up": up_a, "upairs": [p for p, _ in ulist], "gtab": gtab}
        trace = self.layer_trace
        movers = self.output_movers
        first_cell = {}                      # per unique pair: a cell slot of the running batch
        for b in range(nc - 1, -1, -1) if (trace or self.output_shift or movers) else ():
            first_cell[int(up_a[b])] = b
        mv_rows: List[int] = []              # output movers: the tail rows right behind an edited spike, cell by cell
        mv_m0 = np.zeros(nc, np.int64)
        if movers:
            for b, p in enumerate(cell_pairs):
                mv_m0[b] = len(mv_rows)
                f, E, r0 = seg[b]
                if E >= f:
                    mv_rows.extend(r0 + t - f for t in p.spikes_rel if f <= t < len(p.resp))
            res["mv_m0"] = mv_m0
            # the compact outputs are kept in tail-row order (a head sub-chunk's selected rows are then one slice);
            # entry j of the cell-by-cell list lives at mv_at[j]
            mv_g = np.asarray(mv_rows, np.int64)
            mv_ord = np.argsort(mv_g, kind="stable")
            res["mv_at"] = np.argsort(mv_ord, kind="stable")
            mv_g = mv_g[mv_ord]
        comp = self.component_trace
        if comp and not first_cell:
            for b in range(nc - 1, -1, -1):
                first_cell[int(up_a[b])] = b
        ct_rows: List[int] = []              # component trace: the tail rows at and right behind an edited spike
        if comp:
            ct_i0, ct_ts = np.zeros(nc, np.int64), []
            for b, p in enumerate(cell_pairs):
                ct_i0[b] = len(ct_rows)
                f, E, r0 = seg[b]
                hi = min(E, len(p.resp) - 1)
                ts = sorted({u for t in p.spikes_rel if f <= t <= hi for u in (t, t + 1) if u <= hi})
                ct_ts.append(np.asarray(ts, np.int64))
                ct_rows.extend(r0 + t - f for t in ts)
            res["ct_i0"], res["ct_ts"] = ct_i0, ct_ts
        if M == 0:
            if trace or comp:                # no cell has a tail row: the records still report the baseline's side
                self._shift_base([p for p, _ in ulist], [first_cell[u] for u in range(len(ulist))], sync=True)
            return res
        dev = self.dev
        up_ = lambda a: _h2d(a, dev).to(dev, non_blocking=True)     # noqa: E731  (pinned: no stream drain)
        H = torch.cat(srcs, 0) if len(srcs) > 1 else srcs[0]
        src_d = up_(src)
        pos_d = up_(pos)
        slot_d = up_(slot)
        tgt_d = up_(tgt)
        # [greedy id bits, NLL self, NLL target], then with the output readout the rows' tracked log-probs and ranks:
        # one buffer, one D2H copy
        Kt = self._track_cols()
        shift = self.output_shift
        Lt, Tt = (m.spec.layers - self.layer, self._n_trace) if trace else (0, 0)
        n_tr = Lt * M * Tt                   # layer trace: [Lt, M, Tt] lens logits behind the KLs
        # output movers: tv [Ms], four [Ms, Km] lists and dp_track [Ms, Tm] behind everything else
        Ms, Km, Tm = (len(mv_rows), self.movers_k, getattr(self, "_n_movers", 0)) if movers else (0, 0, 0)
        n_mv = Ms * (1 + 4 * Km + Tm)
        # component trace: the hook's slabs over the selected rows at the very end
        ct_dims = (m.spec.layers - 1 - self.layer, len(ct_rows), 2, m.lspec.heads) if comp else None
        n_ct = ComponentHook.out_numel(*ct_dims) if comp else 0
        flat = torch.empty(3 * M + 2 * M * Kt + (2 * M if shift else 0) + n_tr + n_mv + n_ct, dtype=torch.float32,
                           device=dev)
        end = flat.numel() - n_mv - n_ct     # where the layer trace ends
        outs = flat[: 3 * M].view(3, M)
        nxt, ns, nt = outs[0].view(torch.int32), outs[1], outs[2]
        ro = None
        if Kt:
            # tail row t's logits are the distribution that chooses response token t + 1.  The [U, K] id table goes
            # up once per launch; every row picks its pair's ids by its pair-table index
            ttab = np.full((max(1, len(ulist)), Kt), -1, np.int32)
            for u, (p, _) in enumerate(ulist):
                ttab[u, : len(p.track)] = np.asarray(p.track)[p.ro_order()]
            ro = (up_(ttab).index_select(0, up_(up_a[rb_])), flat[3 * M: 3 * M + M * Kt].view(M, Kt),
                  flat[3 * M + M * Kt: 3 * M + 2 * M * Kt].view(torch.int32).view(M, Kt))
        rpb = 16 // max(1, m.lspec.heads // m.lspec.kv_heads)
        cap = TAIL_CHUNK_ROWS
        # vocab-head rows per GEMM: 256-row multiples (GEMM tiles) of at most HEAD_LOGITS_BYTES of bf16 logits
        # (4096 rows of the 256k vocab)
        step = max(256, (HEAD_LOGITS_BYTES // (m.spec.vocab_size * 2)) // 256 * 256)
        if getattr(m, "fused_head", False):
            # the fused head keeps no logits (16 B of partials per 128 vocab columns): whole chunks per GEMM
            step = 16384
        # chunks of whole cells (a cell never spans two chunks), so chunks are independent and
        # alternate between two streams: one chunk's bandwidth-bound kernels (attention, norms, GeGLU,
        # vocab head) overlap the other's GEMMs
        chunks, cur, c_lo, c_rows = [], [], 0, 0
        for b, (f, E, r0) in enumerate(seg):
            if E < f:
                continue
            Ln = E - f + 1
            if cur and c_rows + Ln > cap:
                chunks.append((c_lo, c_lo + c_rows, cur))
                cur, c_lo, c_rows = [], r0, 0
            if not cur:
                c_lo = r0
            cur.append((r0 - c_lo, Ln, b, cell_pairs[b].kv_slot, int(plen_a[b] + f)) if self.tf_prefix
                       else (r0 - c_lo, Ln, b))
            c_rows += Ln
        if cur:
            chunks.append((c_lo, c_lo + c_rows, cur))
        main = torch.cuda.current_stream(dev) if dev.type == "cuda" else None
        streams = [main]
        ws_rows = min(cap, -(-M // 256) * 256)
        # every chunk's attention block table in one upload (no host sync between chunks)
        tabs = [packed_blocks(chunk, rpb) for (_, _, chunk) in chunks]
        tab_off = np.concatenate([[0], np.cumsum([t.shape[0] for t in tabs])]).astype(np.int64)
        tab_d = _h2d(torch.cat(tabs, 0), dev).to(dev, non_blocking=True) if tabs else None
        # reconstruct mode: the tail's hooked-layer rows are the pairs' baseline residuals (H), whose activations
        # at the spikes were encoded once per pair -- the edit hook splices from that table, no encode per cell
        splice = [hk for hk in hooks.get(self.layer, ()) if isinstance(hk, EditHook) and hk.sae is not None and
                  hk.plan.mode == "reconstruct"]
        if splice:
            acts_tab, offs = self._splice_table([p for p, _ in ulist])
            tb = np.full(int(splice[0].plan.spikes.shape[0]), -1, np.int32)
            tb[:nc] = np.asarray(offs, np.int32)[up_a]
            tb_d = up_(tb)
            for hk in splice:
                hk.use_table(acts_tab, tb_d)
        sh = tr = ct = None
        if shift or trace or movers or comp:
            # the pairs' unedited pass of blocks l+1..: the baseline side of the output shift, of the output movers and
            # of the layer trace
            Xb = self._shift_base([p for p, _ in ulist], [first_cell[u] for u in range(len(ulist))])
        if trace:
            # layer trace: one table block per pair of the launch, every tail row reads its pair's; the hook sits at
            # blocks l .. layers - 1 of the tail's packed pass, at block l behind the edit hook
            tr = TraceHook(self._trace_table([p for p, _ in ulist]), up_(up_a[rb_].astype(np.int32)),
                           flat[end - n_tr: end].view(Lt, M, Tt), self.layer, m.spec.eps,
                           float(m.spec.final_softcap or 0.0))
            hooks = {l: list(hooks.get(l, ())) + ([tr] if l in tr.layers else []) for l in set(hooks) | set(tr.layers)}
            self.stats["trace_rows"] = self.stats.get("trace_rows", 0) + Lt * M
            res["_trace"] = (Lt, Tt)
        if comp:
            # component trace: one table block per pair of the launch; the hook sits at block l behind the edit hook,
            # inside every later block and at the last block, and reads the selected rows alone
            sel = np.asarray(ct_rows, np.int32)
            A_, F_, V_ = self._comp_table([p for p, _ in ulist])
            ct = ComponentHook(A_, F_, V_, up_(sel), up_(up_a[rb_[sel]].astype(np.int32)), self.layer, m.lspec.heads,
                               m.spec.eps, out=flat[flat.numel() - n_ct:], sel_host=ct_rows)
            hooks = {l: list(hooks.get(l, ())) + ([ct] if l in (ct.first, ct.last) else [])
                     for l in set(hooks) | {ct.first, ct.last}}
            self.stats["comp_rows"] = self.stats.get("comp_rows", 0) + len(ct_rows)
            res["_comp"] = ct_dims
        if shift or movers:
            # output shift / movers: tail row (cell, t) is compared with its pair's unedited row t.  ``src`` already
            # names that row in the concatenation of the pairs' rows; per head sub-chunk the distinct baseline rows and
            # the rows' indices into them go up once, for the whole launch.  Movers alone: only the sub-chunks that hold
            # a selected row need their baseline rows
            kl_end = end - n_tr
            ub, rmap, uoff, moff = [], np.zeros(M, np.int32), {}, {}
            n_u = 0
            mv_loc = np.zeros(Ms, np.int32)  # a selected row's index inside its head sub-chunk
            for (c0, c1, _chunk) in chunks:
                for q0 in range(0, c1 - c0, step):
                    a, e = c0 + q0, min(c1, c0 + q0 + step)
                    if movers:
                        m0, m1 = (int(x) for x in np.searchsorted(mv_g, [a, e]))
                        moff[a] = (m0, m1)
                        mv_loc[m0:m1] = mv_g[m0:m1] - a
                        if not shift and m1 == m0:
                            continue
                    u, inv = np.unique(src[a:e], return_inverse=True)
                    ub.append(u)
                    rmap[a:e] = inv.reshape(-1)
                    uoff[a] = (n_u, n_u + u.size)
                    n_u += u.size
            sh = {"x": Xb, "ub": up_(np.concatenate(ub).astype(np.int64)) if ub else None, "map": up_(rmap),
                  "off": uoff}
            if shift:
                self.stats["shift_base_rows"] = self.stats.get("shift_base_rows", 0) + n_u
                sh.update({"kl": flat[kl_end - 2 * M: kl_end - M], "kl_rev": flat[kl_end - M: kl_end]})
                res["_shift"] = True
            if movers:
                # the selected rows and their pairs' tracked ids (Pair.track order, -1 padded) go up once as well
                itab = np.full((max(1, len(ulist)), max(1, Tm)), -1, np.int32)
                for u, (p, _) in enumerate(ulist):
                    itab[u, : len(p.track)] = p.track
                cut = np.cumsum([end, Ms, Ms * Km, Ms * Km, Ms * Km, Ms * Km, Ms * Tm])
                part = [flat[cut[j]: cut[j + 1]] for j in range(6)]
                sh["mv"] = {"off": moff, "rows": up_(mv_loc), "k": Km,
                            "ids": up_(itab[up_a[rb_[mv_g]]][:, :Tm].copy()) if Tm and Ms else None,
                            "out": (part[0], part[1].view(torch.int32).view(Ms, Km), part[2].view(Ms, Km),
                                    part[3].view(torch.int32).view(Ms, Km), part[4].view(Ms, Km),
                                    part[5].view(Ms, Tm))}
                self.stats["movers_rows"] = self.stats.get("movers_rows", 0) + Ms
                res["_movers"] = (Ms, Km, Tm)
        try:
            self._tf_chunks(chunks, streams, tab_d, tab_off, pos_d, slot_d, tgt_d, src_d, H, ws_rows, step, hooks,
                            nxt, ns, nt, ro, sh, tr, ct)
        finally:
            for hk in splice:
                hk.use_table(None)
        if len(streams) > 1:
            main.wait_stream(streams[1])
        if dev.type == "cuda":
            host = torch.empty(flat.shape, dtype=torch.float32, pin_memory=True)
            host.copy_(flat, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
        else:
            host, ev = flat, None
        res["_pending"] = (host, ev, M)
        self._tick("tf_launched")
        return res

    def _tf_chunks(self, chunks, streams, tab_d, tab_off, pos_d, slot_d, tgt_d, src_d, H, ws_rows, step, hooks,
                   nxt, ns, nt, ro=None, sh=None, tr=None, ct=None) -> None:
        """The packed forwards + vocab heads of :meth:`_tf_launch`, chunk by chunk.  ``ro`` (output readout): the rows'
        tracked ids ``[M, K]`` and the ``[M, K]`` log-prob / rank outputs of the tracking head.  ``sh`` (output
        shift): the pairs' unedited final-normed rows, per head sub-chunk its distinct baseline rows and the rows'
        indices into them, and the ``[M]`` KL outputs.  ``tr`` (layer trace): the launch's trace hook, already listed
        in ``hooks``; it is told every chunk's row window.  ``ct`` (component trace): likewise, and listed as the
        sub-hook of every later block."""
        m, dev = self.m, self.dev
        extra = {"sub_hooks": {l: [ct.sub] for l in ct.layers}} if ct is not None else {}

        def shift_rows(lg, a, e):
            # the sub-chunk's distinct baseline rows through the same unembedding (whole 256-row tiles), then one pass
            # over each edited row and its baseline row
            if a not in sh["off"]:               # movers alone, and no selected row in this sub-chunk
                return
            u0, u1 = sh["off"][a]
            nu = u1 - u0
            xb = torch.empty(-(-nu // 256) * 256, sh["x"].shape[1], dtype=sh["x"].dtype, device=dev)
            ops.row_gather(sh["x"], sh["ub"][u0:u1], xb)
            xb[nu:].zero_()
            lb = m.logits(xb)[:nu]
            if "kl" in sh:
                ops.head_shift(lg, lb, sh["map"][a:e], m.spec.final_softcap, sh["kl"][a:e], sh["kl_rev"][a:e])
            mv = sh.get("mv")
            if mv is not None and mv["off"][a][1] > mv["off"][a][0]:
                m0, m1 = mv["off"][a]
                ops.head_movers(lg, lb, sh["map"][a:e], mv["rows"][m0:m1], m.spec.final_softcap, mv["k"],
                                None if mv["ids"] is None else mv["ids"][m0:m1], *(o[m0:m1] for o in mv["out"]))

        for ci, (c0, c1, chunk) in enumerate(chunks):
            st = streams[ci % len(streams)]
            with (torch.cuda.stream(st) if st is not None else _nullctx()):
                Mc = c1 - c0
                Mp = -(-Mc // 256) * 256
                blk = tab_d[int(tab_off[ci]):int(tab_off[ci + 1])]
                cp = torch.full((Mp,), -1, dtype=torch.int32, device=dev)
                cs = torch.zeros(Mp, dtype=torch.int32, device=dev)
                cp[:Mc], cs[:Mc] = pos_d[c0:c1], slot_d[c0:c1]
                ws = self._nll_ws(ws_rows, key=ci % len(streams)).rows(Mp)
                # the chunk's input residuals straight into the workspace's residual buffer (forward_packed then
                # skips its own copy); only the padding rows are zeroed
                hin = ws.h
                ops.row_gather(H, src_d[c0:c1], hin)
                if Mp > Mc:
                    hin[Mc:].zero_()
                if tr is not None:
                    tr.use_rows(c0, c1, Mp)
                if ct is not None:
                    ct.use_rows(c0, c1, Mp)
                x = m.forward_packed(None, cp, cs, blk, self.gen.cache, hooks, ws=ws, resume_after=self.layer,
                                     h_in=hin, prefix_kv=self.pair_kv if self.tf_prefix else None, **extra)
                for q0 in range(0, Mc, step):
                    q1 = min(Mc, q0 + step)
                    if getattr(m, "head_path", False):
                        m.head(x[q0:q1], m.spec.final_softcap, tgt_d[c0 + q0:c0 + q1], nxt[c0 + q0:c0 + q1],
                               ns[c0 + q0:c0 + q1], nt[c0 + q0:c0 + q1])
                        continue
                    # the unembedding runs on whole 256-row tiles (padding rows of x included) so the
                    # GEMM shapes stay few and tuned; only the real rows are read out
                    lg = m.logits(x[q0:min(Mp, q0 + step)])[: q1 - q0]
                    if ro is not None:
                        ops.decode_head_track(lg, m.spec.final_softcap, ro[0][c0 + q0:c0 + q1], self._n_rank,
                                              tgt_d[c0 + q0:c0 + q1], nxt[c0 + q0:c0 + q1], ns[c0 + q0:c0 + q1],
                                              nt[c0 + q0:c0 + q1], ro[1][c0 + q0:c0 + q1], ro[2][c0 + q0:c0 + q1])
                    else:
                        ops.decode_head(lg, m.spec.final_softcap, tgt_d[c0 + q0:c0 + q1], nxt[c0 + q0:c0 + q1],
                                        ns[c0 + q0:c0 + q1], nt[c0 + q0:c0 + q1])
                    if sh is not None:
                        shift_rows(lg, c0 + q0, c0 + q1)

    @torch.no_grad()
    def _shift_base(self, upairs: Sequence[Pair], slots: Sequence[int], sync: bool = False) -> Optional[torch.Tensor]:
        """Output shift: the unedited final-normed rows of ``upairs``, concatenated in their order (``[sum n, D]``, the
        row layout of the concatenated ``Pair.resid``).  A pair's rows come from one packed pass of blocks ``l+1..``
        over its kept hooked-layer rows with no edit hook -- the teacher-forced tail's own path, so in the
        batch-invariant GEMM mode a tail row that no edit touched repeats its baseline row bit for bit -- and are
        kept on the pair (``Pair.x_base``, the size of ``Pair.resid``) for its later batches.  The pass writes the
        K/V of blocks ``l+1..`` at the response positions of ``slots[u]``, a cell slot of pair ``u`` in the running
        batch: the tail rewrites what it reads of them, and the decode reads the positions below a cell's first
        edit from the pair's own K/V.

        Layer trace: the same pass carries the tail's trace hook at blocks ``l .. layers - 1`` and keeps the pair's
        ``[n, Lt, T]`` lens logits on the host (``Pair.z_base``, a few KB; their copy is asynchronous on the GPU and
        finished by the time the launch's own D2H event has passed, or on return with ``sync``).  With the trace
        alone the final-normed rows are not kept and nothing is returned; with the output shift alone the pass is
        what it was."""
        from ..models.gemma2 import packed_blocks

        m, dev = self.m, self.dev
        # (the output movers use the output shift's baseline side: the kept final-normed rows)
        shift, trace, comp = self.output_shift or self.output_movers, self.layer_trace, self.component_trace
        stale = lambda v, p: v is None or v[0] is not p.resid      # noqa: E731
        need = [(p, s) for p, s in zip(upairs, slots)
                if ((shift and stale(p.x_base, p)) or (trace and stale(p.z_base, p))
                    or (comp and stale(p.c_base, p))) and p.resid.shape[0]]
        if comp:
            cdim = lambda k: (m.spec.layers - 1 - self.layer, k, 2, m.lspec.heads)      # noqa: E731
            for p in upairs:                 # an empty response has no selected rows
                if not p.resid.shape[0] and stale(p.c_base, p):
                    p.c_base = (p.resid, np.zeros(0, np.int64)) + tuple(
                        t.numpy() for t in ComponentHook.split(torch.zeros(0), *cdim(0)))
        if trace:
            Lt, Tt = m.spec.layers - self.layer, self._n_trace
            for p in upairs:                 # an empty response has an empty trace
                if not p.resid.shape[0] and stale(p.z_base, p):
                    p.z_base = (p.resid, torch.zeros(0, Lt, Tt))
        rpb = 16 // max(1, m.lspec.heads // m.lspec.kv_heads)
        i = 0
        while i < len(need):
            grp, rows = [], 0
            while i < len(need) and (not grp or rows + need[i][0].resid.shape[0] <= TAIL_CHUNK_ROWS):
                grp.append(need[i])
                rows += need[i][0].resid.shape[0]
                i += 1
            Mp = -(-rows // 256) * 256
            seqs, pos, slot, r0 = [], np.full(Mp, -1, np.int32), np.zeros(Mp, np.int32), 0
            for p, s in grp:
                n = p.resid.shape[0]
                seqs.append((r0, n, s, p.kv_slot, p.plen) if self.tf_prefix else (r0, n, s))
                pos[r0:r0 + n] = p.plen + np.arange(n)
                slot[r0:r0 + n] = s
                r0 += n
            ws = self._nll_ws(Mp, key=0).rows(Mp)
            hin = ws.h
            hin[:rows].copy_(torch.cat([p.resid for p, _ in grp], 0) if len(grp) > 1 else grp[0][0].resid)
            if Mp > rows:
                hin[rows:].zero_()
            hooks = tr = None
            if trace:
                vrow = np.repeat(np.arange(len(grp), dtype=np.int32), [p.resid.shape[0] for p, _ in grp])
                tr = TraceHook(self._trace_table([p for p, _ in grp]), _h2d(vrow, dev).to(dev, non_blocking=True),
                               torch.empty(Lt, rows, Tt, dtype=torch.float32, device=dev), self.layer, m.spec.eps,
                               float(m.spec.final_softcap or 0.0))
                tr.use_rows(0, rows, Mp)
                hooks = {l: [tr] for l in tr.layers}
            ct, extra = None, {}
            if comp:
                # component trace: every spike of a pair and the row behind it, for all the pair's cells
                tsel, r0 = [], 0
                for p, _ in grp:
                    n = p.resid.shape[0]
                    tsel.append(np.asarray(sorted({u for t in p.spikes_rel if t < n for u in (t, t + 1) if u < n}),
                                           np.int64))
                    r0 += n
                offs = np.concatenate([[0], np.cumsum([p.resid.shape[0] for p, _ in grp])])
                sel = np.concatenate([t + offs[j] for j, t in enumerate(tsel)]).astype(np.int32)
                sblk = np.repeat(np.arange(len(grp), dtype=np.int32), [len(t) for t in tsel])
                A_, F_, V_ = self._comp_table([p for p, _ in grp])
                ct = ComponentHook(A_, F_, V_, _h2d(sel, dev).to(dev, non_blocking=True),
                                   _h2d(sblk, dev).to(dev, non_blocking=True), self.layer, m.lspec.heads, m.spec.eps,
                                   sel_host=sel.tolist())
                ct.use_rows(0, rows, Mp)
                hooks = {l: list((hooks or {}).get(l, ())) + ([ct] if l in (ct.first, ct.last) else [])
                         for l in set(hooks or {}) | {ct.first, ct.last}}
                extra = {"sub_hooks": {l: [ct.sub] for l in ct.layers}}
            x = m.forward_packed(None, _h2d(pos, dev).to(dev, non_blocking=True),
                                 _h2d(slot, dev).to(dev, non_blocking=True),
                                 _h2d(packed_blocks(seqs, rpb), dev).to(dev, non_blocking=True), self.gen.cache, hooks,
                                 ws=ws, resume_after=self.layer, h_in=hin,
                                 prefix_kv=self.pair_kv if self.tf_prefix else None, **extra)
            if comp:
                if dev.type == "cuda":
                    ch = torch.empty(ct.out.shape, dtype=torch.float32, pin_memory=True)
                    ch.copy_(ct.out, non_blocking=True)
                else:
                    ch = ct.out
                parts = ComponentHook.split(ch, *cdim(len(sel)))         # views of the host copy, sliced per pair
                i0 = 0
                for (p, _), ts in zip(grp, tsel):
                    i1 = i0 + len(ts)
                    p.c_base = (p.resid, ts, parts[0][:, i0:i1], parts[1][i0:i1], parts[2][i0:i1], parts[3][i0:i1])
                    i0 = i1
                self.stats["comp_base_rows"] = self.stats.get("comp_base_rows", 0) + len(sel)
            xs = x[:rows].clone() if shift else None
            zs = None
            if trace:
                zd = tr.out.permute(1, 0, 2).contiguous()                 # [rows, Lt, Tt]
                if dev.type == "cuda":
                    zs = torch.empty(zd.shape, dtype=torch.float32, pin_memory=True)
                    zs.copy_(zd, non_blocking=True)
                else:
                    zs = zd
                self.stats["trace_base_rows"] = self.stats.get("trace_base_rows", 0) + Lt * rows
            r0 = 0
            for p, _ in grp:
                n = p.resid.shape[0]
                if shift:
                    p.x_base = (p.resid, xs[r0:r0 + n])
                if trace:
                    p.z_base = (p.resid, zs[r0:r0 + n])
                r0 += n
            if shift:
                self.stats["shift_base_pass_rows"] = self.stats.get("shift_base_pass_rows", 0) + rows
        if (trace or comp) and sync and dev.type == "cuda":
            torch.cuda.current_stream(dev).synchronize()
        if not shift:
            return None
        parts = [p.x_base[1] if p.resid.shape[0] else p.resid.new_zeros(0, self.D) for p in upairs]
        return torch.cat(parts, 0) if len(parts) > 1 else parts[0]

    @staticmethod
    def _shift_fields(p: Pair, f: int, r0: int, kl: Optional[np.ndarray], kl_rev: Optional[np.ndarray]) -> dict:
        """Record fields of the output shift for a cell whose teacher-forced tail starts at response index ``f`` (row
        ``r0`` of ``kl`` / ``kl_rev``; tail row ``t`` holds the KL between the baseline's and the cell's distribution
        over token ``t + 1``, both after the baseline's tokens ``0..t``).  ``kl_out_mean`` / ``kl_rev_out_mean`` run
        over the positions of the cell's ``nll_edit`` -- the ``n`` response tokens, of which the first ``f + 1`` are
        chosen before the first edit and shift by exactly 0 -- and ``kl_out_max`` over the same; ``kl_out_spike_mean``
        over the pair's spikes ``t`` (row ``t``, the row right behind the edit; spikes before ``f`` were no-op edits:
        0).  The sums are exactly rounded (``math.fsum``), so a cell's fields do not depend on where its rows lie in
        the tail or on leading zero rows."""
        import math

        n = len(p.resp)
        ntail = max(0, n - 1 - f)
        rows = kl[r0: r0 + ntail] if kl is not None else np.zeros(0, np.float32)
        rrev = kl_rev[r0: r0 + ntail] if kl_rev is not None else np.zeros(0, np.float32)
        sp = [t for t in p.spikes_rel if t < n]
        hit = [float(kl[r0 + t - f]) for t in sp if t >= f] if kl is not None else []
        return {"kl_out_mean": math.fsum(rows.tolist()) / n if n else 0.0,
                "kl_out_max": max([0.0] + rows.tolist()),
                "kl_out_spike_mean": math.fsum(hit) / len(sp) if sp else 0.0,
                "kl_rev_out_mean": math.fsum(rrev.tolist()) / n if n else 0.0}

    @staticmethod
    def _movers_fields(p: Pair, f: int, m0: int, at: np.ndarray, mv: Optional[dict], donor: Optional[Pair]) -> dict:
        """Record fields of the output movers for a cell whose teacher-forced tail starts at response index ``f``.
        The cell's selected rows -- tail row ``t`` for each of its pair's spikes ``t >= f``, the rows
        ``kl_out_spike_mean`` reads -- are entries ``m0, m0 + 1, ...`` of the launch's cell-by-cell list, entry ``j``
        at index ``at[j]`` of the compact outputs ``mv``.  A spike before ``f`` was a no-op edit: total variation
        exactly 0 and empty lists, not computed, and counted in the denominators as ``kl_out_spike_mean`` counts it.
        ``movers_up`` / ``movers_dn``: per spike ``[[id, dp], ...]``; ``tv_out_spike_mean``: the mean total variation;
        ``movers_up_share`` / ``movers_dn_share``: the mean over the spikes with ``tv > 0`` of the listed gain / loss
        over ``tv`` (1: all the moved mass went to / came from the listed tokens; NaN without such a spike);
        ``secret_loss_share``: over the same spikes, the larger loss of the secret's two forms over ``tv``;
        ``secret_in_losers`` / ``decoy_in_gainers`` / ``donor_in_gainers`` (swap cells): the share of spikes whose
        list holds a secret form / a decoy / the donor's secret; ``top_gainer``: the id with the largest summed gain
        (the lower id on ties, -1 if none).  Sums are exactly rounded (``math.fsum``)."""
        import math

        n = len(p.resp)
        sp = [t for t in p.spikes_rel if t < n]
        nan = float("nan")
        ups, dns, tvs, up_sh, dn_sh, sec_sh = [], [], [], [], [], []
        secret = {int(t) for t in p.track[:2]}
        decoys = {int(t) for t in p.track[2: 2 + p.n_decoys]}
        dsec = int(donor.track[0]) if donor is not None else None
        in_dn = in_up = in_don = 0
        gain: Dict[int, List[float]] = {}
        j = 0
        for t in sp:
            if t < f or mv is None:
                ups.append([])
                dns.append([])
                tvs.append(0.0)
                continue
            i = int(at[m0 + j])
            j += 1
            up = [[int(c), float(v)] for c, v in zip(mv["up_id"][i], mv["up_dp"][i]) if c >= 0]
            dn = [[int(c), float(v)] for c, v in zip(mv["dn_id"][i], mv["dn_dp"][i]) if c >= 0]
            tv = float(mv["tv"][i])
            ups.append(up)
            dns.append(dn)
            tvs.append(tv)
            if tv > 0.0:
                up_sh.append(math.fsum(v for _, v in up) / tv)
                dn_sh.append(-math.fsum(v for _, v in dn) / tv)
                forms = [float(x) for x in mv["dp_track"][i][:2]]
                sec_sh.append(max(0.0, -min(forms)) / tv if forms else 0.0)
            in_dn += any(c in secret for c, _ in dn)
            in_up += any(c in decoys for c, _ in up)
            in_don += dsec is not None and any(c == dsec for c, _ in up)
            for c, v in up:
                gain.setdefault(c, []).append(v)
        tot = {c: math.fsum(v) for c, v in gain.items()}
        mean = lambda xs: math.fsum(xs) / len(xs) if xs else nan       # noqa: E731
        out = {"movers_up": ups, "movers_dn": dns,
               "tv_out_spike_mean": math.fsum(tvs) / len(sp) if sp else 0.0,
               "movers_up_share": mean(up_sh), "movers_dn_share": mean(dn_sh), "secret_loss_share": mean(sec_sh),
               "secret_in_losers": in_dn / len(sp) if sp else 0.0, "decoy_in_gainers": in_up / len(sp) if sp else 0.0,
               "top_gainer": min(tot, key=lambda c: (-tot[c], c)) if tot else -1}
        if donor is not None:
            out["donor_in_gainers"] = in_don / len(sp) if sp else 0.0
        return out

    def _comp_table(self, upairs: Sequence[Pair]):
        """Component trace: the launch's tables ``A [Lc, U, 2, heads * head_dim]``, ``F [Lc, U, 2, D]`` and
        ``Vd [U, 2, D]`` (``interp.edits.component_tables``), one block per pair: column 0 is the pair's secret (the
        trace's column 0), column 1 its donor word's secret for a pair with swap cells and a zero row otherwise.  A
        pair's block is built once per runner, in fp64 and rounded once, so its bits never depend on which pairs share
        its launch."""
        cache = self.__dict__.setdefault("_comp_blocks", {})
        out = []
        for p in upairs:
            dw = getattr(self, "_pair_donor", {}).get(id(p))
            ids = [int(p.track[0])] + ([int(p.track[p.extra[dw]])] if dw is not None and dw in p.extra else [])
            blk = cache.get(tuple(ids))
            if blk is None:
                blk = cache[tuple(ids)] = tuple(t.to(self.dev) for t in component_tables(self.m, self.layer, ids, 2))
            out.append(blk)
        return (torch.stack([b[0] for b in out], 1).contiguous(), torch.stack([b[1] for b in out], 1).contiguous(),
                torch.stack([b[2] for b in out], 0).contiguous())

    def _comp_base(self, p: Pair, sp: List[int]) -> dict:
        """The baseline side of a pair's component fields in logit units, computed once per pair from ``Pair.c_base``:
        the row of every selected response index, the float64 slabs over the pair's own ``rho_f`` and the
        ``comp_base_spike`` matrix."""
        import math

        cb = p.c_base
        if len(cb) == 7:
            return cb[6]
        _, bt, bcomp, bdir, btot, brho = cb
        H, Lc = self.m.lspec.heads, self.m.spec.layers - 1 - self.layer
        brf = np.asarray(brho, dtype=np.float64)
        k = len(bt)
        d = {"idx": {int(t): i for i, t in enumerate(bt.tolist())},
             "comp": (np.asarray(bcomp, dtype=np.float64) / brf[None, :, None, None] if k
                      else np.zeros((Lc, 0, 2, H + 1))),
             "direct": np.asarray(bdir, dtype=np.float64) / brf[:, None] if k else np.zeros((0, 2)),
             "total": np.asarray(btot, dtype=np.float64) if k else np.zeros((0, 2))}
        rows = [d["idx"][t] for t in sp]
        den = len(sp)
        d["spike"] = [[math.fsum(v) / den if den else 0.0 for v in blk]
                      for blk in d["comp"][:, rows, 0, :].transpose(0, 2, 1).tolist()]
        p.c_base = cb + (d,)
        return d

    def _comp_fields(self, p: Pair, i0: int, ts: np.ndarray, c: Optional[tuple], swap: bool) -> dict:
        """Record fields of the component trace for a cell whose selected tail rows are response indices ``ts`` (its
        spikes ``t >=`` its first effective edit and the rows ``t + 1`` inside its tail), rows ``i0 ..`` of the
        launch's slabs ``c = (comp [Lc, Ms, 2, heads + 1], direct, total, rho_f)``.  Everything is in logit units:
        the edited run over its own ``rho_f``, the pair's unedited pass (``Pair.c_base``) over its own, and the
        difference of the two taken here in float64, so a row no edit reached differs by exactly 0.  ``Lc`` is blocks
        ``l + 1 .. layers - 1``, the components ``h0 .. h{heads-1}``, then ``mlp``.  ``comp_dz_spike`` /
        ``comp_dz_next`` are means over the pair's spikes of the edited row itself and of the row right behind it (spikes before the
        first effective edit, and rows outside the tail, contribute 0; the denominator is the pair's spike count, as
        for ``trace_dz_spike`` and ``kl_out_spike_mean``); ``comp_base_spike`` is the baseline's own value;
        ``comp_attn_dz_spike`` / ``comp_mlp_dz_spike`` the heads' sum and the MLP per block;
        ``comp_direct_dz_spike`` / ``comp_total_dz_spike`` the direct term at block ``l`` and ``z_pre`` of the last
        block, so ``direct + sum(comp_dz_spike)`` can be checked against the total; ``comp_top_spike`` the largest
        ``|comp_dz_spike|`` as ``[block, name, value]``; swap cells also get ``comp_dz_donor_spike`` (column 1).  The
        sums are exactly rounded (``math.fsum``)."""
        import math

        H = self.m.lspec.heads
        Lc = self.m.spec.layers - 1 - self.layer
        n = len(p.resp)
        sp = [t for t in p.spikes_rel if t < n]
        den = len(sp)
        base = self._comp_base(p, sp)
        bidx, bc, bd, bz = base["idx"], base["comp"], base["direct"], base["total"]
        k = len(ts)
        tl = ts.tolist()
        if k and c is not None:
            rf = np.asarray(c[3][i0:i0 + k], dtype=np.float64)
            ec = np.asarray(c[0][:, i0:i0 + k], dtype=np.float64) / rf[None, :, None, None]
            ed = np.asarray(c[1][i0:i0 + k], dtype=np.float64) / rf[:, None]
            ez = np.asarray(c[2][i0:i0 + k], dtype=np.float64)
            at = [bidx[t] for t in tl]
            dc, dd, dz = ec - bc[:, at], ed - bd[at], ez - bz[at]
        else:
            dc, dd, dz = np.zeros((Lc, 0, 2, H + 1)), np.zeros((0, 2)), np.zeros((0, 2))
        eidx = {t: i for i, t in enumerate(tl)}
        # the tail's selected rows start at its first effective spike: every spike among them is an edited one
        hit = [eidx[t] for t in sp if t in eidx]
        nxt = [eidx[t + 1] for t in sp if t in eidx and t + 1 in eidx]
        mean = lambda v: math.fsum(v) / den if den else 0.0        # noqa: E731
        # [Lc][heads + 1] of exactly rounded sums over the listed rows (one transposed copy, then plain lists)
        mat = lambda a, rows, col: [[mean(v) for v in blk]          # noqa: E731
                                    for blk in a[:, rows, col, :].transpose(0, 2, 1).tolist()]
        out = {"comp_dz_spike": mat(dc, hit, 0), "comp_dz_next": mat(dc, nxt, 0),
               "comp_base_spike": base["spike"],
               "comp_direct_dz_spike": mean(dd[hit, 0].tolist()), "comp_total_dz_spike": mean(dz[hit, 0].tolist())}
        out["comp_attn_dz_spike"] = [math.fsum(r[:H]) for r in out["comp_dz_spike"]]
        out["comp_mlp_dz_spike"] = [r[H] for r in out["comp_dz_spike"]]
        names = [f"h{j}" for j in range(H)] + ["mlp"]
        top = max(((abs(v), -kk, -j) for kk, r in enumerate(out["comp_dz_spike"]) for j, v in enumerate(r)),
                  default=(0.0, 0, 0))
        kk, j = -top[1], -top[2]
        out["comp_top_spike"] = [self.layer + 1 + kk, names[j], out["comp_dz_spike"][kk][j] if Lc else 0.0]
        if swap:
            out["comp_dz_donor_spike"] = mat(dc, hit, 1)
        return out

    def _trace_table(self, upairs: Sequence[Pair]) -> torch.Tensor:
        """Layer trace: the ``[U, T, D]`` fp32 table of lens directions, one block per pair, its columns in
        ``Pair.track`` order (``T`` = the run's widest track list; columns a pair does not have, and ids outside the
        vocabulary, are zero rows, which read out as exactly 0).  Each row is ``lens_direction`` of that single id; a
        pair's block is built once per runner."""
        from ..interp.gradient import lens_direction

        T = self._n_trace
        cache = self.__dict__.setdefault("_trace_blocks", {})
        V = self.m.spec.vocab_size
        out = []
        for p in upairs:
            key = tuple(int(t) for t in p.track)
            blk = cache.get(key)
            if blk is None or blk.shape[0] != T:
                blk = torch.zeros(T, self.D, dtype=torch.float32, device=self.dev)
                for j, t in enumerate(key):
                    if 0 <= t < V:
                        blk[j] = lens_direction(self.m, [t]).to(self.dev)
                cache[key] = blk
            out.append(blk)
        return torch.stack(out, 0).contiguous()

    def _trace_fields(self, p: Pair, f: int, E: int, r0: int, z: Optional[np.ndarray],
                      donor: Optional[Pair] = None) -> dict:
        """Record fields of the layer trace for a cell whose teacher-forced tail holds response rows ``f..E`` from row
        ``r0`` of ``z [Lt, M, T]`` (the capped lens logit of the pair's tracked ids at blocks ``l .. layers - 1``;
        column 0 is the secret).  Every field but ``trace_recovery`` is a list over those blocks.  ``dz`` is the plain
        difference ``z_edit - z_base`` of the two fp32 values against the pair's unedited pass (``Pair.z_base``), so a
        row no edit reached differs by exactly 0; rows before ``f`` are the baseline's and are not computed.
        ``trace_dz_spike`` / ``trace_z_base_spike`` / ``trace_decoy_dz_spike`` / ``trace_dz_donor_spike`` (swap cells:
        the donor's secret) are means over the pair's spikes ``t`` of row ``t`` itself, the row the edit is written to
        (spikes before ``f`` were no-op edits: 0); ``trace_dz_mean`` runs over the rows of the cell's ``nll_edit``
        (``f .. n - 2``) with its denominator ``n``.  ``trace_recovery = 1 - trace_dz_spike[-1] / trace_dz_spike[0]``
        is the share of the direct effect that the later blocks undo (nan where there is no direct effect).  The sums
        are exactly rounded (``math.fsum``)."""
        import math

        Lt = self.m.spec.layers - self.layer
        n = len(p.resp)
        zb = p.z_base[1].numpy() if p.z_base is not None else np.zeros((0, Lt, len(p.track)), np.float32)
        Ln = max(0, min(E, n - 1) - f + 1) if z is not None else 0
        # dz[k, i, col]: block l + k, response row f + i
        dz = (z[:, r0:r0 + Ln].astype(np.float64) - zb[f:f + Ln].transpose(1, 0, 2).astype(np.float64)
              if Ln else np.zeros((Lt, 0, zb.shape[2])))
        sp = [t for t in p.spikes_rel if t < n]
        hit = [t - f for t in sp if f <= t < f + Ln]
        ntail = min(max(0, n - 1 - f), Ln)
        # per block: an exactly rounded sum over the listed values (one list per block), over a fixed denominator
        mean = lambda rows, den: [math.fsum(v) / den if den else 0.0 for v in rows.tolist()]      # noqa: E731
        nd = p.n_decoys
        dzs = dz[:, hit, :]                                                  # [Lt, spikes at or past f, T]
        out = {"trace_dz_spike": mean(dzs[:, :, 0], len(sp)),
               "trace_dz_mean": mean(dz[:, :ntail, 0], n),
               "trace_z_base_spike": mean(zb[sp, :, 0].T.astype(np.float64), len(sp)),
               "trace_decoy_dz_spike": mean(dzs[:, :, 2:2 + nd].reshape(Lt, len(hit) * nd), len(sp) * nd)}
        if donor is not None:
            out["trace_dz_donor_spike"] = mean(dzs[:, :, p.extra.get(donor.word, 0)], len(sp))
        d0, d1 = out["trace_dz_spike"][0], out["trace_dz_spike"][-1]
        out["trace_recovery"] = 1.0 - d1 / d0 if d0 != 0.0 else float("nan")
        return out

    def _cell_result(self, c: Cell, p: Pair, n_gen: int, resp: List[int], probs: np.ndarray, topk_ids: List[int],
                     nll_edit: float, nll_self: float, ro=None) -> dict:
        ps = probs[:, 0] if probs.shape[0] else np.zeros(0, dtype=np.float32)
        stats = (float(ps.mean()), float(ps[-1]), float(ps.max())) if ps.size else (0.0, 0.0, 0.0)
        dec = [float(x) for x in probs[:, 2: 2 + p.n_decoys].mean(0)] if probs.shape[0] else []
        q = self._run_pairs[c.donor] if c.donor >= 0 else None
        return self._cell_record(c, p, n_gen, resp, stats, dec, topk_ids, nll_edit, nll_self, q,
                                 probs[:, p.extra.get(q.word, 0)] if q is not None else None, ro=ro)

    def _cell_record(self, c: Cell, p: Pair, n_gen: int, resp: List[int], stats: Tuple[float, float, float],
                     decoy: List[float], topk_ids: List[int], nll_edit: float, nll_self: float,
                     donor: Optional[Pair] = None, p_donor: Optional[np.ndarray] = None, ro=None) -> dict:
        """``donor`` / ``p_donor`` (swap cells only): the donor pair and the lens probability of its secret (space
        form) over the cell's response.  ``ro`` (output readout only): the cell's ``(logp, rank) [n_gen, K]`` table."""
        dc = self._dec_cache
        guesses = []
        for t in topk_ids:
            g = dc.get(t)
            if g is None:
                g = dc[t] = self.tok.decode([t]).strip()
            guesses.append(g)
        if resp is p.resp or resp == p.resp:     # unchanged response: the baseline's leak verdict
            if p.leak is None:
                p.leak = contains_secret(self.tok.decode(p.resp), p.forms)
            leak = p.leak
        else:
            leak = contains_secret(self.tok.decode(resp), p.forms)
        if p.p_secret_mean is None:
            p.p_secret_mean = float(p.p_secret.mean()) if p.p_secret is not None and p.p_secret.size else 0.0
            p.forms_l = {f.lower() for f in p.forms}
        rec = {
            "word": p.word, "prompt_idx": p.pidx, "method": c.method, "budget": c.budget, "trial": c.trial,
            "seed": c.seed, "n_gen": n_gen, "spikes": p.spikes_rel,
            "p_secret_mean": stats[0], "p_secret_final": stats[1], "p_secret_max": stats[2],
            "p_secret_mean_base": p.p_secret_mean,
            "topk_ids": topk_ids, "guesses": guesses,
            "secret_in_topk": any(g.lower() in p.forms_l for g in guesses),
            "decoy_probs": decoy,
            "leak": leak,
            "nll_edit": nll_edit, "nll_base": p.nll, "delta_nll": nll_edit - p.nll,
            "nll_self": nll_self,
            "response_ids": resp,
        }
        if c.method in NOISE_METHODS:            # norm-matched controls only: the other records keep their keys
            rec["edit_norm"] = p.edit_norm[1][(c.method, c.budget)]
        if c.method in SWAP_METHODS:             # interchange cells only: what became of the donor's secret
            q, col = donor, p.extra.get(donor.word, 0)        # next_prompt: the donor's secret is the pair's own
            pd = np.asarray(p_donor, dtype=np.float32)
            base = float(p.track_probs[:, col].mean()) if p.track_probs is not None and p.track_probs.shape[0] else 0.0
            mean = float(pd.mean()) if pd.size else 0.0
            rec.update({
                "donor_word": q.word, "donor_prompt_idx": q.pidx,
                "p_donor_mean": mean, "p_donor_final": float(pd[-1]) if pd.size else 0.0,
                "p_donor_max": float(pd.max()) if pd.size else 0.0,
                "delta_p_donor": mean - base,       # against the target pair's own baseline
                "donor_leak": contains_secret(self.tok.decode(resp), q.forms),
                "donor_in_topk": int(q.track[0]) in [int(t) for t in topk_ids],
            })
        if ro is not None:                       # output readout only: the other runs keep their keys
            n = len(p.resp)
            base = self._out_fields(p, p.out_logp[:n], p.out_rank[:n], donor if c.method in SWAP_METHODS else None)
            f = self._out_fields(p, ro[0][:n_gen], ro[1][:n_gen], donor if c.method in SWAP_METHODS else None)
            f["delta_logp_out"] = f["logp_out_mean"] - base["logp_out_mean"]
            f["logp_out_mean_base"] = base["logp_out_mean"]
            if "logp_out_donor_mean" in f:
                f["delta_logp_out_donor"] = f["logp_out_donor_mean"] - base["logp_out_donor_mean"]
            rec.update(f)
        return rec

    def _nll_ws(self, M: int, key: int = 0):
        """Workspace for the ragged passes (one per stream ``key``), grown in 4096-row steps and sliced
        per chunk."""
        pool = self.__dict__.setdefault("_nll_wsp", {})
        ws = pool.get(key)
        if ws is None or ws.M < M:
            from ..models.gemma2 import _Workspace

            pool.pop(key, None)
            ws = pool[key] = self.m.new_workspace(-(-M // 4096) * 4096)
        return ws

    @torch.no_grad()
    def _nll_cells(self, cell_pairs: Sequence[Pair], plan_hook: EditHook, out, c0s: Sequence[int]) -> List[float]:
        """Mean NLL of each cell's *baseline* hint under the edit (teacher forced, EP:136).

        The edited decode already scored the baseline's token at every column (``out.tf_nll``); those
        are the teacher-forced NLLs up to the column ``d`` where the cell's own greedy tokens leave the
        baseline's (:func:`teacher_divergence`).  Targets before the decode's first column ``c0`` are
        the baseline's own NLLs (identical prefix), and only targets after ``d`` need a teacher-forced
        pass: a ragged (packed, unpadded) forward over positions ``plen+d .. plen+n-2`` in the cell's
        own KV slot, whose prefix ``< plen+d`` holds exactly the baseline tokens."""
        from ..models.gemma2 import packed_blocks
        from ..runtime.generation import teacher_divergence

        m = self.m
        nc = len(cell_pairs)
        tfn = out.tf_nll[:nc].float().cpu().numpy()
        own = out.tokens[:nc].cpu().numpy()
        sums = [0.0] * nc
        ids, pos, tgt, owner, seqs = [], [], [], [], []
        for b, p in enumerate(cell_pairs):
            n = len(p.resp)
            if not n:
                continue
            c0 = c0s[b]
            tot = float(np.sum(p.tok_nll[: min(c0, n)]))
            d = teacher_divergence(own[b].tolist(), p.resp, c0)
            hi = min(d, n - 1)
            if hi >= c0:
                tot += float(np.sum(tfn[b, c0: hi + 1]))
            sums[b] = tot
            if d < n - 1:
                L = n - 1 - d
                seqs.append((len(ids), L, b))
                ids += p.resp[d: n - 1]
                pos += range(p.plen + d, p.plen + n - 1)
                tgt += p.resp[d + 1: n]
                owner += [b] * L
        self.nll_rows = getattr(self, "nll_rows", 0) + len(ids)
        if ids:
            rpb = 16 // max(1, m.lspec.heads // m.lspec.kv_heads)
            cap = TAIL_CHUNK_ROWS
            dev = self.dev
            nll = torch.empty(len(ids), device=dev)
            ids_d = torch.tensor(ids, dtype=torch.int32, device=dev)
            pos_d = torch.tensor(pos, dtype=torch.int32, device=dev)
            slot_d = torch.tensor(owner, dtype=torch.int32, device=dev)
            tgt_d = torch.tensor(tgt, dtype=torch.int32, device=dev)
            step = max(256, (HEAD_LOGITS_BYTES // (m.spec.vocab_size * 2)) // 256 * 256)
            for r0 in range(0, len(ids), cap):
                r1 = min(len(ids), r0 + cap)
                M = r1 - r0
                Mp = -(-M // 256) * 256                 # few distinct GEMM shapes
                chunk = []
                for (s0, L, b) in seqs:                  # sequences clipped to this chunk
                    a0, a1 = max(s0, r0), min(s0 + L, r1)
                    if a1 > a0:
                        chunk.append((a0 - r0, a1 - a0, b))
                blk = packed_blocks(chunk, rpb).to(dev)
                ci = torch.zeros(Mp, dtype=torch.int32, device=dev)
                cp = torch.full((Mp,), -1, dtype=torch.int32, device=dev)
                cs = torch.zeros(Mp, dtype=torch.int32, device=dev)
                ci[:M], cp[:M], cs[:M] = ids_d[r0:r1], pos_d[r0:r1], slot_d[r0:r1]
                ws = self._nll_ws(min(cap, -(-len(ids) // 256) * 256)).rows(Mp)
                x = m.forward_packed(ci, cp, cs, blk, self.gen.cache, {self.layer: [plan_hook]}, ws=ws)
                for q0 in range(0, M, step):
                    q1 = min(M, q0 + step)
                    if getattr(m, "head_path", False):
                        m.head(x[q0:q1], m.spec.final_softcap, tgt_d[r0 + q0: r0 + q1],
                               nll_tgt=nll[r0 + q0: r0 + q1])
                        continue
                    lg = m.logits(x[q0:q1])
                    ops.xent_rows(lg, tgt_d[r0 + q0: r0 + q1], m.spec.final_softcap, True,
                                  out=nll[r0 + q0: r0 + q1])
            extra = torch.zeros(nc, device=dev).index_add_(0, slot_d.long(), nll).cpu().tolist()
            sums = [a + e for a, e in zip(sums, extra)]
        return [sums[b] / len(p.resp) if p.resp else float("nan") for b, p in enumerate(cell_pairs)]
