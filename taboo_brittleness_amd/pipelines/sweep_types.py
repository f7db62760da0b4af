"""Data types and small helpers shared by the sweep modules (:mod:`.sweep`, :mod:`.sweep_plan`,
:mod:`.sweep_decode`, :mod:`.sweep_readout`): a (word, prompt) pair with its baseline artifacts, a cell (one
intervention setting), a decode-tail carry record, the prefetched next batch, pinned host -> device staging."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

METHODS = ("sae_targeted", "sae_random", "proj_targeted", "proj_random")
# reconstruct mode only (intervention.ablation_mode): the pure splice -- the residual replaced by the SAE's
# reconstruction with nothing ablated (budget 0, one cell per pair), the control that separates "the SAE error was
# dropped" from "these latents were removed"
SPLICE_METHOD = "sae_splice"
# norm-matched controls (opt-in, never part of METHODS): the cell of ``sae_targeted`` / ``proj_targeted`` at the same
# budget / rank, whose residual moves exactly as far at the same positions but along a seeded random direction
# (ops.matched_noise_edit); ``intervention.noise_trials`` cells per budget / rank
NOISE_METHODS = ("sae_noise", "proj_noise")
# interchange (donor-swap) interventions (opt-in, never part of METHODS): at the pair's spikes the selected latents
# (``sae_swap``: the target's and the donor's targeted latents; ``sae_swap_random``: random active ones) or subspace
# coordinates (``proj_swap``: the basis pooled over all pairs; ``proj_swap_random``: a random one) take the values they
# have in a donor pair's residuals (ops.interchange_edit); the donor is chosen by ``intervention.swap_donor``
SWAP_METHODS = ("sae_swap", "sae_swap_random", "proj_swap", "proj_swap_random")
SWAP_DONORS = ("next_word", "next_prompt")


def check_swap_donor(rule: str) -> str:
    if rule not in SWAP_DONORS:
        raise ValueError(f"intervention.swap_donor must be one of {', '.join(SWAP_DONORS)}, not {rule!r}")
    return rule


@dataclass
class Pair:
    word: str
    pidx: int
    prompt: str
    ids: List[int]
    forms: List[str]
    track: List[int]                       # [secret(space), secret(bare), decoys...]
    resp: List[int] = field(default_factory=list)
    p_secret: Optional[np.ndarray] = None  # [n_resp] lens prob of the secret (space form) at the hooked layer
    spikes_rel: List[int] = field(default_factory=list)
    top_ids: List[int] = field(default_factory=list)
    resid: Optional[torch.Tensor] = None   # [n_resp, D] hooked-layer residuals (device)
    nll: float = float("nan")
    targeted: List[int] = field(default_factory=list)
    active_pool: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))  # sorted, unique
    gen_toks: List[int] = field(default_factory=list)   # generated tokens incl. the stop token (if any)
    tok_nll: Optional[np.ndarray] = None                # per generated token NLL under the unedited model
    kv_slot: int = -1                                   # slot in the runner's pair-KV store
    lens_cum: Optional[torch.Tensor] = None             # [n_resp + 1, V] running lens sums (layer resume)
    track_probs: Optional[np.ndarray] = None            # [n_resp, K] lens probs of the tracked ids
    leak: Optional[bool] = None                         # baseline response contains the secret (cached)
    p_secret_mean: Optional[float] = None               # cached mean of p_secret (result records)
    forms_l: Optional[set] = None
    rep: int = 0                                        # replicate of this (word, prompt): seeds its random cells
    # exact per-latent activity at the edited spikes (SweepRunner._spike_activity): sorted candidate latent
    # ids and, per id, a bitmask over spikes_rel[:K] of where the edit kernel's own JumpReLU fires
    act_ids: Optional[np.ndarray] = None
    act_mask: Optional[np.ndarray] = None
    act_key: Optional[tuple] = None                     # SAE parameter identity/versions the table was built with
    # reconstruct mode: SAE activations [len(spikes_rel[:K]), d_sae] of the baseline residuals at the spikes (the
    # rows the teacher-forced tail splices), and the SAE parameter key they were encoded under
    splice_acts: Optional[torch.Tensor] = None
    splice_key: Optional[tuple] = None
    # intervention.latent_score = effect_lens | attr_model only: the score values of ``targeted`` (same order), the
    # correlational ranking of the same pair (reported as the overlap of the two top lists) and, for attr_model, the
    # spike gradients with the baseline they were taken from (one backward pass per baseline)
    targeted_scores: Optional[List[float]] = None
    targeted_corr: Optional[List[int]] = None
    score_grads: Optional[tuple] = None
    # norm-matched controls only: (the baseline residuals the figures were taken from, {(method, budget): mean over
    # the spikes of |targeted delta|_2 / |h|_2}) -- SweepRunner._edit_norms
    edit_norm: Optional[tuple] = None
    # swap methods only: word -> column of ``track`` holding that other word's secret id (space form), appended after
    # the decoys (SweepRunner.build_pairs); the decoy readouts stop before these columns
    extra: Dict[str, int] = field(default_factory=dict)
    # intervention.output_readout only: [len(gen_toks), K] next-token log-prob / rank of ``track`` under the
    # distribution that chose each generated token (index 0: the prefill's last prompt row), from the baseline's decode
    out_logp: Optional[np.ndarray] = None
    out_rank: Optional[np.ndarray] = None
    # intervention.output_shift / output_movers only: (the ``resid`` they were computed from, [n, D] final-normed rows
    # of the unedited blocks past the hooked layer over ``resid``) -- the baseline side of the cells' KL and of their
    # movers (ReadoutMixin._shift_base)
    x_base: Optional[tuple] = None
    # intervention.layer_trace only: (the ``resid`` they were computed from, [n, Lt, T] fp32 host tensor: the capped lens
    # logits of ``track`` at blocks l .. layers - 1 of the same unedited pass) -- the baseline side of the cells'
    # ``trace_*`` fields (ReadoutMixin._shift_base)
    z_base: Optional[tuple] = None
    # intervention.component_trace only: (the ``resid`` they were computed from, the selected response rows ``t``
    # [k] -- every spike and the row behind it -- and the host copies ``comp [Lc, k, T, heads + 1]``, ``direct [k, T]``,
    # ``total [k, T]``, ``rho_f [k]`` of the same unedited pass) -- the baseline side of the cells' ``comp_*`` fields
    # (ReadoutMixin._shift_base)
    c_base: Optional[tuple] = None

    def ro_order(self) -> List[int]:
        """Column order of ``track`` in the tracking head's id table (output readout): the secret's two forms, the
        other words' secrets, then the decoys -- the head ranks a leading block of columns, and a swap donor's secret
        must be inside it while the decoys need not.  Table column ``j`` holds ``track[ro_order()[j]]``;
        ``np.argsort`` of it maps a table back to ``track`` order (``table[..., inv]``)."""
        ex = sorted(self.extra.values())
        return list(range(min(2, len(self.track)))) + ex + [j for j in range(2, len(self.track)) if j not in ex]

    @property
    def n_decoys(self) -> int:
        return len(self.track) - 2 - len(self.extra)

    @property
    def first_edit(self) -> int:
        """Response index of the first edited position (last token if there is nothing to edit)."""
        if self.spikes_rel:
            return min(self.spikes_rel)
        return max(len(self.resp) - 1, 0)

    @property
    def plen(self) -> int:
        return len(self.ids)

    @property
    def spikes_abs(self) -> List[int]:
        return [self.plen + i for i in self.spikes_rel]


@dataclass
class Cell:
    pair: int
    method: str
    budget: int
    trial: int
    seed: int
    donor: int = -1                        # swap methods: index of the donor pair among the call's pairs

    @property
    def kind(self) -> str:
        return "sae" if self.method.startswith("sae") else "proj"


@dataclass
class _Carry:
    """A diverged cell whose decode continues in the next batch (decode-tail carry-over): its KV,
    capture-store row and edit-plan row live in the runner's carry region at ``slot``."""
    cell: Cell
    pair: Pair
    d: int                       # divergence point D
    nll: float                   # teacher-forced edit NLL of the baseline hint (already complete)
    slot: int
    tok: int                     # next token to feed, at position ``pos``
    pos: int
    prefix: List[int]            # response tokens so far (ends with ``tok``)
    prefix_nll: np.ndarray       # their NLLs
    steps: int                   # decode steps still needed
    pre: Tuple[int, int, int]    # (pair KV slot, len_lo, len_hi) of the shared prefix
    plan_row: Tuple[np.ndarray, int, np.ndarray, int, int]   # host (spikes, kind, idx, cnt, noise seed) of the slot


class NextBatch:
    """The next :meth:`SweepRunner.run_cells` batch, for :meth:`SweepRunner.stage_next`: its pairs, and
    either its ``(cells, plan)`` prefetch future, or ``cells`` (``plan`` built when staged).  Run the
    next call with ``nb.cells`` (the same list object) so the staged work is used."""

    def __init__(self, pairs, methods=METHODS, cells=None, plan=None, future=None):
        self.pairs, self.methods, self.cells, self.plan, self.future = pairs, methods, cells, plan, future

    def resolve(self, runner) -> None:
        if self.future is not None:
            self.cells, self.plan = self.future.result()
            self.future = None
        if self.cells is None:
            self.cells = runner.make_cells(self.pairs, self.methods)


def _h2d(a, dev):
    """Host array -> pinned CPU tensor for a non-blocking upload (plain tensor on CPU devices)."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.pin_memory() if dev.type == "cuda" else t


class _Deferred:
    """Result records of :meth:`SweepRunner.run_cells_async` (lists and/or futures, in cell order)."""

    def __init__(self, parts):
        self.parts = parts

    def result(self) -> List[dict]:
        out: List[dict] = []
        for p in self.parts:
            out += p.result() if hasattr(p, "result") else p
        return out


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
