"""Tiny end-to-end smoke of the flagship path (used by ``__graft_entry__.smoke``).

One hooked greedy decode with an SAE-latent ablation at the hooked layer,
then the logit-lens readout and a teacher-forced NLL — every step on the HIP
kernels when ``device`` is a GPU.
"""
from __future__ import annotations

import torch

from .config import Config
from .interp.sae import JumpReLUSAE
from .models.gemma2 import Gemma2Model
from .models.spec import get_spec
from .models.tokenizer import SyntheticTokenizer
from .models.weights import random_gemma2
from .pipelines.sweep import SweepRunner


def run_smoke(device, arch: str = "gemma2-tiny", max_new: int = 8) -> dict:
    spec = get_spec(arch)
    cfg = Config()
    cfg.experiment.max_new_tokens = max_new
    cfg.intervention.budgets = [1, 4]
    cfg.intervention.random_trials = 1
    cfg.intervention.ranks = [1, 2]
    cfg.intervention.proj_random_trials = 1
    w = random_gemma2(spec, device=device, seed=3)
    m = Gemma2Model(w, device)
    tok = SyntheticTokenizer(vocab_size=spec.vocab_size)
    sae = JumpReLUSAE.random(spec.hidden, 2048, seed=1, device=device)
    layer = spec.layers // 2
    r = SweepRunner(cfg, m, tok, sae, batch=16, device=device, layer=layer)
    pairs = r.build_pairs(["ship"], cfg.prompts[:2])
    r.run_baselines(pairs)
    sae.calibrate(torch.cat([p.resid for p in pairs], 0), target_l0=20)
    r._score_pairs(pairs)
    cells = r.make_cells(pairs)
    res = r.run_cells(pairs, cells)
    if device.type == "cuda":
        torch.cuda.synchronize()
    assert len(res) == len(cells) and all(x["n_gen"] >= 0 for x in res)
    return {"cells": len(res), "p_secret_mean": sum(x["p_secret_mean"] for x in res) / len(res),
            "delta_nll_finite": all(x["delta_nll"] == x["delta_nll"] for x in res),
            "movers_tv": _smoke_movers(device, spec.vocab_size, float(spec.final_softcap or 30.0))}


def _smoke_movers(device, V: int, cap: float) -> float:
    """One ``ops.head_movers`` call against ops/reference.py: an edited row with one logit raised (its column must
    head the gainers, the values within 1e-5 of the fp32 reference) and an untouched row (exact zeros)."""
    from . import ops
    from .ops import reference as ref

    g = torch.Generator().manual_seed(11)
    base = (4 * torch.randn(2, V, generator=g)).to(torch.bfloat16)
    logits = base.clone()
    col = V - 3
    logits[0, col] = base[0].float().max() + 2
    rm = torch.tensor([0, 1], dtype=torch.int32)
    rows = torch.tensor([1, 0], dtype=torch.int32)
    ids = torch.tensor([[col, -1], [col, 0]], dtype=torch.int32)
    want = ref.head_movers(logits, base, rm, rows, cap, 4, ids)
    got = [t.cpu() for t in ops.head_movers(logits.to(device), base.to(device), rm.to(device), rows.to(device), cap, 4,
                                            ids.to(device))]
    assert int(got[1][1, 0]) == col == int(want[1][1, 0]) and bool((got[1][1, 1:] == -1).all())
    assert not got[0][0] and bool((got[1][0] == -1).all()) and bool((got[3][0] == -1).all()) and not got[5][0].any()
    assert bool((got[3][1] >= 0).all()) and bool((got[4][1] < 0).all())
    for j in (0, 1, 2, 5):                   # tv, the gainers and the tracked differences; the losers may tie
        assert torch.allclose(got[j].float(), want[j].float(), atol=1e-5, rtol=0), (j, got[j], want[j])
    assert torch.allclose(got[4].sum(-1), want[4].sum(-1), atol=1e-5, rtol=0)
    assert got[5][1, 0] == got[2][1, 0]
    return float(got[0][1])
