"""Figures and tables of the write-up (EP:160, 182-184; reference `results/artifacts.md:7-11`):

* ``fig1_ablation_saes.png`` — SAE-ablation curves, targeted vs random, vs budget m
  (secret probability with 95% CI, LL-Top-k Pass@10, ΔNLL, leak rate);
* ``fig2_lowrank.png`` — the same for the low-rank projection vs rank r;
* ``fig3_content_vs_inhibition.png`` — Δ secret probability vs Δ inhibition
  (token-forcing success when measured, else leak rate), one point per setting;
* ``fig4_interchange.png`` — interchange (donor-swap) interventions, only for sweeps that ran them: the
  target's and the donor's secret probability vs budget / rank, targeted swap vs random swap;
* ``fig5_collateral.png`` — output shift (``intervention.output_shift``), only for sweeps run with it: the KL between
  the baseline's and the edited next-token distribution vs budget / rank, targeted against its controls; with the
  output readout also the specificity plane (Δ log-prob of the secret against that KL);
* ``fig8_components.png`` — component trace (``intervention.component_trace``), only for sweeps run with it: a heatmap
  of block × component (heads, then the MLP) of the change of each later component's direct contribution to the
  secret's lens logit, the targeted method at its largest budget beside its random control.
* ``fig6_layer_trace.png`` — layer trace (``intervention.layer_trace``), only for sweeps run with it: the change of the
  secret's capped lens logit at the edited rows against the block it is read at, one line per budget, targeted
  against its controls;
* ``fig7_movers.png`` — output movers (``intervention.output_movers``), only for sweeps run with it: the share of the
  moved probability that landed on the listed gainers and the share of it that the secret lost, vs budget / rank,
  targeted against its controls;
* ``table_baselines.csv`` — LL-Top-k / SAE-Top-k / token forcing rows with
  Pass@10, Majority@10, Accuracy.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional

import matplotlib

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402

from ..utils.io import atomic_write_text  # noqa: E402


def token_prob_heatmap(p_layers_tokens, tokens: List[str], path: str, plotting: Dict, title: str = "") -> None:
    """Secret-token probability, layers × response tokens (reference `src/plots.py:4-50`; LL heatmap,
    SURVEY C14 / P1).  ``plotting``: the reference's plotting config keys."""
    fig, ax = plt.subplots(figsize=tuple(plotting["figsize"]))
    plt.rcParams.update({"font.size": plotting["font_size"]})
    im = ax.imshow(p_layers_tokens, cmap=plotting["colormap"], aspect="auto", vmin=0, vmax=1,
                   interpolation="nearest")
    cb = fig.colorbar(im, ax=ax)
    cb.ax.tick_params(labelsize=plotting["tick_font_size"])
    ax.set_ylabel("Layers", fontsize=plotting["title_font_size"])
    ax.set_yticks(list(range(p_layers_tokens.shape[0]))[::4])
    ax.tick_params(axis="y", labelsize=plotting["tick_font_size"])
    if len(tokens):
        ax.set_xticks(list(range(len(tokens))))
        ax.set_xticklabels(list(tokens), rotation=75, ha="right", fontsize=plotting["font_size"])
    if title:
        ax.set_title(title, fontsize=plotting["title_font_size"])
    plt.tight_layout()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fig.savefig(path, bbox_inches="tight", dpi=plotting["dpi"])
    plt.close(fig)


def _heatmap_job(job) -> str:
    token_prob_heatmap(*job)
    return job[2]


def render_heatmaps(jobs: List[tuple], workers: Optional[int] = None) -> List[str]:
    """Render many heatmaps; large batches go to a spawned process pool (this module imports only
    matplotlib/numpy, so workers start without torch or the GPU runtime)."""
    workers = workers if workers is not None else min(8, os.cpu_count() or 1, len(jobs))
    if workers <= 1 or len(jobs) < 4:
        return [_heatmap_job(j) for j in jobs]
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor

    with ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(_heatmap_job, jobs))


def _curve(curves: List[Dict], method: str, key: str):
    pts = sorted((c["budget"], c) for c in curves if c["method"] == method)
    xs = [b for b, _ in pts]
    if not pts:
        return xs, [], [], []
    v = pts[0][1][key]
    if isinstance(v, dict):
        return xs, [c[key]["mean"] for _, c in pts], [c[key]["lo"] for _, c in pts], [c[key]["hi"] for _, c in pts]
    return xs, [c[key] for _, c in pts], None, None


def mode_label(summary: Dict) -> str:
    """``"clamp, c = 4"`` for a sweep file of the clamp / steer modes (their ``sae`` cells push the latents towards
    ``clamp_value``), ``""`` for the ablation modes."""
    if "clamp_value" not in summary:
        return ""
    return f"{summary.get('ablation_mode', '?')}, c = {summary['clamp_value']:g}"


def intervention_curves(summary: Dict, kind: str, path: str) -> None:
    curves = summary["curves"]
    tgt, rnd = f"{kind}_targeted", f"{kind}_random"
    series = [(tgt, "tab:red", tgt), (rnd, "tab:blue", rnd)]
    if any(c["method"] == f"{kind}_noise" for c in curves):       # the norm-matched control, when the sweep ran it
        series.append((f"{kind}_noise", "tab:green", f"{kind}_noise (norm-matched noise)"))
    panels = [("p_secret_mean", "LL secret prob @ hooked layer"), ("delta_nll", "ΔNLL of baseline hint"),
              ("leak_rate", "leak rate")]
    fig, axes = plt.subplots(1, len(panels) + 1, figsize=(5 * (len(panels) + 1), 4))
    for ax, (key, title) in zip(axes, panels):
        for meth, col, lab in series:
            xs, ys, lo, hi = _curve(curves, meth, key)
            if not xs:
                continue
            ax.plot(xs, ys, "o-", color=col, label=lab)
            if lo is not None:
                ax.fill_between(xs, lo, hi, color=col, alpha=0.2)
        if kind == "sae":
            # reconstruct mode: the pure splice (SAE reconstruction, nothing ablated) as a reference level
            _, ys, _, _ = _curve(curves, "sae_splice", key)
            if ys:
                ax.axhline(ys[0], color="0.4", ls="--", lw=1, label="sae_splice (nothing ablated)")
        ax.set_xscale("log", base=2)
        ax.set_title(title)
        ax.set_xlabel("budget m" if kind == "sae" else "rank r")
    ax = axes[-1]
    for meth, col, lab in series:
        pts = sorted((c["budget"], c.get("ll_topk", {}).get("any_pass", float("nan"))) for c in curves
                     if c["method"] == meth)
        if pts:
            ax.plot([p[0] for p in pts], [p[1] for p in pts], "o-", color=col, label=lab)
    ax.set_xscale("log", base=2)
    ax.set_title("LL-Top-k Pass@10")
    axes[0].legend()
    # the selector of the targeted latents, named when it is not the correlational default
    sel = (summary.get("config") or {}).get("latent_score", "corr")
    label = "; ".join(x for x in (mode_label(summary), f"targets ranked by {sel}" if sel != "corr" else "") if x)
    if kind == "sae" and label:
        fig.suptitle(f"SAE latents: {label}")
    plt.tight_layout()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fig.savefig(path, dpi=150)
    plt.close(fig)


def interchange_curves(summary: Dict, path: str) -> None:
    """Interchange interventions: the target's secret probability and the donor's against budget m (SAE latents) and
    rank r (subspace), the swap of the targeted set against the swap of a random one."""
    curves = summary["curves"]
    rows = [("sae", "budget m"), ("proj", "rank r")]
    panels = [("p_secret_mean", "target: LL secret prob"), ("p_donor_mean", "donor: LL secret prob"),
              ("delta_p_donor", "donor: Δ vs the target's baseline")]
    fig, axes = plt.subplots(len(rows), len(panels), figsize=(5 * len(panels), 4 * len(rows)), squeeze=False)
    for i, (kind, xlabel) in enumerate(rows):
        for ax, (key, title) in zip(axes[i], panels):
            for meth, col in ((f"{kind}_swap", "tab:red"), (f"{kind}_swap_random", "tab:blue")):
                xs, ys, lo, hi = _curve(curves, meth, key)
                if not xs:
                    continue
                ax.plot(xs, ys, "o-", color=col, label=meth)
                if lo is not None:
                    ax.fill_between(xs, lo, hi, color=col, alpha=0.2)
            ax.set_xscale("log", base=2)
            ax.set_title(title)
            ax.set_xlabel(xlabel)
        if axes[i][0].get_legend_handles_labels()[0]:
            axes[i][0].legend()
    donor = (summary.get("config") or {}).get("swap_donor")
    if donor:
        fig.suptitle(f"interchange interventions, donor: {donor}")
    plt.tight_layout()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fig.savefig(path, dpi=150)
    plt.close(fig)


def content_vs_inhibition(summary: Dict, path: str, forcing_delta: Optional[Dict] = None) -> None:
    fig, ax = plt.subplots(figsize=(6, 5))
    for c in summary["curves"]:
        x = c["delta_p_secret"]["mean"]
        key = (c["method"], c["budget"])
        y = forcing_delta.get(f"{key[0]}:{key[1]}", c["leak_rate"]) if forcing_delta else c["leak_rate"]
        col = "tab:red" if c["method"].endswith("targeted") else \
            "tab:green" if c["method"].endswith("noise") else "tab:blue"
        mk = "o" if c["method"].startswith("sae") else "s"
        ax.scatter([x], [y], color=col, marker=mk)
        ax.annotate(f"{c['method'].split('_')[0]}{c['budget']}", (x, y), fontsize=7)
    ax.axvline(0, color="k", lw=0.5)
    ax.axhline(0, color="k", lw=0.5)
    ax.set_xlabel("Δ LL secret probability (content)")
    ax.set_ylabel("Δ token-forcing success" if forcing_delta else "leak rate (inhibition failure)")
    if mode_label(summary):
        ax.set_title(f"sae cells: {mode_label(summary)}")
    plt.tight_layout()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fig.savefig(path, dpi=150)
    plt.close(fig)


def content_vs_output(summary: Dict, path: str) -> None:
    """Output-side readout (intervention.output_readout): what an edit does to the lens content at the hooked layer
    (Δ LL secret probability) against what it does to the model's own next-token log-prob of the secret
    (``delta_logp_out``), one point per (method, budget) with the 95 % bootstrap interval of the latter."""
    fig, ax = plt.subplots(figsize=(6, 5))
    for c in summary["curves"]:
        if "delta_logp_out" not in c:
            continue
        x, y = c["delta_p_secret"]["mean"], c["delta_logp_out"]
        col = "tab:red" if c["method"].endswith("targeted") else \
            "tab:green" if c["method"].endswith("noise") else "tab:purple" if "swap" in c["method"] else "tab:blue"
        mk = "o" if c["method"].startswith("sae") else "s"
        ax.errorbar([x], [y["mean"]], yerr=[[y["mean"] - y["lo"]], [y["hi"] - y["mean"]]], color=col, marker=mk,
                    capsize=2, lw=0.8)
        ax.annotate(f"{c['method'].split('_')[0]}{c['budget']}", (x, y["mean"]), fontsize=7)
    ax.axvline(0, color="k", lw=0.5)
    ax.axhline(0, color="k", lw=0.5)
    ax.set_xlabel("Δ LL secret probability at the hooked layer (content)")
    ax.set_ylabel("Δ next-token log-prob of the secret (output)")
    if mode_label(summary):
        ax.set_title(f"sae cells: {mode_label(summary)}")
    plt.tight_layout()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fig.savefig(path, dpi=150)
    plt.close(fig)


def _method_colour(method: str) -> str:
    return "tab:red" if method.endswith("targeted") else "tab:green" if method.endswith("noise") else \
        "tab:purple" if "swap" in method else "0.4" if method == "sae_splice" else "tab:blue"


def collateral_curves(summary: Dict, path: str) -> None:
    """Output shift (intervention.output_shift): ``kl_out_mean`` -- KL(baseline || edited) of the next-token
    distribution, averaged over the teacher-forced response -- against budget m (SAE methods) and rank r (subspace
    methods), every method the sweep ran (targeted against its random / noise / swap controls, the pure splice as a
    level), with 95 % bootstrap intervals.  With the output readout a further panel, the specificity plane: what the
    edit did to the secret's own log-prob (``delta_logp_out``) against what it did to the whole distribution."""
    curves = [c for c in summary["curves"] if "kl_out_mean" in c]
    plane = any("delta_logp_out" in c for c in curves)
    fig, axes = plt.subplots(1, 2 + int(plane), figsize=(5.5 * (2 + int(plane)), 4.2), squeeze=False)
    for ax, (kind, xlabel) in zip(axes[0], (("sae", "budget m"), ("proj", "rank r"))):
        for meth in sorted({c["method"] for c in curves if c["method"].startswith(kind + "_")}):
            xs, ys, lo, hi = _curve(curves, meth, "kl_out_mean")
            if meth == "sae_splice":
                ax.axhline(ys[0], color="0.4", ls="--", lw=1, label="sae_splice (nothing ablated)")
                continue
            ls = "o-" if meth.endswith("targeted") or meth.endswith("_swap") else "s--"
            ax.plot(xs, ys, ls, color=_method_colour(meth), label=meth, alpha=0.9)
            ax.fill_between(xs, lo, hi, color=_method_colour(meth), alpha=0.15)
        ax.set_xscale("log", base=2)
        ax.set_xlabel(xlabel)
        ax.set_ylabel("KL(baseline || edited), nats per response token")
        ax.set_title(f"collateral shift of the output distribution: {kind}")
        if ax.get_legend_handles_labels()[0]:
            ax.legend(fontsize=7)
    if plane:
        ax = axes[0][2]
        for c in curves:
            if "delta_logp_out" not in c:
                continue
            x, y = c["kl_out_mean"], c["delta_logp_out"]
            ax.errorbar([x["mean"]], [y["mean"]], xerr=[[x["mean"] - x["lo"]], [x["hi"] - x["mean"]]],
                        yerr=[[y["mean"] - y["lo"]], [y["hi"] - y["mean"]]], color=_method_colour(c["method"]),
                        marker="o" if c["method"].startswith("sae") else "s", capsize=2, lw=0.8)
            ax.annotate(f"{c['method'].split('_')[0]}{c['budget']}", (x["mean"], y["mean"]), fontsize=7)
        ax.axhline(0, color="k", lw=0.5)
        ax.set_xlabel("KL(baseline || edited) (everything)")
        ax.set_ylabel("Δ next-token log-prob of the secret (the target)")
        ax.set_title("specificity plane")
    if mode_label(summary):
        fig.suptitle(f"sae cells: {mode_label(summary)}")
    plt.tight_layout()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fig.savefig(path, dpi=150)
    plt.close(fig)


def layer_trace_curves(summary: Dict, path: str) -> None:
    """Layer trace (intervention.layer_trace): ``trace_dz_spike`` -- the change of the secret's capped logit-lens logit
    at the edited rows, edited minus baseline -- against the block it is read at, from the hooked layer (where the edit
    is written) to the last: one line per budget m (SAE methods) or rank r (subspace methods), the targeted method
    solid against its controls dashed, with 95 % bootstrap intervals.  A line that returns towards 0 is an edit the
    later blocks repair; the legend carries each line's ``trace_recovery``."""
    curves = [c for c in summary["curves"] if "trace_dz_spike" in c]
    blocks = summary.get("config", {}).get("trace_blocks") or list(range(len(curves[0]["trace_dz_spike"])))
    fig, axes = plt.subplots(1, 2, figsize=(11, 4.2), squeeze=False)
    for ax, kind in zip(axes[0], ("sae", "proj")):
        mine = [c for c in curves if c["method"].startswith(kind + "_")]
        buds = sorted({c["budget"] for c in mine})
        for c in sorted(mine, key=lambda c: (c["method"], c["budget"])):
            main = c["method"].endswith("targeted") or c["method"].endswith("_swap")
            ys = [ci["mean"] for ci in c["trace_dz_spike"]]
            shade = 0.35 + 0.65 * (buds.index(c["budget"]) + 1) / len(buds)
            rec = c["trace_recovery"]["mean"]
            ax.plot(blocks, ys, "o-" if main else "s--", color=_method_colour(c["method"]), alpha=shade, lw=1.2,
                    ms=3, label=f"{c['method']} {c['budget']}" + (f" (rec {rec:.2f})" if rec == rec else ""))
            ax.fill_between(blocks, [ci["lo"] for ci in c["trace_dz_spike"]], [ci["hi"] for ci in c["trace_dz_spike"]],
                            color=_method_colour(c["method"]), alpha=0.08)
        ax.axhline(0, color="k", lw=0.5)
        ax.set_xlabel("block")
        ax.set_ylabel("Δ capped lens logit of the secret at the spikes")
        ax.set_title(f"layer trace downstream of the edit: {kind}")
        if ax.get_legend_handles_labels()[0]:
            ax.legend(fontsize=6, ncol=2)
    if mode_label(summary):
        fig.suptitle(f"sae cells: {mode_label(summary)}")
    plt.tight_layout()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fig.savefig(path, dpi=150)
    plt.close(fig)


def movers_curves(summary: Dict, path: str) -> None:
    """Output movers (intervention.output_movers): ``movers_up_share`` -- the share of the total variation at the
    edited spikes that landed on the listed top gainers (near 1: a small competition of substitutes; near 0: a diffuse
    edit) -- and ``secret_loss_share`` -- the share of it that the secret's own forms lost -- against budget m (SAE
    methods, top row) and rank r (subspace methods, bottom row), targeted against its controls, with 95 % bootstrap
    intervals."""
    curves = [c for c in summary["curves"] if "movers_up_share" in c]
    fields = (("movers_up_share", "share of the moved mass on the listed gainers"),
              ("secret_loss_share", "share of the moved mass lost by the secret"))
    fig, axes = plt.subplots(2, 2, figsize=(11, 8), squeeze=False)
    for row, (kind, xlabel) in zip(axes, (("sae", "budget m"), ("proj", "rank r"))):
        for ax, (key, ylabel) in zip(row, fields):
            for meth in sorted({c["method"] for c in curves if c["method"].startswith(kind + "_")}):
                xs, ys, lo, hi = _curve(curves, meth, key)
                if meth == "sae_splice":
                    if ys and ys[0] == ys[0]:
                        ax.axhline(ys[0], color="0.4", ls="--", lw=1, label="sae_splice (nothing ablated)")
                    continue
                ls = "o-" if meth.endswith("targeted") or meth.endswith("_swap") else "s--"
                ax.plot(xs, ys, ls, color=_method_colour(meth), label=meth, alpha=0.9)
                ax.fill_between(xs, lo, hi, color=_method_colour(meth), alpha=0.15)
            ax.set_xscale("log", base=2)
            ax.set_ylim(-0.02, 1.02)
            ax.set_xlabel(xlabel)
            ax.set_ylabel(ylabel)
            ax.set_title(f"where the probability went: {kind}")
            if ax.get_legend_handles_labels()[0]:
                ax.legend(fontsize=7)
    k = summary.get("config", {}).get("movers_k")
    fig.suptitle(" | ".join(x for x in (f"top {k} gainers per spike" if k else "",
                                        f"sae cells: {mode_label(summary)}" if mode_label(summary) else "") if x))
    plt.tight_layout()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fig.savefig(path, dpi=150)
    plt.close(fig)


def component_heatmaps(summary: Dict, path: str) -> None:
    """Component trace (intervention.component_trace): the mean ``comp_dz_spike`` -- the change of each later
    component's direct contribution to the secret's lens logit at the edited rows, edited minus baseline -- as a
    heatmap of block x component (heads, then the MLP): per kind (SAE / subspace) the targeted method at its largest
    budget beside its random control at the same budget, on one symmetric colour scale.  One bright cell is one head
    re-writing the secret; an even wash is a distributed repair."""
    curves = [c for c in summary["curves"] if "comp_dz_spike" in c]
    cfg = summary.get("config", {})
    blocks = cfg.get("comp_blocks") or list(range(len(curves[0]["comp_dz_spike"])))
    names = cfg.get("comp_names") or [str(j) for j in range(len(curves[0]["comp_dz_spike"][0]))]
    panels = []
    for kind in ("sae", "proj"):
        tg = [c for c in curves if c["method"] in (f"{kind}_targeted", f"{kind}_swap")]
        if not tg:
            continue
        top = max(tg, key=lambda c: (c["budget"], c["method"].endswith("targeted")))
        panels.append(top)
        ctl = [c for c in curves if c["method"] == f"{kind}_random" and c["budget"] == top["budget"]]
        panels += ctl[:1]
    panels = panels or curves[:2]
    vmax = max((abs(v) for c in panels for row in c["comp_dz_spike"] for v in row), default=0.0) or 1.0
    fig, axes = plt.subplots(1, len(panels), figsize=(1.5 + 3.6 * len(panels), 1.6 + 0.28 * len(blocks)),
                             squeeze=False)
    im = None
    for ax, c in zip(axes[0], panels):
        im = ax.imshow(c["comp_dz_spike"], cmap="RdBu_r", vmin=-vmax, vmax=vmax, aspect="auto")
        ax.set_xticks(range(len(names)))
        ax.set_xticklabels(names, fontsize=6, rotation=90)
        ax.set_yticks(range(len(blocks)))
        ax.set_yticklabels(blocks, fontsize=6)
        ax.set_xlabel("component")
        ax.set_ylabel("block")
        ax.set_title(f"{c['method']} {c['budget']} (n = {c['n']})", fontsize=8)
    if im is not None:
        fig.colorbar(im, ax=list(axes[0]), shrink=0.8, label="Δ direct contribution to the secret's lens logit")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fig.savefig(path, dpi=150)
    plt.close(fig)


def baselines_table(rows: Dict[str, Dict[str, float]], path: str) -> None:
    lines = ["method,pass@10,majority@10,accuracy"]
    for name, m in rows.items():
        lines.append(f"{name},{m.get('any_pass', '')},{m.get('global_majority_vote', '')},{m.get('prompt_accuracy', '')}")
    atomic_write_text(path, "\n".join(lines) + "\n")


def make_report(results_dir: str, out_dir: str) -> List[str]:
    """Collects whatever result files exist under ``results_dir`` and renders the artefacts."""
    made: List[str] = []
    sweeps = os.path.join(results_dir, "sweeps")
    for root, _, files in os.walk(sweeps) if os.path.isdir(sweeps) else []:
        if "sweep_summary.json" in files:
            s = json.load(open(os.path.join(root, "sweep_summary.json")))
            tag = os.path.basename(root)
            methods = {c["method"] for c in s["curves"]}
            if {"sae_targeted", "sae_random"} & methods:
                p = os.path.join(out_dir, f"fig1_ablation_saes_{tag}.png")
                intervention_curves(s, "sae", p)
                made.append(p)
            if {"proj_targeted", "proj_random"} & methods:
                p = os.path.join(out_dir, f"fig2_lowrank_{tag}.png")
                intervention_curves(s, "proj", p)
                made.append(p)
            if any("p_donor_mean" in c for c in s["curves"]):      # only sweeps that ran the swap methods
                p = os.path.join(out_dir, f"fig4_interchange_{tag}.png")
                interchange_curves(s, p)
                made.append(p)
            p = os.path.join(out_dir, f"fig3_content_vs_inhibition_{tag}.png")
            fd = ({f"{c['method']}:{c['budget']}": c["delta"] for c in s["forcing"]["curves"]}
                  if s.get("forcing") else None)
            content_vs_inhibition(s, p, fd)
            made.append(p)
            if any("delta_logp_out" in c for c in s["curves"]):    # only sweeps run with the output readout
                p = os.path.join(out_dir, f"fig3b_content_vs_output_{tag}.png")
                content_vs_output(s, p)
                made.append(p)
            if any("kl_out_mean" in c for c in s["curves"]):       # only sweeps run with the output shift
                p = os.path.join(out_dir, f"fig5_collateral_{tag}.png")
                collateral_curves(s, p)
                made.append(p)
            if any("trace_dz_spike" in c for c in s["curves"]):    # only sweeps run with the layer trace
                p = os.path.join(out_dir, f"fig6_layer_trace_{tag}.png")
                layer_trace_curves(s, p)
                made.append(p)
            if any("movers_up_share" in c for c in s["curves"]):   # only sweeps run with the output movers
                p = os.path.join(out_dir, f"fig7_movers_{tag}.png")
                movers_curves(s, p)
                made.append(p)
            if any("comp_dz_spike" in c for c in s["curves"]):     # only sweeps run with the component trace
                p = os.path.join(out_dir, f"fig8_components_{tag}.png")
                component_heatmaps(s, p)
                made.append(p)
            if s.get("baselines"):
                from .dashboards import write_latent_dashboard

                made.append(write_latent_dashboard(s, os.path.join(out_dir, f"latent_dashboard_{tag}.html")))
    rows: Dict[str, Dict[str, float]] = {}
    ll = None
    for root, _, files in os.walk(results_dir):
        if "logit_lens_evaluation_results.json" in files:
            ll = json.load(open(os.path.join(root, "logit_lens_evaluation_results.json")))
    if ll:
        rows["LL-top-k"] = ll["overall"]
    sae_json = os.path.join(results_dir, "tables", "sae_baseline.json")
    if os.path.exists(sae_json):
        rows["SAE-top-k"] = json.load(open(sae_json))["overall"]
    for mode in ("pregame", "postgame", "naive"):
        f = os.path.join(results_dir, "token_forcing", f"{mode}.json")
        if os.path.exists(f):
            rows[f"token-forcing-{mode}" if mode != "naive" else "naive-prompting"] = json.load(open(f))["metrics"]["overall"]
    if rows:
        p = os.path.join(out_dir, "table_baselines.csv")
        baselines_table(rows, p)
        made.append(p)
    made += write_summaries(results_dir, out_dir, rows, made)
    return made


def write_summaries(results_dir: str, out_dir: str, rows: Dict[str, Dict[str, float]], made: List[str]) -> List[str]:
    """Executive summary + artefact manifest (the reference's ``reports/exec_summary``,
    ``results/artifacts.md`` stubs), filled from whatever was computed."""
    os.makedirs(out_dir, exist_ok=True)
    lines = ["# Executive summary", "", "Elicitation baselines (Pass@10 / Majority@10 / Accuracy):", ""]
    if rows:
        lines += ["| method | any_pass | global_majority_vote | prompt_accuracy |", "|---|---|---|---|"]
        for k, v in rows.items():
            lines.append(f"| {k} | {v.get('any_pass', float('nan')):.3f} | "
                         f"{v.get('global_majority_vote', float('nan')):.3f} | {v.get('prompt_accuracy', float('nan')):.3f} |")
    else:
        lines.append("(no baseline results found)")
    sweeps = os.path.join(results_dir, "sweeps")
    for root, _, files in os.walk(sweeps) if os.path.isdir(sweeps) else []:
        if "sweep_summary.json" not in files:
            continue
        s = json.load(open(os.path.join(root, "sweep_summary.json")))
        lines += ["", f"## Sweep `{os.path.relpath(root, results_dir)}`", "",
                  "| method | budget | n | Δp_secret (mean) | ΔNLL (mean) | leak | LL-top-k Pass@10 |", "|---|---|---|---|---|---|---|"]
        for c in s["curves"]:
            lines.append(f"| {c['method']} | {c['budget']} | {c['n']} | {c['delta_p_secret']['mean']:.4f} | "
                         f"{c['delta_nll']['mean']:.4f} | {c['leak_rate']:.3f} | {c['ll_topk'].get('any_pass', float('nan')):.3f} |")
    p1 = os.path.join(out_dir, "executive_summary.md")
    with open(p1, "w") as f:
        f.write("\n".join(lines) + "\n")
    p2 = os.path.join(out_dir, "artifacts.md")
    with open(p2, "w") as f:
        f.write("# Artifacts\n\n" + "\n".join(f"- `{os.path.relpath(m, out_dir)}`" for m in made + [p1]) + "\n")
    return [p1, p2]
