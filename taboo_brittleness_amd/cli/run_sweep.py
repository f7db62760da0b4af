"""``python -m taboo_brittleness_amd.cli.run_sweep [cfg] [--methods sae|proj|all]`` — targeted-vs-random
SAE-latent ablation and low-rank projection sweeps (EP:112-152); ``--methods sae_noise|proj_noise|all_noise`` add the
norm-matched controls, ``--methods sae_swap|proj_swap|swap`` the interchange (donor-swap) methods.  Multi-GPU:
``python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m taboo_brittleness_amd.cli.run_sweep cfg``."""
import os

from ..parallel import dist as D
from ..pipelines.run_sweep import run_sweep
from .common import parser, setup

METHOD_SETS = {"sae": ("sae_targeted", "sae_random"), "proj": ("proj_targeted", "proj_random"),
               "all": ("sae_targeted", "sae_random", "proj_targeted", "proj_random")}
# each set plus its norm-matched control(s) (pipelines/sweep_types.py NOISE_METHODS; intervention.noise_trials draws)
METHOD_SETS.update({"sae_noise": METHOD_SETS["sae"] + ("sae_noise",),
                    "proj_noise": METHOD_SETS["proj"] + ("proj_noise",),
                    "all_noise": METHOD_SETS["all"] + ("sae_noise", "proj_noise")})
# each set plus its interchange (donor-swap) methods (pipelines/sweep_types.py SWAP_METHODS; intervention.swap_donor)
METHOD_SETS.update({"sae_swap": METHOD_SETS["sae"] + ("sae_swap", "sae_swap_random"),
                    "proj_swap": METHOD_SETS["proj"] + ("proj_swap", "proj_swap_random"),
                    "swap": METHOD_SETS["all"] + ("sae_swap", "sae_swap_random", "proj_swap", "proj_swap_random")})


def main(argv=None):
    ap = parser(__doc__)
    ap.add_argument("--methods", default="all", choices=sorted(METHOD_SETS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--forcing", action="store_true",
                    help="also measure postgame token forcing under each (method, budget) edit (EP:100-104)")
    ap.add_argument("--output-readout", action="store_true",
                    help="also record the model's next-token log-prob / rank of the tracked ids at every response "
                         "position (intervention.output_readout; no fused head, TP or decode-tail carry-over)")
    ap.add_argument("--output-shift", action="store_true",
                    help="also record the KL divergence between each cell's and its baseline's next-token distribution "
                         "over the teacher-forced response (intervention.output_shift; needs layer resume; no fused "
                         "head, TP or decode-tail carry-over)")
    ap.add_argument("--layer-trace", action="store_true",
                    help="also record the capped lens logit of the tracked ids at every block from the hooked layer on, "
                         "for each cell and its baseline over the teacher-forced response (intervention.layer_trace; "
                         "needs layer resume; no TP or decode-tail carry-over)")
    ap.add_argument("--output-movers", action="store_true",
                    help="also record, per edited spike, the tokens that gained and lost the most next-token "
                         "probability against the baseline and the total variation (intervention.output_movers, "
                         "intervention.movers_k; needs layer resume; no fused head, TP or decode-tail carry-over)")
    ap.add_argument("--component-trace", action="store_true",
                    help="also split the secret's lens logit behind each edit into the direct term and one term per "
                         "attention head and per MLP of every later block, at the edited spike rows and the rows right "
                         "behind them, for each cell and its baseline (intervention.component_trace; needs layer "
                         "resume and GEMM mode tb; no TP, LoRA bank or decode-tail carry-over)")
    args = ap.parse_args(argv)
    cfg, dev = setup(args)
    if args.component_trace:
        cfg.intervention.component_trace = True
    if args.output_movers:
        cfg.intervention.output_movers = True
    if args.layer_trace:
        cfg.intervention.layer_trace = True
    if args.forcing:
        cfg.intervention.measure_forcing = True
    if args.output_readout:
        cfg.intervention.output_readout = True
    if args.output_shift:
        cfg.intervention.output_shift = True
    info = D.init_distributed(cfg.parallel.backend, "cpu" if dev.type == "cpu" else "auto")
    out = args.out or os.path.join(cfg.data.results_dir, "sweeps", f"{args.methods}_seed{cfg.experiment.seed}")
    summary = run_sweep(cfg, out, METHOD_SETS[args.methods], info=info, batch=args.batch)
    D.destroy(info)
    return summary


if __name__ == "__main__":
    main()
