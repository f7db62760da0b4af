"""The vocabulary readouts of csrc/lens.hip -- argmax_rows, row_lse, xent_rows, decode_head, decode_head_stats,
gather_probs, lens_colsum and topk_rows -- held to float64 references at every row geometry of their streams
(criteria, cases and runners: tests/readout_cases.py, checked against themselves in tests/test_readouts_cpu.py).
Integer outputs are exact; log-sum-exps, NLLs and probabilities lie within bounds derived from the fp32 arithmetic
of the kernels.  Every test prints the largest error it saw as a fraction of its bound.

Seen on an MI355X, largest error as a fraction of the bound over all cases: row_lse and xent_rows 0.24, decode_head
NLLs 0.18, decode_head_stats lse 0.12, gather_probs 0.06 (rounded: always the correctly rounded float64 value);
lens_colsum unrounded 0.06 of its window from zero and 0.99 onto a start, where the window is one fp32 rounding of
the sum; with ``round_bf16`` it sits on the window's edge whenever a term's window is two neighbouring bf16 values.
No integer output, bit identity or exact zero was ever off."""
import pytest
import torch

import readout_cases as rd
from taboo_brittleness_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("V", rd.STREAM_WIDTHS)
def test_streamed_readouts(gpu, V):
    """argmax_rows, row_lse / xent_rows (``emulate_bf16`` both ways), decode_head and decode_head_stats at caps 30, 50
    and 0 on random, planted-maximum, saturated-tie, constant, far-negative and lens-like rows; targets -1, V, 0,
    V - 1, a tail column, a tie member and the argmax; and the bit identities of kernels that share one row pass
    (xent_rows = row_lse - capped target logit; the running-max decode_head's nll_tgt = xent_rows)."""
    rd.run_stream(ops, gpu, V, fill=True, bits=True).assert_ok(f"V {V}")


def test_decode_head_more_rows_than_workgroups(gpu):
    """decode_head and decode_head_stats (non-zero ``off``) over 2 x compute units + 3 different rows: the persistent
    kernel's workgroups each take more than one row, and every row is held to the float64 reference."""
    R = 2 * torch.cuda.get_device_properties(gpu).multi_processor_count + 3
    rd.run_persist(ops, gpu, R, fill=True).assert_ok("persistent grid")


@pytest.mark.parametrize("V", rd.GATHER_WIDTHS)
def test_gather_probs(gpu, V):
    """``round_bf16`` both ways, ids -1, V, duplicates and the row maximum, direct and through a ``rowmap`` with
    repeated and permuted rows, fed the reference's fp32 lse."""
    rd.run_gather(ops, gpu, V, fill=True).assert_ok(f"V {V}")


@pytest.mark.parametrize("rb", [False, True])
@pytest.mark.parametrize("V", rd.COLSUM_WIDTHS)
def test_lens_colsum(gpu, V, rb):
    """Dense with skipped rows and exclusions aimed at the column holding over 90 % of a row's mass, overwriting a
    NaN-filled ``acc`` and accumulating onto a start, ``cum`` at every prefix; packed with empty sequences; through a
    ``rowmap``; and the bit identities of a kernel that adds row by row."""
    rd.run_colsum(ops, gpu, V, rb, bits=True).assert_ok(f"V {V}")


@pytest.mark.parametrize("V", rd.TOPK_WIDTHS)
def test_topk_rows(gpu, V):
    """K at both ends of every candidate-list size, on rows with ties, a constant row, fewer than K finite values,
    the K best inside one chunk and at the chunk edges; indices exact, values bit-equal."""
    rd.run_topk(ops, gpu, V).assert_ok(f"V {V}")


def test_topk_rows_whole_row_and_k_past_the_row(gpu):
    """K == V returns the whole row in stable order; K > V raises instead of writing sentinel indices."""
    rd.run_topk_all(ops, gpu).assert_ok("K == V")
    with pytest.raises(RuntimeError):
        ops.topk_rows(torch.zeros(2, 5, device=gpu), 6)
