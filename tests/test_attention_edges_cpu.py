"""The attention edge cases (tests/attention_cases.py) on the CPU: the project's reference agrees with the fp64 ground
truth on every family, and each family's inputs tell deliberately wrong attention variants apart from the right one.

The GPU tests (tests/test_attention_edges_gpu.py) compare the kernels with the same ``truth`` under the same
tolerance, so a kernel with one of these faults fails there on the family named here.
"""
import pytest
import torch

from attention_cases import ATOL, FAMILIES, RTOL, case, case_truth, family_names, off_count, truth
from taboo_brittleness_amd.ops import reference as ref


def wrong(c, kind: str) -> torch.Tensor:
    """``truth`` with one fault, in float64.

    no_cap          the softcap is skipped
    cap_unscaled    the cap is applied to the raw dot product, the scale after it
    cap_low         a cap 10 % too small (45 for 50)
    window_le       window mask ``pos - key <= window``
    window_round32  keys from the window start rounded down to a multiple of 32, without the window mask
    prefix_le       keys ``[0, plen]`` instead of ``[0, plen)`` from the prefix slot
    online_no_acc   online softmax over 32-key blocks that does not rescale the accumulator when the maximum rises
    online_no_l     the same, not rescaling the running sum ``l`` only
    drop_tail16     the last, partial 16-key tile of a row's keys is dropped
    """
    pos, slot_rows, pre = c.rows()
    Hkv, HD, G = c.kc.shape[1], c.HD, c.G
    Hq = Hkv * G
    cap = c.cap * 0.9 if kind == "cap_low" else c.cap
    out = torch.zeros(c.M, Hq, HD, dtype=torch.float64)
    qd = c.q.reshape(c.M, Hq, HD).double()
    for i in range(c.M):
        p = int(pos[i])
        if p < 0:
            continue
        n = p + 1
        K = c.kc[int(slot_rows[i]), :, :n].double()
        V = c.vc[int(slot_rows[i]), :, :n].double()
        if pre is not None:
            npre = min(int(pre[3][i]) + (kind == "prefix_le"), n)
            if npre > 0:
                K[:, :npre] = pre[0][int(pre[2][i]), :, :npre].double()
                V[:, :npre] = pre[1][int(pre[2][i]), :, :npre].double()
        key = torch.arange(n)
        ok = key <= p
        if c.window > 0:
            if kind == "window_le":
                ok &= (p - key) <= c.window
            elif kind == "window_round32":
                ok &= key >= (max(0, p - c.window + 1) & ~31)
            else:
                ok &= (p - key) < c.window
        if kind == "drop_tail16" and n % 16:
            ok &= key < (n & ~15)
        s = torch.einsum("hgd,hnd->hgn", qd[i].view(Hkv, G, HD), K)
        if kind == "cap_unscaled":
            s = cap * torch.tanh(s / cap) * c.scale if cap > 0 else s * c.scale
        else:
            s = s * c.scale
            if cap > 0 and kind != "no_cap":
                s = cap * torch.tanh(s / cap)
        s = s.masked_fill(~ok, float("-inf"))
        if kind in ("online_no_acc", "online_no_l"):
            m = torch.full((Hkv, G, 1), float("-inf"), dtype=torch.float64)
            l = torch.zeros(Hkv, G, 1, dtype=torch.float64)
            acc = torch.zeros(Hkv, G, HD, dtype=torch.float64)
            for k0 in range(0, n, 32):
                sb = s[..., k0:k0 + 32]
                mn = torch.maximum(m, sb.amax(-1, keepdim=True))
                a = torch.exp(m - mn).nan_to_num(nan=1.0)              # nothing live yet: -inf - -inf
                pw = torch.exp(sb - mn).nan_to_num(nan=0.0)
                l = (l if kind == "online_no_l" else l * a) + pw.sum(-1, keepdim=True)
                acc = (acc if kind == "online_no_acc" else acc * a) + torch.einsum("hgn,hnd->hgd", pw, V[:, k0:k0 + 32])
                m = mn
            o = torch.where(l > 0, acc / l.clamp_min(1e-300), torch.zeros_like(acc))
        else:
            w = torch.softmax(s, dim=-1)
            w = torch.where(torch.isnan(w), torch.zeros_like(w), w)      # every key dropped: zeros
            o = torch.einsum("hgn,hnd->hgd", w, V)
        out[i] = o.reshape(Hq, HD)
    return out.view(c.M, Hq * HD)


# the families meant to catch each fault
CATCHES = {
    "softcap": ("no_cap", "cap_unscaled", "cap_low"),
    "prefill": ("online_no_acc", "online_no_l", "no_cap"),
    "packed": ("online_no_acc", "online_no_l"),
    "packed_prefix": ("prefix_le",),
    "order": ("online_no_acc", "online_no_l", "drop_tail16"),
    "window": ("window_le", "window_round32", "drop_tail16"),
    "window_prefix": ("window_le", "window_round32", "prefix_le"),
    "long": ("no_cap", "online_no_acc", "online_no_l"),
    "degenerate": ("drop_tail16",),
}


def test_wrong_is_truth_without_a_fault():
    """The variant code with no fault switched on is ``truth`` itself (to fp64 rounding), on inputs with a window, a
    prefix and padding rows: a variant's failures come from its fault, not from a second implementation."""
    for name in ("window_w17_prefix", "softcap_q12_cap5", "degenerate_256x4"):
        c = case(name)
        assert (wrong(c, "none") - case_truth(name)).abs().max().item() < 1e-12


@pytest.mark.parametrize("family", FAMILIES)
def test_reference_within_tolerance_of_truth(family):
    """``ops.reference.attention`` (bf16-rounded softmax weights, bf16 output) against ``truth``: 0 elements outside
    atol = rtol = 2e-2, the tolerance of the existing attention tests.  Measured maximum error per family:
    softcap 0.0147, prefill 0.0150, packed 0.0117, packed_prefix 0.0155, order 0.0078, window 0.0087,
    window_prefix 0.0081, long 0.0080, degenerate 0.0086.  The bf16 output rounding dominates: half an ulp is 0.0078
    for an output between 2 and 4 and 0.0156 between 4 and 8, where the tolerance is 0.06 and 0.1."""
    for name in family_names(family):
        c = case(name)
        pos, slot_rows, pre = c.rows()
        got = ref.attention(c.q, c.kc, c.vc, pos, slot_rows, c.M, 1, c.scale, c.cap, c.window, prefix=pre)
        bad, err = off_count(got, case_truth(name))
        print(f"ATTN_EDGE ref {family} {name} max_err {err:.4g}")
        assert bad == 0, f"{name}: {bad} / {got.numel()} elements off; max err {err:.4g}"
        assert (got[pos < 0] == 0).all()


@pytest.mark.parametrize("family,kind", [(f, k) for f, ks in CATCHES.items() for k in ks])
def test_inputs_tell_wrong_variant_apart(family, kind):
    """Each wrong variant is outside the tolerance on at least 1 % of the elements of the family meant to catch it."""
    bad = total = 0
    for name in family_names(family):
        c = case(name)
        b, _ = off_count(wrong(c, kind), case_truth(name))
        bad += b
        total += c.M * c.kc.shape[1] * c.G * c.HD
    print(f"ATTN_EDGE variant {family} {kind} off {bad} / {total} = {100.0 * bad / total:.2f} %")
    assert bad >= 0.01 * total, f"{kind} on {family}: only {bad} / {total} elements off"


def test_truth_is_independent_and_plain():
    """``truth`` on a hand-checkable input: two keys, scores 0 and ln 3 -> weights 1/4 and 3/4; window 1 keeps the
    last key only; a padding row gives zeros."""
    HD = 128
    q = torch.zeros(3, 1, HD, dtype=torch.float64)
    q[:, 0, 0] = 1.0
    kc = torch.zeros(1, 1, 2, HD, dtype=torch.float64)
    kc[0, 0, 1, 0] = torch.log(torch.tensor(3.0, dtype=torch.float64)) / HD ** -0.5
    vc = torch.zeros(1, 1, 2, HD, dtype=torch.float64)
    vc[0, 0, 0, 0], vc[0, 0, 1, 0] = 4.0, 8.0
    pos = torch.tensor([1, 0, -1], dtype=torch.int32)
    slot = torch.zeros(3, dtype=torch.int32)
    o = truth(q, kc, vc, pos, slot, HD ** -0.5, 0.0, 0)
    assert torch.allclose(o[:, 0], torch.tensor([7.0, 4.0, 0.0], dtype=torch.float64), atol=1e-9)
    o = truth(q, kc, vc, pos, slot, HD ** -0.5, 0.0, 1)
    assert torch.allclose(o[:, 0], torch.tensor([8.0, 4.0, 0.0], dtype=torch.float64), atol=1e-9)
    assert ATOL == RTOL == 2e-2
