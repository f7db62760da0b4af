"""Cases, float64 truth and the derived error criterion of ``ops.lens_track`` (csrc/lens_track.hip), shared by
tests/test_layer_trace_cpu.py and tests/test_layer_trace_gpu.py.

The criterion is derived, not measured.  Notation: ``u = 2^-24`` (fp32 unit roundoff), ``gamma = D u / (1 - D u)``,
``S = sum_d |h_d v_d|``, ``r = sqrt(|h|^2 / D + eps)``, ``z = (h . v) / r``, ``f`` the softcap.

* The kernel forms ``h . v`` and ``|h|^2`` as fp32 FMA chains per lane and a fixed tree over the 64 lanes.  Whatever
  the order, a sum of ``D`` products carries at most ``D`` roundings on any path: ``|fl(h . v) - h . v| <= gamma S``
  and ``fl(|h|^2) = |h|^2 (1 + t)``, ``|t| <= gamma`` (Higham, Accuracy and Stability, section 3.1; an FMA does not
  round its product, so this is not tight).
* The quotient and the root are fp64.  ``1 / sqrt(1 + t) = 1 + rho`` with ``|rho| <= gamma / 2 + gamma^2`` for
  ``gamma < 0.1``; ``eps >= 0`` only shrinks the relative change of ``r``.  The fp64 operations (two conversions,
  a division by ``D``, a sum, a root, a quotient) add less than ``2 u`` relative, generously.
* So ``|z_hat - z| <= gamma S / r (1 + gamma / 2 + gamma^2) + |z| (gamma / 2 + gamma^2 + 2 u)``: the first-order
  bound ``gamma S / r + |z| (gamma / 2 + 2 u)`` with its second-order slack (``gamma^2`` terms; ``gamma / 2 +
  gamma^2 <= gamma`` is used for the slack factor of the first term).
* ``f`` is 1-Lipschitz (``|f'| = 1 - tanh^2 <= 1``), so the bound carries through the cap; the fp64 ``tanh`` is good
  to a few fp64 ulps, inside the ``2 u |z|`` above.  The fp32 store adds ``u |f_hat| <= u (|f(z)| + bound)``.
* The float64 truth itself sums ``D`` products in float64: ``D 2^-52 (S / r + |z|)``.

Every term is computed per element from the inputs; nothing here comes from a run of the code under test.
"""
import math

import torch

BF = torch.bfloat16
U32 = 2.0 ** -24
EPS = 1e-6
TRACE_D = (64, 328, 3584)        # most lanes idle; a ragged last 16-byte pass; the 9B width (7 LDS chunks)
TRACE_T = (1, 3, 8)
TRACE_M = (1, 5, 257)            # fewer rows than a workgroup takes; one row past a multiple of 16
TRACE_CAPS = (0.0, 30.0)
TRACE_U = 3


def trace_vrow(M: int) -> torch.Tensor:
    """Row map over ``U = 3`` table blocks: unsorted, repeated, with ``-1`` and ``U`` (both skipped).  At 257 rows
    there are runs long enough that whole workgroups share a block, runs that change block inside a workgroup and
    inside a wave, skipped rows inside a run, and a last workgroup of one row."""
    if M == 1:
        return torch.tensor([1], dtype=torch.int32)
    if M == 5:
        return torch.tensor([2, 0, -1, TRACE_U, 0], dtype=torch.int32)
    v = torch.empty(M, dtype=torch.int32)
    v[:100] = 2
    v[100:102] = -1
    v[102:200] = 0
    v[200] = TRACE_U
    v[201:] = torch.tensor([1, 0, 2], dtype=torch.int32).repeat(M)[: M - 201]
    v[40] = 1                    # one row of another block inside a run
    v[150] = -1                  # one skipped row inside a run
    return v


def trace_case(D: int, T: int, M: int, seed: int = 0):
    """``(h [M, D] bf16, V [U, T, D] fp32, vrow [M] int32)``.  Rows cycle through three scales: ``|h|^2 / D`` near 1,
    near ``eps`` (so a missing ``eps`` shows) and near 900; every third row and every table row carry a large aligned
    entry in the last column (so a dropped tail shows).  The last column of table block 1 is an absent id: zeros."""
    g = torch.Generator().manual_seed(1000 * D + 10 * T + M + seed)
    h = torch.randn(M, D, generator=g)
    scale = torch.tensor([1.0, 1e-3, 30.0]).repeat(M)[:M]
    h = h * scale[:, None]
    h[::3, D - 1] = 6.0 * scale[::3]
    V = 0.5 * torch.randn(TRACE_U, T, D, generator=g)
    V[:, :, D - 1] = 2.0
    V[1, T - 1] = 0.0
    return h.to(BF), V.contiguous(), trace_vrow(M)


def trace_truth(h: torch.Tensor, V: torch.Tensor, vrow: torch.Tensor, eps: float, cap: float) -> dict:
    """Float64 truth ``f [M, T]`` and the per-element ``bound`` of the module docstring; ``ok [M]`` marks the rows
    that are read out, ``zero [M, T]`` the elements that must be exactly 0.0 (skipped rows, all-zero table rows)."""
    M, D = h.shape
    U, T = V.shape[0], V.shape[1]
    u = vrow.long()
    ok = (u >= 0) & (u < U)
    hd = h.double().cpu()
    Vd = V.double().cpu()[u.clamp(0, U - 1).cpu()]                     # [M, T, D]
    prod = hd[:, None, :] * Vd
    dot, S = prod.sum(-1), prod.abs().sum(-1)
    r = torch.sqrt(hd.pow(2).sum(-1) / D + eps)[:, None]
    z = dot / r
    f = cap * torch.tanh(z / cap) if cap > 0 else z
    gam = D * U32 / (1.0 - D * U32)
    bz = gam * (S / r) * (1.0 + gam) + z.abs() * (gam / 2 + gam * gam + 2 * U32)
    bound = bz + U32 * (f.abs() + bz) + D * 2.0 ** -52 * (S / r + z.abs())
    okc = ok.cpu()[:, None]
    zero = ~okc | (Vd.abs().sum(-1) == 0)
    return {"f": torch.where(okc, f, torch.zeros_like(f)), "z": z, "S_over_r": S / r,
            "bound": torch.where(okc, bound, torch.zeros_like(bound)), "ok": ok.cpu(), "zero": zero}


def check_trace(out: torch.Tensor, t: dict, what: str = "") -> list:
    """Failures of ``out [M, T]`` against a truth: elements past their bound, and elements that must be exactly 0."""
    o = out.detach().cpu()
    bad = []
    if o.dtype != torch.float32 or tuple(o.shape) != tuple(t["f"].shape):
        return [f"{what}: out is {o.dtype} {tuple(o.shape)}"]
    err = (o.double() - t["f"]).abs()
    over = (err > t["bound"]) | ~torch.isfinite(o)
    for i, j in over.nonzero().tolist()[:4]:
        bad.append(f"{what}: [{i}, {j}] = {float(o[i, j])!r}, truth {float(t['f'][i, j])!r}, "
                   f"error {float(err[i, j]):.3e} > bound {float(t['bound'][i, j]):.3e}")
    nz = t["zero"] & (o.view(torch.int32) != 0)                       # +0.0 exactly
    for i, j in nz.nonzero().tolist()[:4]:
        bad.append(f"{what}: [{i}, {j}] = {float(o[i, j])!r}, want exactly 0.0")
    return bad


def run_trace(fn, device, D: int, T: int, Ms=TRACE_M, caps=TRACE_CAPS) -> list:
    """``fn(h, V, vrow, eps, cap, out=)`` over every row count and cap at one ``(D, T)``, NaN-filled outputs."""
    bad = []
    for M in Ms:
        h, V, vrow = trace_case(D, T, M)
        for cap in caps:
            t = trace_truth(h, V, vrow, EPS, cap)
            out = torch.full((M, T), float("nan"), dtype=torch.float32, device=device)
            got = fn(h.to(device), V.to(device), vrow.to(device), EPS, cap, out=out)
            bad += check_trace(out if got is None else got, t, f"D {D} T {T} M {M} cap {cap}")
    return bad


def trace_mutant(drop_tail: bool = False, rms_is_d: bool = False, no_eps: bool = False, t_stride: bool = False):
    """A float64 stand-in for the kernel with one planted bug: the last 16-byte piece of every row dropped; ``D``
    where ``|h|^2 / D`` belongs; ``eps`` left out; table column ``t`` read with a stride of ``D - 8`` floats instead
    of ``D``.  Without a bug it meets the criterion."""
    def fn(h, V, vrow, eps, cap, out=None):
        M, D = h.shape
        U, T = V.shape[0], V.shape[1]
        u = vrow.long()
        ok = (u >= 0) & (u < U)
        hd = h.double()
        Vb = V.double()
        if t_stride:
            flat = torch.cat([Vb.reshape(U, T * D), torch.zeros(U, 8 * T, dtype=torch.float64)], 1)
            Vb = torch.stack([flat[:, t * (D - 8): t * (D - 8) + D] for t in range(T)], 1)
        Vr = Vb[u.clamp(0, U - 1)]
        n = D - 8 if drop_tail else D
        dot = (hd[:, None, :n] * Vr[:, :, :n]).sum(-1)
        ms = torch.full((M,), float(D), dtype=torch.float64) if rms_is_d else hd[:, :n].pow(2).sum(-1) / D
        z = dot / torch.sqrt(ms + (0.0 if no_eps else eps))[:, None]
        f = cap * torch.tanh(z / cap) if cap > 0 else z
        res = torch.where(ok[:, None], f, torch.zeros_like(f)).float()
        if out is not None:
            out.copy_(res)
            return out
        return res
    return fn


def lens_z(model, h: torch.Tensor, ids) -> dict:
    """Float64 capped lens logits of residual rows ``h [n, D]`` for the token ids ``ids`` through the model's final
    norm gain and unembedding rows (the closed form of interp/gradient.py::lens_direction), with the per-element
    bound: ``trace_truth`` over a one-block table."""
    from taboo_brittleness_amd.interp.gradient import lens_direction

    D = h.shape[1]
    V = torch.zeros(1, len(ids), D)
    for j, t in enumerate(ids):
        V[0, j] = lens_direction(model, [int(t)]).float().cpu()
    cap = float(model.spec.final_softcap or 0.0)
    return trace_truth(h.cpu(), V, torch.zeros(h.shape[0], dtype=torch.int32), model.spec.eps, cap)


assert math.isclose(U32, torch.finfo(torch.float32).eps / 2)
