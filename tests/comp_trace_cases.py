"""Cases, float64 truth and the derived error criteria of ``ops.seg_dots`` (csrc/comp_trace.hip) and of the component
trace built on it, shared by tests/test_comp_trace_cpu.py and tests/test_comp_trace_gpu.py.

The kernel criterion is derived, not measured.  Notation: ``u = 2^-24`` (fp32 unit roundoff), ``n = K / S`` the length
of a segment, ``gamma_m = m u / (1 - m u)``, ``A = sum_{k in segment} |x_k w_k|``, ``rho = sqrt(|R|^2 / Dn + eps)``
(1 without ``R``), ``z = (x . w)_segment / rho``.

* The kernel forms a segment's dot product as fp32 FMA chains per lane and a fixed tree over the lanes of its team.
  Whatever the order, a sum of ``n`` products carries at most ``n`` roundings on any path:
  ``|fl(x . w) - x . w| <= gamma_n A`` (Higham, Accuracy and Stability, section 3.1; an FMA does not round its
  product, so this is not tight).  Likewise ``fl(|R|^2) = |R|^2 (1 + t)``, ``|t| <= gamma_Dn``.
* The quotient and the root are fp64.  ``1 / sqrt(1 + t) = 1 + r`` with ``|r| <= gamma / 2 + gamma^2`` for
  ``gamma < 0.1`` (the ``gamma / 2`` of the root); ``eps >= 0`` only shrinks the relative change of ``rho``.  The fp64
  tail (two conversions, a division by ``Dn``, a sum, a root, a quotient) adds less than ``2 u`` relative, generously.
* So ``|z_hat - z| <= gamma_n A / rho (1 + gamma_Dn) + |z| (gamma_Dn / 2 + gamma_Dn^2 + 2 u)``
  (``gamma / 2 + gamma^2 <= gamma`` is used for the slack factor of the first term).  Without ``R`` the ``gamma_Dn``
  terms vanish.
* The fp32 store adds ``u |z_hat| <= u (|z| + bound)``.
* The float64 truth itself sums ``n`` products and ``Dn`` squares in float64: ``max(n, Dn) 2^-52 (A / rho + |z|)``.
* ``rms``: ``|rho_hat - rho| <= rho (gamma_Dn / 2 + gamma_Dn^2 + 2 u)`` and the store's ``u rho_hat``.

The completeness criterion of the component trace (:func:`completeness_bound`) is derived from the model's own bf16
roundings.  With the final norm frozen, ``h_last . v = h_l . v + sum_b (n_b,attn + n_b,ffn) . v + (rounding of the
residual adds)``, where ``n = rbf(y_bf / rho(y_bf) * (1 + g))`` is the normed sublayer output the model adds and
``y_bf = rbf(y)`` the bf16 projection output.  A component is ``(y' . ((1 + g) v)) / rho(y_bf)`` with ``y' = y_bf`` for
an MLP and ``y' = a @ W_o^T`` unrounded for the heads (the table carries ``W_o``).  With
``t = y_bf / rho(y_bf) (1 + g)`` the unrounded normed output, a later sublayer contributes to the difference between
the telescoped sum and the components, in the numerator ``. v``:

* ``y`` rounded to bf16 (heads only; kept for the MLP as slack): ``|y_bf - y'| <= 2^-9 |y_bf|`` plus the GEMM's fp32
  accumulation ``gamma_K sum_k |a_k| |W_o,dk|``; through the gain and ``1 / rho``:
  ``2^-9 sum_d |t_d| |v_d| + gamma_K sum_d (|a| @ |W_o|^T)_d (1 + g_d) |v_d| / rho``;
* the normed output rounded to bf16: ``2^-9 sum_d |t_d| |v_d|``, and the fp32 arithmetic of the norm before that
  rounding (a mean of ``D`` squares, a reciprocal root, two products), ``(gamma_D + 4 u) sum_d |t_d| |v_d|``;
* the residual add rounded to bf16: ``2^-9 sum_d |h'_d| |v_d|`` with ``h'`` the new residual row.

That is three terms of ``2^-9 sum_d |.| |v_d|`` per later sublayer and their fp32 riders, computed in fp64 from the
captured rows, plus the kernel criterion of every component, of the direct term and of the total, all over ``rho_f``.

Every term is computed per element from the inputs; nothing here comes from a run of the code under test.
"""
import math

import torch

BF = torch.bfloat16
U32 = 2.0 ** -24
UBF = 2.0 ** -9
EPS = 1e-6
# (K, S, Dn): one group per segment, most lanes idle; three groups per segment, segments straddling lane boundaries;
# a ragged last pass; the tiny model's attention (Dn != K); the 9B attention; the 9B MLP / residual
SEG_SHAPES = ((64, 8, 64), (120, 5, 64), (328, 1, 328), (1024, 4, 512), (4096, 16, 3584), (3584, 1, 3584))
SEG_T = (1, 2, 4)
SEG_MS = (1, 5, 257)
SEG_U = 3
SEG_M = 24                       # source rows the selection picks from


def seg_sel(Ms: int):
    """``(rows [Ms], blk [Ms])`` int32: rows unsorted, repeated and out of range (``-1``, ``M``), blocks with ``-1``
    and ``U``; both kinds of skipped entries sit inside runs and inside a workgroup's four rows."""
    if Ms == 1:
        return torch.tensor([7], dtype=torch.int32), torch.tensor([1], dtype=torch.int32)
    if Ms == 5:
        return (torch.tensor([3, 0, SEG_M, 3, -1], dtype=torch.int32),
                torch.tensor([2, -1, 0, SEG_U, 1], dtype=torch.int32))
    g = torch.Generator().manual_seed(Ms)
    rows = torch.randint(0, SEG_M, (Ms,), generator=g).to(torch.int32)
    blk = torch.empty(Ms, dtype=torch.int32)
    blk[:100] = 2
    blk[100:200] = 0
    blk[200:] = torch.tensor([1, 0, 2], dtype=torch.int32).repeat(Ms)[: Ms - 200]
    rows[10], rows[11], rows[150] = -1, SEG_M, SEG_M + 5
    blk[40], blk[41], blk[201] = 1, -1, SEG_U
    rows[60] = rows[59]
    return rows, blk


def seg_case(K: int, S: int, Dn: int, T: int, Ms: int, seed: int = 0):
    """``(X [M, K] bf16, W [U, T, K] fp32, rows, blk, R [M, Dn] bf16)``.  The rows of ``R`` cycle through three
    scales: ``|R|^2 / Dn`` near 1, near ``eps`` (so a missing ``eps`` shows) and near 900; ``X`` runs at a third of
    ``R``'s scale (so a ``rho`` taken from ``X`` shows).  Every third row of ``X`` and every table row carry large
    aligned entries in the first and the last column of every segment, the table's growing with the segment (so a
    dropped last group and a shifted boundary show).  The last segment of the last column of table block 1 is zero."""
    g = torch.Generator().manual_seed(100000 * S + 10 * K + T + 1000 * Ms + seed)
    n = K // S
    scale = torch.tensor([1.0, 1e-3, 30.0]).repeat(SEG_M)[:SEG_M]
    R = torch.randn(SEG_M, Dn, generator=g) * scale[:, None]
    X = torch.randn(SEG_M, K, generator=g) * (scale[:, None] / 3.0)
    W = 0.5 * torch.randn(SEG_U, T, K, generator=g)
    for s in range(S):
        X[::3, s * n] = 2.0 * scale[::3]
        X[::3, (s + 1) * n - 1] = 2.0 * scale[::3]
        W[:, :, s * n] = 1.0 + 0.5 * s
        W[:, :, (s + 1) * n - 1] = 2.0 + 0.25 * s
    W[1, T - 1, K - n:] = 0.0
    rows, blk = seg_sel(Ms)
    return X.to(BF), W.contiguous(), rows, blk, R.to(BF)


def _gamma(m: int) -> float:
    return m * U32 / (1.0 - m * U32)


def seg_truth(X, W, rows, blk, S: int, R, eps: float) -> dict:
    """Float64 truth ``z [Ms, T, S]`` and ``rho [Ms]`` with the per-element bounds of the module docstring; ``ok [Ms]``
    marks the selected rows that are read, ``zero [Ms, T, S]`` the elements that must be exactly +0.0."""
    M, K = X.shape
    U, T = W.shape[0], W.shape[1]
    n = K // S
    r, u = rows.long().cpu(), blk.long().cpu()
    ok = (r >= 0) & (r < M) & (u >= 0) & (u < U)
    rc, uc = r.clamp(0, M - 1), u.clamp(0, U - 1)
    xd = X.double().cpu()[rc]
    Wd = W.double().cpu()[uc]                                          # [Ms, T, K]
    prod = (xd[:, None, :] * Wd).view(-1, T, S, n)
    dot, A = prod.sum(-1), prod.abs().sum(-1)
    if R is None:
        Dn, gd = 0, 0.0
        rho = torch.ones(r.shape[0], dtype=torch.float64)
    else:
        Dn = R.shape[1]
        gd = _gamma(Dn)
        rho = torch.sqrt(R.double().cpu()[rc].pow(2).sum(-1) / Dn + eps)
    rr = rho[:, None, None]
    z = dot / rr
    gn = _gamma(n)
    bz = gn * (A / rr) * (1.0 + gd) + z.abs() * (gd / 2 + gd * gd + 2 * U32)
    bound = bz + U32 * (z.abs() + bz) + max(n, Dn) * 2.0 ** -52 * (A / rr + z.abs())
    brho = rho * (gd / 2 + gd * gd + 2 * U32)
    brho = brho + U32 * (rho + brho) + max(Dn, 1) * 2.0 ** -52 * rho
    o3 = ok[:, None, None]
    zero = ~o3 | (Wd.view(-1, T, S, n).abs().sum(-1) == 0)
    zz = torch.zeros_like(z)
    return {"z": torch.where(o3, z, zz), "bound": torch.where(o3, bound, zz), "ok": ok, "zero": zero,
            "rho": torch.where(ok, rho, torch.zeros_like(rho)),
            "rho_bound": torch.where(ok, brho, torch.zeros_like(rho))}


def check_seg(out: torch.Tensor, rms: torch.Tensor, t: dict, what: str = "") -> list:
    """Failures of ``(out [Ms, T, S], rms [Ms])`` against a truth: elements past their bound and elements that must be
    exactly +0.0."""
    o, q = out.detach().cpu(), rms.detach().cpu()
    if o.dtype != torch.float32 or tuple(o.shape) != tuple(t["z"].shape):
        return [f"{what}: out is {o.dtype} {tuple(o.shape)}"]
    if q.dtype != torch.float32 or tuple(q.shape) != tuple(t["rho"].shape):
        return [f"{what}: rms is {q.dtype} {tuple(q.shape)}"]
    bad = []
    err = (o.double() - t["z"]).abs()
    over = (err > t["bound"]) | ~torch.isfinite(o)
    for i, j, k in over.nonzero().tolist()[:4]:
        bad.append(f"{what}: [{i}, {j}, {k}] = {float(o[i, j, k])!r}, truth {float(t['z'][i, j, k])!r}, "
                   f"error {float(err[i, j, k]):.3e} > bound {float(t['bound'][i, j, k]):.3e}")
    nz = t["zero"] & (o.view(torch.int32) != 0)                       # +0.0 exactly
    for i, j, k in nz.nonzero().tolist()[:4]:
        bad.append(f"{what}: [{i}, {j}, {k}] = {float(o[i, j, k])!r}, want exactly +0.0")
    er = (q.double() - t["rho"]).abs()
    ov = (er > t["rho_bound"]) | ~torch.isfinite(q) | (~t["ok"] & (q.view(torch.int32) != 0))
    for (i,) in ov.nonzero().tolist()[:4]:
        bad.append(f"{what}: rms[{i}] = {float(q[i])!r}, truth {float(t['rho'][i])!r}, error {float(er[i]):.3e} > "
                   f"bound {float(t['rho_bound'][i]):.3e}")
    return bad


def run_seg(fn, device, K: int, S: int, Dn: int, Ts=SEG_T, Mss=SEG_MS, with_R=(True, False)) -> list:
    """``fn(X, W, rows, blk, S, R, eps, out=, rms=)`` over every ``T``, selection size and with / without ``R`` at
    one shape, NaN-filled outputs."""
    bad = []
    for T in Ts:
        for Ms in Mss:
            X, W, rows, blk, R = seg_case(K, S, Dn, T, Ms)
            for wr in with_R:
                Rr = R if wr else None
                t = seg_truth(X, W, rows, blk, S, Rr, EPS)
                out = torch.full((Ms, T, S), float("nan"), dtype=torch.float32, device=device)
                rms = torch.full((Ms,), float("nan"), dtype=torch.float32, device=device)
                got = fn(X.to(device), W.to(device), rows.to(device), blk.to(device), S,
                         None if Rr is None else Rr.to(device), EPS, out=out, rms=rms)
                o, q = (out, rms) if got is None else got
                bad += check_seg(o, q, t, f"K {K} S {S} Dn {Dn} T {T} Ms {Ms} R {wr}")
    return bad


MUTANTS = ("drop_last", "shift", "rho_from_x", "no_eps", "t_stride", "dn_is_k")


def seg_mutant(bug: str = ""):
    """A float64 stand-in for the kernel with one planted bug: ``drop_last`` a segment's last 8-column group dropped;
    ``shift`` segment boundaries shifted by one group; ``rho_from_x`` the RMS taken from ``X`` instead of ``R``;
    ``no_eps`` ``eps`` left out; ``t_stride`` table column ``t`` read with a stride of ``K - 8`` floats;
    ``dn_is_k`` ``K`` where ``Dn`` belongs in the mean.  Without a bug it meets the criterion."""
    assert bug in MUTANTS + ("",)

    def fn(X, W, rows, blk, S, R, eps, out=None, rms=None):
        M, K = X.shape
        U, T = W.shape[0], W.shape[1]
        n = K // S
        r, u = rows.long(), blk.long()
        ok = (r >= 0) & (r < M) & (u >= 0) & (u < U)
        rc, uc = r.clamp(0, M - 1), u.clamp(0, U - 1)
        xd = X.double()[rc]
        Wb = W.double()
        if bug == "t_stride":
            flat = torch.cat([Wb.reshape(U, T * K), torch.zeros(U, 8 * T, dtype=torch.float64)], 1)
            Wb = torch.stack([flat[:, t * (K - 8): t * (K - 8) + K] for t in range(T)], 1)
        prod = xd[:, None, :] * Wb[uc]                                  # [Ms, T, K]
        if bug == "shift":
            prod = torch.cat([prod[:, :, 8:], torch.zeros_like(prod[:, :, :8])], -1)
        prod = prod.view(-1, T, S, n)
        if bug == "drop_last":
            prod = prod[..., : n - 8]
        dot = prod.sum(-1)
        if R is None:
            rho = torch.ones(r.shape[0], dtype=torch.float64)
        else:
            src = xd if bug == "rho_from_x" else R.double()[rc]
            Dn = K if bug == "dn_is_k" else R.shape[1]
            rho = torch.sqrt(src.pow(2).sum(-1) / Dn + (0.0 if bug == "no_eps" else eps))
        z = torch.where(ok[:, None, None], dot / rho[:, None, None], torch.zeros_like(dot)).float()
        q = torch.where(ok, rho, torch.zeros_like(rho)).float()
        if out is not None:
            out.copy_(z)
            rms.copy_(q)
            return out, rms
        return z, q
    return fn


# ---------------------------------------------------------------- the component trace on a model

def lens_dirs(model, ids) -> torch.Tensor:
    """``v [T, D]`` fp64: ``lm_head[id] * (1 + norm_f)`` (interp/gradient.py::lens_direction) per tracked id."""
    from taboo_brittleness_amd.interp.gradient import lens_direction

    return torch.stack([lens_direction(model, [int(t)]).double().cpu() for t in ids])


def rho_of(y: torch.Tensor, eps: float) -> torch.Tensor:
    y = y.double()
    return torch.sqrt(y.pow(2).sum(-1) / y.shape[-1] + eps)


def head_truth(attn_row, o_row, Wo, gain, v, heads: int, eps: float) -> dict:
    """One row's per-head components in fp64, from the captured ``ws.attn`` row ``[heads * head_dim]``, the bf16
    ``o_proj`` output ``o_row [D]``, ``Wo [D, heads * head_dim]``, ``gain = ln_post_attn [D]`` and ``v [D]``:
    ``c_head = (a_head . A_head) / rho(o)`` with ``A = ((1 + gain) * v) @ Wo`` rounded once to fp32 as the table is,
    and the kernel criterion of each at ``n = head_dim``, ``Dn = D``."""
    a = attn_row.double().cpu()
    A = (((1.0 + gain.double().cpu()) * v.double().cpu()) @ Wo.double().cpu()).float().double()
    hd = a.shape[0] // heads
    prod = (a * A).view(heads, hd)
    rho = float(rho_of(o_row.cpu(), eps))
    c, Ab = prod.sum(-1) / rho, prod.abs().sum(-1) / rho
    gn, gd = _gamma(hd), _gamma(o_row.shape[0])
    bz = gn * Ab * (1.0 + gd) + c.abs() * (gd / 2 + gd * gd + 2 * U32)
    return {"c": c, "bound": bz + U32 * (c.abs() + bz) + max(hd, o_row.shape[0]) * 2.0 ** -52 * (Ab + c.abs())}


def sublayer_slack(y_bf, gain, h_new, v, eps: float, attn=None, Wo=None):
    """The bf16 roundings of one later sublayer and their fp32 riders, in the numerator of the lens logit (module
    docstring), fp64, for one row ``[D]`` (a float) or for rows ``[n, D]`` (a tensor ``[n]``):
    ``(2 * 2^-9 + gamma_D + 4 u) sum_d |t_d| |v_d|`` for ``t = y_bf / rho(y_bf) (1 + gain)``,
    ``2^-9 sum_d |h'_d| |v_d|`` for the residual add and, for the heads (``attn`` rows and ``Wo`` given), the GEMM's
    ``gamma_K`` term."""
    one = y_bf.dim() == 1
    y = y_bf.double().cpu().reshape(-1, y_bf.shape[-1])
    va = v.double().cpu().abs()
    g1 = (1.0 + gain.double().cpu()).abs()
    rho = rho_of(y, eps)
    t = y / rho[:, None] * g1
    out = (2.0 * UBF + _gamma(y.shape[1]) + 4 * U32) * (t.abs() * va).sum(-1)
    out = out + UBF * (h_new.double().cpu().reshape(-1, y.shape[1]).abs() * va).sum(-1)
    if attn is not None:
        a = attn.double().cpu().reshape(y.shape[0], -1)
        acc = a.abs() @ Wo.double().cpu().abs().T
        out = out + _gamma(a.shape[1]) * (acc * g1 * va).sum(-1) / rho
    return float(out[0]) if one else out


def completeness_bound(slacks, kernel_bounds, rho_f: float) -> float:
    """Bound on ``|direct + sum of components - z_pre|`` in logit units: the later sublayers' rounding slacks (in the
    numerator, so over ``rho_f``) plus the kernel criterion of every reported number (already in logit units)."""
    return sum(slacks) / rho_f + sum(kernel_bounds)


assert math.isclose(U32, torch.finfo(torch.float32).eps / 2)
