"""Backward of compositing (ns_raw2outputs_backward) against float64 torch autograd: the reference, the error model and its
comparator.  Used by tests/test_gpu_composite_backward.py; the inputs are composite_bounds.make_inputs (every sigma regime,
duplicate depths, the last sample's 1e10 step, opaque / transparent / thin rays, a NaN and an inf sigma).

The error model, first order, every fp32 rounding counted once (u = 2^-24), on top of the forward's model of
composite_bounds.py: e_alpha_i (absolute), rel_T_i (relative, of T_i), e_w_i, e_acc, e_depth, e_q (of 1 / disp).  Everything
else is the float64 reference on the same fp32 inputs; |x| marks a sum taken with the absolute value of every term.
  per ray: Gq = -G_disp disp^2 [q > 1e-10] (half on the tie), rel_q = e_q / q + 4u;
     Gd = G_depth + Gq / den,  Ga = G_acc - white sum_c G_c - Gq depth / den^2   (den = acc + 1e-10)
     e_Gd = |Gq / den| (2 rel_q + e_acc / den + 4u) + u |Gd|
     e_Ga = |Gq depth / den^2| (2 rel_q + e_depth / depth + 2 e_acc / den + 6u) + 3u (|Ga| + sum_c |G_c|)
  g_i = G_w_i + sum_c G_c c_i + Gd z_i + Ga;   e_g_i = sum_c |G_c| E_SIG + e_Gd z_i + e_Ga + 4u |g|_i
  U_k = keep_{k+1} U_{k+1} + g_{k+1} alpha_{k+1};  |U| by the same recurrence on |g|;  e_U by the recurrence with
      b_i = |g_i| e_alpha_i + e_g_i alpha_i, plus rel_T_N |U|_k (the keep factors' own errors, at most the whole ray's)
  dalpha_k = G_alpha_k + T_k (g_k - U_k):
      e_da_k = T_k [(rel_T_k + 3u)(|g|_k + |U|_k) + e_g_k + e_U_k] + L u T_k |U|_k       (L: the scan's depth,
      log2(SW) + 2 for one chunk, 8 + chunks beyond 64 samples)
  with e = exp(-relu(s) dist) and its absolute error e_exp (composite_bounds.py's, or e itself below 2^-126: the
  transcendental unit flushes a result below fp32's normal range to 0, and ga, dist, relu can be large), dist's relative
  error 8u:
      d_sigma_k = da_k e_k dist_k [s_k > 0]:  e_ds = e_da e dist + |da| (e_exp + 8u e) dist + 3u |d_sigma|
      ddist_k   = da_k e_k relu(s_k):         e_dd = e_da e relu + |da| (e_exp + 8u e) relu + 3u |ddist|
  d_rgb_kc = G_c w_k c (1 - c):  |G_c| (e_w_k c (1 - c) + w_k E_SIG) + 4u |d_rgb|
  d_z_k = Gd w_k + n ddist_{k-1} - n ddist_k  (n = |d|):
      e_Gd w + |Gd| e_w + n (e_dd_{k-1} + e_dd_k) + 8u n (|ddist_{k-1}| + |ddist_k|) + 3u |d_z|
  d_rays_d = d (sum_i ddist_i dist_raw_i) / n:  |d| / n (sum_i e_dd_i |dr_i| + (L + 8) u sum_i |ddist_i dr_i|) + 6u |d_rays_d|
Every rounding above is one of fp32's normal range.  Behind an opaque sample w and T reach fp32's denormals (~1e-40), where a
rounding is absolute (2^-150) and a product of such a value with a large factor loses its relative precision: every entry is
held to at least DENORMAL_FLOOR = 2^-110 (7.7e-34) absolute.
NaN and inf: the same entries as torch's.
"""

import math

import torch

import composite_bounds as CB
from oracle import nerf_oracle as O

U = CB.U
DENORMAL_FLOOR = 2.0 ** -110
MIN_NORMAL = 2.0 ** -126
GRADS = ("rgb", "disp", "acc", "depth", "alphas", "weights")
# the upstream gradient sets of the sweep: each output alone, then all six together
GRAD_SETS = [(k,) for k in GRADS] + [GRADS]


def upstream(R, N, which, seed):
    g = torch.Generator().manual_seed(seed)
    n = 0 if N == 1 else N
    shapes = dict(rgb=(R, 3), disp=(R,), acc=(R,), depth=(R,), alphas=(R, n), weights=(R, n))
    out = {k: None for k in GRADS}
    for k in which:
        out[k] = torch.randn(*shapes[k], generator=g, dtype=torch.float64).float()
    if out["disp"] is not None:
        out["disp"] = out["disp"] * 1e-10           # disp reaches 1e10 on transparent rays: keep the products in range
    return out


def reference(raw, z, d, noise, white, G):
    """float64 torch autograd of the oracle's raw2outputs on the fp32 inputs -> (d_raw, d_z, d_rays_d), forward dict"""
    r, zz, dd = (t.double().requires_grad_(True) for t in (raw, z, d))
    n = None if noise is None else noise.double()
    rgb, disp, acc, depth, _, alphas, weights = O.raw2outputs(r, zz, dd, 1.0 if n is not None else 0.0, white, noise=n)
    outs = dict(rgb=rgb, disp=disp, acc=acc, depth=depth, alphas=alphas, weights=weights)
    used = [k for k in GRADS if G[k] is not None and G[k].numel()]
    if used:
        loss = sum((outs[k] * G[k].double()).sum() for k in used)
        gr = torch.autograd.grad(loss, (r, zz, dd), allow_unused=True)
    else:
        gr = (None, None, None)
    gr = [torch.zeros_like(x) if g is None else g for g, x in zip(gr, (r, zz, dd))]
    fwd = {k: v.detach() for k, v in outs.items()}
    return gr, fwd


def _bounds(raw, z, d, noise, white, G, fwd):
    R, N = z.shape
    f64 = torch.float64
    r, zz, dd = raw.double(), z.double(), d.double()
    Gc = G["rgb"].double() if G["rgb"] is not None else torch.zeros(R, 3, dtype=f64)
    c = torch.sigmoid(r[..., :3])
    if N == 1:
        d_rgb = Gc * c[:, 0] * (1 - c[:, 0])
        b_raw = torch.zeros(R, 1, 4, dtype=f64)
        b_raw[:, 0, :3] = Gc.abs() * CB.E_SIG + 4 * U * d_rgb.abs()     # IEEE sigmoid: well inside E_SIG
        return b_raw, torch.zeros(R, 1, dtype=f64), torch.zeros(R, 3, dtype=f64)
    fb = CB._model(raw, z, d, noise, white, fwd)                        # the forward's own error model
    e_alpha, e_w = fb["alphas"], fb["weights"]
    alpha, w, acc, depth = fwd["alphas"], fwd["weights"], fwd["acc"], fwd["depth"]
    keep = 1.0 - alpha + 1e-10
    rho = e_alpha / keep + 3 * U
    i = torch.arange(N, dtype=f64)
    rel_T = torch.cumsum(torch.cat([torch.zeros(R, 1, dtype=f64), rho[:, :-1]], -1), -1) + CB.C_T * (i + torch.ceil(i / 64) + 1) * U
    T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=f64), keep[:, :-1]], -1), -1)
    # per ray
    den = acc + 1e-10
    q = depth / den
    zero = torch.zeros(R, dtype=f64)
    Gd = G["depth"].double() if G["depth"] is not None else zero.clone()
    Ga = G["acc"].double() if G["acc"] is not None else zero.clone()
    if white:
        Ga = Ga - Gc.sum(-1)
    e_Gd, e_Ga = zero.clone(), 3 * U * (Ga.abs() + Gc.abs().sum(-1))
    if G["disp"] is not None:
        qm = torch.clamp(q, min=1e-10)
        disp = 1.0 / qm
        fac = torch.where(q > 1e-10, 1.0, torch.where(q == 1e-10, 0.5, 0.0))
        Gq = -G["disp"].double() * disp * disp * fac
        e_q = fb["depth"] / den + q * (fb["acc"] / den + 7 * U)
        rel_q = e_q / qm + 4 * U
        t1, t2 = Gq / den, Gq * depth / (den * den)
        Gd = Gd + t1
        Ga = Ga - t2
        e_Gd = e_Gd + t1.abs() * (2 * rel_q + fb["acc"] / den + 4 * U)
        e_Ga = e_Ga + t2.abs() * (2 * rel_q + fb["depth"] / depth.abs().clamp(min=1e-300) + 2 * fb["acc"] / den + 6 * U)
    e_Gd = e_Gd + U * Gd.abs()
    Gw = G["weights"].double() if G["weights"] is not None else torch.zeros(R, N, dtype=f64)
    Gal = G["alphas"].double() if G["alphas"] is not None else torch.zeros(R, N, dtype=f64)
    g_abs = Gw.abs() + (Gc.abs()[:, None, :] * c).sum(-1) + Gd.abs()[:, None] * zz.abs() + Ga.abs()[:, None]
    e_g = (Gc.abs().sum(-1) * CB.E_SIG)[:, None] + e_Gd[:, None] * zz.abs() + e_Ga[:, None] + 4 * U * g_abs
    # reverse recurrences
    Uabs = torch.zeros(R, N, dtype=f64)
    eU = torch.zeros(R, N, dtype=f64)
    for k in range(N - 2, -1, -1):
        Uabs[:, k] = keep[:, k + 1] * Uabs[:, k + 1] + g_abs[:, k + 1] * alpha[:, k + 1]
        eU[:, k] = keep[:, k + 1] * eU[:, k + 1] + g_abs[:, k + 1] * e_alpha[:, k + 1] + e_g[:, k + 1] * alpha[:, k + 1]
    eU = eU + rel_T[:, -1:] * Uabs
    L = (math.log2(CB.lane_width(N)) + 2) if N <= 64 else (8 + math.ceil(N / 64))
    has_w = any(G[k] is not None for k in ("rgb", "disp", "acc", "depth", "weights"))
    e_da = Gal.abs() * U
    if has_w:
        e_da = e_da + T * ((rel_T + 3 * U) * (g_abs + Uabs) + e_g + eU) + L * U * T * Uabs
    # |da| itself (float64, from the reference's own pieces)
    Gdv, Gav = Gd[:, None], Ga[:, None]
    GwC = (Gc[:, None, :] * c).sum(-1)
    g = Gw + GwC + Gdv * zz + Gav
    Uv = torch.zeros(R, N, dtype=f64)
    for k in range(N - 2, -1, -1):
        Uv[:, k] = keep[:, k + 1] * Uv[:, k + 1] + g[:, k + 1] * alpha[:, k + 1]
    da = Gal + (T * (g - Uv) if has_w else 0.0)
    sig = r[..., 3] + (noise.double() if noise is not None else 0.0)
    dist_raw = torch.cat([zz[:, 1:] - zz[:, :-1], torch.full((R, 1), 1e10, dtype=f64)], -1)
    n = dd.norm(dim=-1, keepdim=True)
    dist = dist_raw * n
    rl = torch.relu(sig)
    e = torch.exp(-rl * dist)
    s = rl * dist
    e_exp = torch.where(e > 0, e * (2.0 ** -23 * (1.0 + s / math.log(2.0)) + 8 * U * s), torch.zeros_like(e))
    e_exp = torch.where(e < MIN_NORMAL, torch.maximum(e_exp, e), e_exp)     # v_exp_f32 flushes results below 2^-126 to 0
    ds = da * e * dist * (sig > 0)
    ddist = da * e * rl
    pos = (sig > 0).double()
    b_sig = (e_da * e * dist + da.abs() * (e_exp + 8 * U * e) * dist) * pos + 3 * U * ds.abs()
    e_dd = e_da * e * rl + da.abs() * (e_exp + 8 * U * e) * rl + 3 * U * ddist.abs()
    b_raw = torch.zeros(R, N, 4, dtype=f64)
    cc = c * (1 - c)
    b_raw[..., :3] = Gc.abs()[:, None, :] * (e_w[..., None] * cc + w.abs()[..., None] * CB.E_SIG) \
        + 4 * U * (Gc[:, None, :] * w[..., None] * cc).abs()
    b_raw[..., 3] = b_sig
    dpth = G["depth"] is not None or G["disp"] is not None
    prev_dd = torch.cat([torch.zeros(R, 1, dtype=f64), ddist[:, :-1]], -1)
    prev_e = torch.cat([torch.zeros(R, 1, dtype=f64), e_dd[:, :-1]], -1)
    own_dd = torch.cat([ddist[:, :-1], torch.zeros(R, 1, dtype=f64)], -1)
    own_e = torch.cat([e_dd[:, :-1], torch.zeros(R, 1, dtype=f64)], -1)
    dz_mag = (Gdv * w).abs() * dpth + n * (prev_dd.abs() + own_dd.abs())
    b_z = (e_Gd[:, None] * w.abs() + Gdv.abs() * e_w) * dpth + n * (prev_e + own_e) \
        + 8 * U * n * (prev_dd.abs() + own_dd.abs()) + 3 * U * dz_mag
    gn = (ddist * dist_raw)
    b_d = dd.abs() / n * ((e_dd * dist_raw.abs()).sum(-1, keepdim=True) + (L + 8) * U * gn.abs().sum(-1, keepdim=True)) \
        + 6 * U * (dd.abs() / n * gn.sum(-1, keepdim=True).abs())
    return b_raw, b_z, b_d


def check(got, raw, z, d, noise, white, G):
    """got: (d_raw, d_z, d_rays_d) of the kernel.  Raises AssertionError on the first entry out of its bound (or with another
    NaN / inf pattern than torch's); returns {name: (max |err| / bound, max |err|)} over the finite entries."""
    ref, fwd = reference(raw, z, d, noise, white, G)
    bounds = _bounds(raw, z, d, noise, white, G, fwd)
    stats = {}
    for name, gt, x, b in zip(("d_raw", "d_z", "d_rays_d"), got, ref, bounds):
        gt = gt.detach().cpu().double()
        assert gt.shape == x.shape, (name, tuple(gt.shape), tuple(x.shape))
        nan_g, nan_x = torch.isnan(gt), torch.isnan(x)
        assert torch.equal(nan_g, nan_x), (name, "NaN pattern", int((nan_g & ~nan_x).sum()), int((nan_x & ~nan_g).sum()))
        inf_x = torch.isinf(x)
        assert torch.equal(torch.isinf(gt), inf_x) and bool((gt[inf_x] == x[inf_x]).all()), (name, "inf")
        fin = torch.isfinite(x)
        err = (gt[fin] - x[fin]).abs()
        bb = torch.clamp(b[fin].nan_to_num(nan=float("inf")), min=DENORMAL_FLOOR)
        ratio = err / (bb + CB.TINY) if err.numel() else err
        worst = float(ratio.max()) if ratio.numel() else 0.0
        stats[name] = (worst, float(err.max()) if err.numel() else 0.0)
        if worst > 1.0:
            j = int(ratio.argmax())
            raise AssertionError(f"{name}: |err| {float(err[j]):.3e} > bound {float(bb[j]):.3e} (got {float(gt[fin][j])!r}, "
                                 f"ref {float(x[fin][j])!r}; N={z.shape[1]}, white={white}, noise={noise is not None}, "
                                 f"grads={[k for k in GRADS if G[k] is not None]}; worst ratio {worst:.2f})")
    return stats
