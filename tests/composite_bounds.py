"""Compositing (raw2outputs) against float64: the inputs, the reference and the error model with its comparator.

Shared by tests/test_gpu_composite.py (the HIP kernels) and tests/test_composite_bounds.py (float32 mutants of the oracle on
the CPU: the comparator must reject every one of them, so the bounds below are tight enough to mean something).

The error model, in the style of DESIGN.md section 4.2.  u = 2^-24; everything marked _ref is the float64 oracle on the same
fp32 inputs; sample i of a ray of N samples, s_i = relu(sigma_i + noise_i) * dist_i, k_i = 1 - alpha_i + 1e-10 the factor
of the transmittance product, T_i = prod_{j<i} k_j the exclusive transmittance.

  exp(-s) on the transcendental unit, with s from the fp32 dist (z difference, ||d|| as an fma chain and a 1-ulp root,
  the product: |rel err of s| <= 8u):
      e_exp_i   = e^-s_i * (2^-23 (1 + s_i log2 e) + 8u s_i)                        (absolute)
  alpha:  e_alpha_i = e_exp_i + min(u alpha_i, 2 e^-s_i)    (<= 3.2e-7 for every s; the rounding of 1 - exp, which is
                                                               exact below alpha = 1/2 and never more than exp itself)
  k:      rho_i     = e_alpha_i / k_i + 3u         (relative; 1 - alpha, + 1e-10 and fp32(1e-10) each round once.  Behind
                                                   a near-opaque sample k ~ e^-s is far below the rounding of alpha: large)
  T:      rel_T_i   = sum_{j<i} rho_j + C_T (i + ceil(i / 64) + 1) u       (one rounding per factor, per chunk carry, per
                                                                                 carry * exclusive product)
  w:      e_w_i     = T_i e_alpha_i + w_i (rel_T_i + u) + (i + 2) 2^-149    (NOT an absolute tolerance: behind an opaque sample
                                                                                 w is ~1e-10 and this bound scales with it)
  sums, a reduction tree of depth L = log2(SW) + 1 (one chunk) or 6 + chunks (N > 64; the chunk totals are added in order):
      e_acc   = sum_i e_w_i + C_S L u sum_i w_i
      e_depth = sum_i z_i (e_w_i + u w_i) + C_S L u sum_i w_i z_i
      e_rgb   = sum_i (c_i e_w_i + w_i e_sig + u w_i c_i) + C_S L u sum_i w_i c_i  (+ e_acc + u with a white background)
              where c_i = sigmoid of the colour logit and e_sig = 1.5e-7 its bound on the transcendental unit
  disp:   1 / disp against q_ref = max(1e-10, depth / (acc + 1e-10)):
      |1/disp - q_ref| <= e_depth / (acc + 1e-10) + q_ref (e_acc / (acc + 1e-10) + 7u)   (two 1-ulp reciprocals, a product)
      a transparent ray (acc_ref = 0) gives 1e10 to 1 ulp.
  N = 1 (no compositing, rgb = sigmoid(raw) by IEEE expf and division): e_rgb = 4u c.

C_T and C_S are the model's constants: every rounding counted once, first order (both 1).
NaN: the same entries are NaN as in the reference, for every output.
"""

import math

import torch

from oracle import nerf_oracle as O

U = 2.0 ** -24
E_SIG = 1.5e-7            # sigmoid on the transcendental unit (tests/test_gpu_kernels.py, measured 9.3e-8)
TINY = 2.0 ** -149        # one denormal rounding
C_T = 1.0
C_S = 1.0
OUTPUTS = ("rgb", "disp", "acc", "depth", "alphas", "weights")

# every sample count of the sweep: each layout's full range, each multi-chunk case at, below and above a multiple of 64
SWEEP = list(range(1, 71)) + [95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 383, 384, 448, 511, 512, 513, 1000]


def lane_width(N):
    """SW of raw2outputs_kernel for N samples (0: the single-sample kernel)."""
    if N == 1:
        return 0
    sw = 2
    while sw < N and sw < 64:
        sw *= 2
    return sw


def layout_name(N):
    sw = lane_width(N)
    return "single" if sw == 0 else (f"sw{sw}" if N <= 64 else "chunks")


def rays_for(N):
    """3 workgroups and one ray more: a partial last block."""
    sw = max(lane_width(N), 1)
    return 3 * (256 // sw) + 1 if sw > 1 else 3 * 256 + 1


def make_inputs(R, N, seed, with_noise):
    """fp32 inputs mixing every regime within one batch:
    sigma negative, 0, 1e-6, moderate, 1e6 (alpha = 1 exactly); colour logits in +-30; z increasing with uneven gaps and
    duplicate depths (dist = 0); ||d|| in [0.3, 3]; every 8th ray fully transparent, every 8th (offset 2) opaque at sample 0,
    every 8th (offset 3) thin (transmittance left at the end); ray 5 has a NaN sigma in the middle, ray 6 a +inf one."""
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64

    def rnd(*shape):
        return torch.rand(*shape, generator=g, dtype=f64)

    d = torch.randn(R, 3, generator=g, dtype=f64)
    d = d / d.norm(dim=-1, keepdim=True) * (0.3 * 10.0 ** rnd(R, 1))
    gap = rnd(R, N) ** 2 * (4.0 / N)
    gap[rnd(R, N) < 0.08] = 0.0
    gap[:, 0] = 0.0
    z = 2.0 + rnd(R, 1) + torch.cumsum(gap, -1)
    cat = rnd(R, N)
    sigma = 10.0 ** (rnd(R, N) * 3.5 - 3.0) * N                    # s = sigma * dist from ~1e-3 to ~3
    sigma = torch.where(cat < 0.15, -10.0 * rnd(R, N), sigma)
    sigma = torch.where((cat >= 0.15) & (cat < 0.25), torch.zeros_like(sigma), sigma)
    sigma = torch.where((cat >= 0.25) & (cat < 0.35), torch.full_like(sigma, 1e-6), sigma)
    sigma = torch.where(cat >= 0.97, torch.full_like(sigma, 1e6), sigma)
    kind = torch.arange(R) % 8
    sigma[kind == 1] = -sigma[kind == 1].abs()                      # transparent
    sigma[kind == 3] = 1e-3 * sigma[kind == 3].abs()                # thin
    sigma[kind == 2, 0] = 1e6                                        # opaque at sample 0
    if R > 6:
        sigma[5, N // 2] = float("nan")
        sigma[6, N // 2] = float("inf")
    raw = torch.empty(R, N, 4, dtype=f64)
    raw[..., :3] = (rnd(R, N, 3) * 2.0 - 1.0) * 30.0
    raw[..., 3] = sigma
    noise = None
    if with_noise:
        noise = torch.randn(R, N, generator=g, dtype=f64)
        noise[kind == 1] = -noise[kind == 1].abs()                  # transparent stays transparent
        noise = noise.float()
    return raw.float(), z.float(), d.float(), noise


def reference(raw, z, d, noise, white):
    """The oracle in float64 on the fp32 inputs, plus what the bounds need."""
    r, zz, dd = raw.double(), z.double(), d.double()
    n = None if noise is None else noise.double()
    rgb, disp, acc, depth, _, alphas, weights = O.raw2outputs(r, zz, dd, 1.0 if n is not None else 0.0, white, noise=n)
    return dict(rgb=rgb, disp=disp, acc=acc, depth=depth, alphas=alphas, weights=weights)


def _model(raw, z, d, noise, white, ref):
    """Per-element bounds of the error model above (float64)."""
    R, N = z.shape
    r, zz, dd = raw.double(), z.double(), d.double()
    if N == 1:
        c = torch.sigmoid(r[:, 0, :3])
        return dict(rgb=4 * U * c + TINY, acc=torch.zeros(R, dtype=torch.float64), depth=torch.zeros(R, dtype=torch.float64),
                    alphas=torch.zeros(R, 0, dtype=torch.float64), weights=torch.zeros(R, 0, dtype=torch.float64))
    sig = r[..., 3] + (noise.double() if noise is not None else 0.0)
    dist = torch.cat([zz[:, 1:] - zz[:, :-1], torch.full((R, 1), 1e10, dtype=torch.float64)], -1) * dd.norm(dim=-1, keepdim=True)
    s = torch.relu(sig) * dist
    e = torch.exp(-s)
    e_exp = torch.where(e > 0, e * (2.0 ** -23 * (1.0 + s / math.log(2.0)) + 8 * U * s), torch.zeros_like(e))
    alpha = ref["alphas"]
    e_alpha = e_exp + torch.minimum(U * alpha.abs(), 2.0 * e.nan_to_num(0.0))
    k = 1.0 - alpha + 1e-10
    rho = e_alpha / k + 3 * U
    i = torch.arange(N, dtype=torch.float64)
    n_round = i + torch.ceil(i / 64) + 1
    rel_T = torch.cumsum(torch.cat([torch.zeros(R, 1, dtype=torch.float64), rho[:, :-1]], -1), -1) + C_T * n_round * U
    T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=torch.float64), k[:, :-1]], -1), -1)
    w = ref["weights"]
    e_w = T * e_alpha + w.abs() * (rel_T + U) + (i + 2) * TINY
    sw = lane_width(N)
    L = (math.log2(sw) + 1) if N <= 64 else (6 + math.ceil(N / 64))
    c = torch.sigmoid(r[..., :3])
    e_acc = e_w.sum(-1) + C_S * L * U * w.abs().sum(-1)
    e_depth = (zz * (e_w + U * w.abs())).sum(-1) + C_S * L * U * (w.abs() * zz).sum(-1)
    e_rgb = (c * e_w[..., None] + w.abs()[..., None] * E_SIG + U * w.abs()[..., None] * c).sum(-2) \
        + C_S * L * U * (w.abs()[..., None] * c).sum(-2)
    if white:
        e_rgb = e_rgb + (e_acc + U)[:, None]
    return dict(rgb=e_rgb, acc=e_acc, depth=e_depth, alphas=e_alpha, weights=e_w)


def _check_one(name, g, x, bound, tag):
    """One output against its reference and per-element bound: (max |err| / bound, max |err|) over the finite entries"""
    assert g.shape == x.shape, (name, tuple(g.shape), tuple(x.shape))
    assert torch.equal(torch.isnan(g), torch.isnan(x)), (name, "NaN pattern", int((torch.isnan(g) ^ torch.isnan(x)).sum()))
    fin = torch.isfinite(x)
    assert torch.equal(torch.isinf(g), torch.isinf(x)) and bool((g[torch.isinf(x)] == x[torch.isinf(x)]).all()), (name, "inf")
    err = (g[fin] - x[fin]).abs()
    ratio = err / (bound[fin] + TINY) if err.numel() else err
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        j = int(ratio.argmax())
        raise AssertionError(f"{name}: |err| {float(err[j]):.3e} > bound {float(bound[fin][j]):.3e} "
                             f"(got {float(g[fin][j])!r}, ref {float(x[fin][j])!r}; {tag}; worst ratio {worst:.2f})")
    return worst, float(err.max()) if err.numel() else 0.0


def _check_disp(g, ref, b, N, white):
    """disp: 1 / disp against max(1e-10, depth / (acc + 1e-10)); transparent rays exactly the clamp"""
    x = ref["disp"]
    assert torch.equal(torch.isnan(g), torch.isnan(x)), ("disp", "NaN pattern")
    fin = torch.isfinite(x)
    acc = ref["acc"]
    q = 1.0 / x
    if N == 1:
        e_q = torch.zeros_like(q)
    else:
        den = acc + 1e-10
        e_q = b["depth"] / den + q * (b["acc"] / den + 7 * U)
    clear = fin & (acc == 0)
    one_ulp = float(torch.tensor(1e10, dtype=torch.float32).nextafter(torch.tensor(2e10)) - torch.tensor(1e10, dtype=torch.float32))
    assert bool(((g[clear] - 1e10).abs() <= one_ulp).all()), ("disp", "transparent rays", g[clear][:4].tolist())
    sel = fin & ~clear
    err = (1.0 / g[sel] - q[sel]).abs()
    ratio = err / (e_q[sel] + 4 * U * q[sel])  # (+ the fp32 rounding of disp itself, 2u relative through the reciprocal)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        j = int(ratio.argmax())
        raise AssertionError(f"disp: |1/disp err| {float(err[j]):.3e} over its bound (N={N}, white={white}; ratio {worst:.2f})")
    return worst, float(err.max()) if err.numel() else 0.0


def _check(names, got, raw, z, d, noise, white, ref):
    if ref is None:
        ref = reference(raw, z, d, noise, white)
    b = _model(raw, z, d, noise, white, ref)
    N = z.shape[1]
    tag = f"N={N}, white={white}, noise={noise is not None}"
    stats = {name: _check_one(name, got[name], ref[name], b[name], tag) for name in names}
    stats["disp"] = _check_disp(got["disp"], ref, b, N, white)
    return stats


def check(got, raw, z, d, noise, white, ref=None):
    """got: the six outputs (float32, any device).  Raises AssertionError naming the first output out of its bound; returns
    {output: (max |err| / bound, max |err|)} over the finite entries."""
    got = dict(zip(OUTPUTS, (x.detach().cpu().double() if x is not None else None for x in got)))
    return _check(("alphas", "weights", "acc", "depth", "rgb"), got, raw, z, d, noise, white, ref)


def check_maps(got, raw, z, d, noise, white, ref=None):
    """The same for a renderer that returns the per-ray maps only: got = dict(rgb [R, 3], disp, acc, depth [R])."""
    got = {k: got[k].detach().cpu().double() for k in ("rgb", "disp", "acc", "depth")}
    return _check(("acc", "depth", "rgb"), got, raw, z, d, noise, white, ref)
