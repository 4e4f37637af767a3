"""The depth-tangent renderer (ns_render_rays_fused_tangent, ns_tangent.h) against float64 on fields with one right answer.

Shared by tests/test_exact_tangent_host.py (the conditions T1 - T5 below, the float64 reference against torch autograd, an fp32
transcription of the kernel's walk against the error model, the mutants) and tests/test_gpu_exact_tangent.py (the HIP kernels).
Nothing here calls the library.

The field is an "identity" network of exact_field.make_exact_nerf (every sine and cosine column has weight zero), evaluated on
points that are short dyadic numbers.  It is piecewise linear in the point, every sum is exact in fp32 in any order and every
ReLU pre-activation is a multiple of its layer's quantum: `raw` AND d raw / d m -- the chain of masked weight matrices applied
to the ray direction -- are exact in fp32, in hi + lo f16 tiles and, on most rays, in plain f16 tiles.  All a kernel can differ
by from float64 is the fp32 arithmetic of walk_samples and write_jacobian, and every ray is held to the bound derived below:
no kink exemption, no share of rays left out.

Pools.  A: 32 rays, o multiples of 1/4 in [-2, 2], d from {0, +-1/2, +-1}, view directions multiples of 1/4, the 17 depths
2, 2.25, .., 6 (544 rows).  B: the 33 depths in steps of 1/8 with d from {0, +-1}.  The heads (alpha_linear, rgb_linear) are
scaled by 2^-5, weights and biases: unscaled sigma reaches ~100 and every ray is opaque after one sample.

Placement on the pool's depths at every supported N: with step = 1/4 (B: 1/8) and std = step (N - 2) / 2 (N = 2: std = step)
linspace(-std, std, N - 1) has the fp32 step `step` exactly, so with m a multiple of `step` every unclipped depth is a pool
depth, every clipped one is 2 or 6 (dz = 0, and dist = 0 between equal depths), and the window of unclipped samples slides
along the ray with m: `means(N, step)` puts it at the ray's start, its end, across every multiple of 64, wholly inside every
chunk, with the merged mean inside [2, 6], below 2 and above 6, and with samples exactly on 2 and on 6.

The conditions (check_t1 .. check_t5; the host test asserts them for every case the GPU test walks):
  T1  C1 - C3 of exact_field.py hold for the scaled network on the pool, and every sample of every case is a pool row;
  T2  every tangent activation (the direction, each layer's dh, the folded view layer's) splits exactly into hi = fl16(x),
      lo = fl16(x - hi) (f16x3), and d raw is an fp32 number; for the f16 instance each of those activations is itself an f16
      number (normal or zero) -- d raw is an fp32 accumulator in both instances.  A ray that fails the f16 form is left out of
      the f16 cases only; at most a quarter of a network's rays may fail it, the f16x3 and one-sample cases drop none;
  T3  in every tangent GEMM sum_k |w_k dh_k| / q < 2^24, q the product of the operands' quanta;
  T4  in every case at least a quarter of the rays have |J_c| > 100 bound_c in every column c not zero by rule;
  T5  every mutant of MUTANTS moves some entry of J by more than twice its bound on every case it applies to.

The error model (u = 2^-24; first order, every fp32 rounding of walk_samples / write_jacobian counted once; on top of
composite_bounds.py's e_exp, e_alpha, rho, rel_T and E_SIG; everything else is the float64 reference on the same fp32 inputs).
Per sample, with s = relu(sigma) dist, e = exp(-s), dist and d dist = (dz_{j+1} - dz_j) |d| carrying 8u (|d| as an fma chain
and a 1-ulp root, one product):
  e_exp, e_alpha, rho   composite_bounds.py's; for s == 0 exactly the transcendental unit returns exp2(0) = 1, 1 - 1 = 0 and
                        1 - 0 + 1e-10f rounds to 1: e_alpha = 0 and the factor's relative error is the dropped 1e-10
  D = dist dsigma [sigma > 0] + relu(sigma) ddist:   e_D = 9u (|.| + |.|) + u |D|          (8u and a product each, one sum)
  dalpha = e D:          e_dalpha = e_exp |D| + e e_D + u |dalpha|
  c = sigmoid(raw_c):    E_SIG;   c (1 - c):  e_cc = E_SIG |1 - 2c| + 2u c (1 - c);   dc = c (1 - c) draw_c:  e_cc |draw_c| + u |dc|
  T (relative):          rel_T = 1u + sum_{i<j} (rho_i + u) + u per 64 samples passed   (one rounding per factor, one per
                         carried state; a factor that is exactly 1 -- a zero-dist sample -- rounds nothing)
  w = alpha T:           e_w = T e_alpha + w (rel_T + u)
  dw = T dalpha + alpha dT:   e_dw = T e_dalpha + |T dalpha| rel_T + alpha e_dT + |dT| e_alpha + 2u (|T dalpha| + |alpha dT|)
  dT' = keep dT - T dalpha:   e_dT' = keep e_dT + |dT| (e_alpha + 3u keep) + T e_dalpha + |T dalpha| rel_T
                                      + 2u (|keep dT| + |T dalpha|)
  the sums are sequential.  A term t_j = x dw + w dx has e_t = e_x |dw| + x e_dw + w e_dx + |dx| e_w + 2u (|x dw| + |w dx|)
  (x = c, z or 1: e_z = 0), and each addition rounds the running sum: u sum_{i<=j} |t_i| per sample j that adds a non-zero
  term (depth N).  The primal sums the walk carries for disp (depth, acc) are bounded the same way.
write_jacobian:
  white background:  d rgb - d acc:  e_drgb + e_dacc + u |J|
  inv = rcp(acc + 1e-10): rel_inv = e_acc / den + 4u (the sum, fp32(1e-10), a 1-ulp reciprocal);  q = depth inv:
  e_q = e_depth inv + q (rel_inv + u);  dq = inv (ddepth - q dacc):
      e_dq = inv (e_ddepth + |dacc| e_q + q e_dacc + 2u (|ddepth| + |q dacc|)) + |dq| (rel_inv + u)
  disp = rcp(max(1e-10, q)): rel_disp = e_q / q + 2u;  d disp = -disp^2 dq:  disp^2 e_dq + |d disp| (2 rel_disp + 2u); where
  q is within e_q of 1e-10 the branch may differ and the whole |disp^2 dq| is allowed.
Two inputs per sample and colour channel, zero on these fields (tests/exact_tangent_probes.py sets them): e_raw_c and e_draw_c,
what the kernel's raw_c and d raw_c may differ by from the tables; they enter c, c (1 - c) and dc to first order (jacobian64).
Every entry is held to at least DENORMAL_FLOOR (composite_backward_bounds.py).  No constant is fitted to a kernel.
One sample per ray (raw2outputs' N == 1 rule): |d rgb - ref| <= 6u |ref| + |d raw| E, E = 4u c the IEEE sigmoid's bound.

The mutants are faults of the reference: `jacobian64(..., mutant=name)`.  Three of them change nothing any fp32 kernel could
show on these fields, and `applies` says so: "ddist_last" (the last sample's exp(-sigma 1e10 |d|) is 0 for every positive
sigma a network with quantum 2^-9 produces, and relu(sigma) is 0 otherwise), "keep_no_eps" (keep >= 0.1 on every sample but
the last: 1e-10 is 1e-9 of it, far below u) and "disp_tie" (q = depth / acc is 0 or >= 2, never 1e-10).

Measured worst |J - J64| / bound over every case (the tests print it per instance and network):
  MI355X   f16x3 0.287 (d9w256, N = 4), f16 0.389 (prod, N = 4), one sample per ray 0.359 (prod); per network the f16x3
           instance 0.12 .. 0.29, the f16 one 0.12 .. 0.39, the one-sample one 0.23 .. 0.36 (d9w256 on pool B: 0.227, 0.227,
           0.252); the primal maps 0.16 of composite_bounds.py's bound (one sample: 0.47 of 4u c)
  CPU      the fp32 transcription `walk_fp32` (torch fp32, its exp and sigmoid) over every case of both instances:
           0.115 .. 0.389 per network (prod, N = 4: the same ray as the f16 kernel's worst)
  T3       the worst tangent GEMM: 2^16.8 (prod, d9w256 on pool A; d9w256 on pool B 2^14.6); the f16 form keeps 30 / 32 rays of
           prod, 24 / 32 of d9w256 on pool A, 31 / 32 of d9w256 on pool B, all of the rest
  pool B   draws for prod, d2w128, d5w128s03 and d9w256 with the second draw of the pool's rays
"""

import math

import numpy as np
import torch

import composite_bounds as CB
import exact_field as E

U = CB.U
E_SIG = CB.E_SIG
DENORMAL_FLOOR = 2.0 ** -110
MIN_NORMAL = 2.0 ** -126
HEAD_SCALE = 2.0 ** -5
NEAR, FAR = 2.0, 6.0
POOL_RAYS = 32
# salt: pool B's first draw of rays fits d2w128 and d9w256 only; this one fits every network of the table, prod included
POOLS = {"A": dict(step=0.25, dirs=(0.0, 0.5, -0.5, 1.0, -1.0), salt=0), "B": dict(step=0.125, dirs=(0.0, 1.0, -1.0), salt=1000)}
ALL_N = (2, 4, 8, 16, 32, 64, 128, 192, 256, 512)
RAY_COUNTS = (1, 2, 3, 5, 33, 67)
SINGLE_COUNTS = (1, 63, 64, 65, 257)
REQUIRED = ("prod", "d2w128")
# (network, pool) pairs the tests walk; the library decides which of them it accepts (d9w256 takes 17 s to draw on pool B)
TABLE = [(name, "A") for name in E.NETWORKS if E.NETWORKS[name]["use_viewdirs"]] \
    + [("prod", "B"), ("d2w128", "B"), ("d5w128s03", "B"), ("d9w256", "B")]
INSTANCES = ("f16x3", "f16", "single")          # f16x3 handle; f16 handle, approximate=True; f16x3 handle, mode="depth_only"
GROUP = {"f16x3": 64, "f16": 128}               # samples of a workgroup's group
COLS = ("r", "g", "b", "disp", "depth", "acc")
MUTANTS = ("dz_open", "slot_off", "ddist_dropped", "ddist_last", "relu_sigma0", "dT_new_T", "keep_no_eps", "reset64", "reset128",
           "reset_second", "skip_d_dropped", "view_dir_tangent", "mask_above", "white_dropped", "disp_tie", "draw_order")
NET_MUTANTS = ("skip_d_dropped", "view_dir_tangent", "mask_above", "draw_order")
NEVER = ("ddist_last", "keep_no_eps", "disp_tie")


def depths(which):
    step = POOLS[which]["step"]
    return NEAR + step * np.arange(int(round((FAR - NEAR) / step)) + 1)


def std_of(N, step):
    return step * (N - 2) / 2 if N > 2 else step


# ---- pools and networks ---------------------------------------------------------------------------------------------
def make_tangent_pool(seed, which):
    """(pool [32 K, 90], dict(o, d, z, viewdirs)): row r K + k is ray r at depth z[k]."""
    z = depths(which)
    K = len(z)
    rng = np.random.default_rng(seed + 104729 * (1 + "AB".index(which)) + POOLS[which]["salt"])
    pool = E.make_pool(seed, True, POOL_RAYS * K)
    o = rng.integers(-8, 9, size=(POOL_RAYS, 3)).astype(np.float64) / 4
    d = rng.choice(np.array(POOLS[which]["dirs"]), size=(POOL_RAYS, 3))
    d[np.all(d == 0, axis=1), 0] = 1.0
    v = rng.integers(-4, 5, size=(POOL_RAYS, 3)).astype(np.float64) / 4
    pool[:, 0:3] = (o[:, None, :] + d[:, None, :] * z[None, :, None]).reshape(-1, 3)
    pool[:, E.IN_PTS:E.IN_PTS + 3] = np.repeat(v, K, axis=0)
    return pool, dict(o=o, d=d, z=z, viewdirs=v)


_cache = {}


def network(name, which="A"):
    """The cached identity network of E.NETWORKS[name] drawn on pool `which`, heads scaled by 2^-5, with its tangent tables:
    net["G"] [P, 4] = d (r, g, b, sigma) / d z of every pool row."""
    key = (name, which)
    if key not in _cache:
        pool, rays = make_tangent_pool(E.NETWORKS[name]["seed"], which)
        net = dict(E.make_exact_nerf(columns="identity", pool=pool, **E.NETWORKS[name]))
        net["rays"], net["name"], net["which"], net["step"] = rays, name, which, POOLS[which]["step"]
        scale = {"alpha", "rgb"}
        net["weights"] = [w * HEAD_SCALE if n in scale else w for n, w in zip(net["names"], net["weights"])]
        net["biases"] = [b * HEAD_SCALE if n in scale else b for n, b in zip(net["names"], net["biases"])]
        net["raw"] = E.chain(net, pool)
        net["G"], net["acts"], net["outs"] = tangent_chain(net)
        net["Gm"] = {}
        _cache[key] = net
    return _cache[key]


def tangent_chain(net, mutant=None):
    """d raw / d z of every pool row by the literal chain, dh_{l+1} = [pre_l > 0] (W_l dh_l) from dh_0 = [d, 0 ..]: the skip layer
    sees [d, dh], the view layer [dh_feature, 0].  Returns (G [P, 4] in the order r, g, b, sigma; the tangent GEMMs as the
    kernels run them, [(name, weights, tangent input)]; the tangent activations the kernels hold in operand tiles)."""
    x = net["pool"]
    P, K = x.shape[0], len(net["rays"]["z"])
    d = np.repeat(net["rays"]["d"], K, axis=0)
    _, seen = E.chain(net, x, keep=True)
    w = dict(zip(net["names"], net["weights"]))
    dx = np.zeros((P, E.IN_PTS))
    dx[:, :3] = d
    acts, outs, dh, D = [], [dx], dx, net["D"]
    for i in range(D):
        name = f"pts{i}"
        acts.append((name, w[name], dh))
        pre = seen[f"pts{i + 1}"][1] if (mutant == "mask_above" and i + 1 < D) else seen[name][1]
        dh = (pre > 0) * (dh @ w[name].T)
        outs.append(dh)
        if i in net["skips"]:
            dh = np.concatenate([np.zeros_like(dx) if mutant == "skip_d_dropped" else dx, dh], axis=1)
    acts.append(("alpha", w["alpha"], dh))
    dsig = dh @ w["alpha"].T
    dv = np.zeros((P, E.IN_VIEWS))
    if mutant == "view_dir_tangent":
        dv[:, :3] = d
    mask = seen["views"][1] > 0
    dhv = mask * (np.concatenate([dh @ w["feature"].T, dv], axis=1) @ w["views"].T)
    wf, _ = E.fold_views(net)
    vin = np.concatenate([dh, dv], axis=1)
    acts.append(("views", wf, vin))
    if mutant is None:
        assert (mask * (vin @ wf.T) == dhv).all(), "the folded view layer's tangent is not the literal chain's"
    outs.append(dhv)
    acts.append(("rgb", w["rgb"], dhv))
    G = np.concatenate([dhv @ w["rgb"].T, dsig], axis=1)
    if mutant is None:                 # the sums of magnitudes behind G: what a float64 evaluation in another order may differ by
        net["Gabs"] = np.concatenate([np.abs(dhv) @ np.abs(w["rgb"]).T, np.abs(dh) @ np.abs(w["alpha"]).T], axis=1)
    if mutant == "draw_order":
        G = G[:, [3, 0, 1, 2]]
    return G, acts, outs


def _G(net, mutant):
    if mutant not in NET_MUTANTS:
        return net["G"]
    if mutant not in net["Gm"]:
        net["Gm"][mutant] = tangent_chain(net, mutant)[0]
    return net["Gm"][mutant]


# ---- the conditions -------------------------------------------------------------------------------------------------
def check_t1(net, cases=()):
    """C1 - C3 for the scaled network on its pool (C1 without exact_field's coefficient set: the heads are scaled by a power of
    two); every sample depth of every case is a pool depth."""
    for name, w, b, _, _ in E.kernel_layers(net):
        assert E.fits16(w).all() and E.is_f32(b), f"T1 (C1): {name}"
    for name, w, b in zip(net["names"], net["weights"], net["biases"]):
        assert E.fits16(w).all() and E.is_f32(b), f"T1 (C1): {name}"
    E.check_c2(net)
    worst = E.check_c3(net)
    grid = set(net["rays"]["z"].tolist())
    for case in cases:
        mean = case["mean"][np.isfinite(case["mean"])]
        if case["N"] == 1:
            assert set(mean.tolist()) <= grid, "T1: a one-sample depth is no pool depth"
            continue
        z = place64(mean, case["N"], net["step"])[0]
        assert set(np.unique(z).tolist()) <= grid, f"T1: N = {case['N']}: a sample depth is no pool depth"
    return worst


def _split_exact(x):
    hi, lo = E.split(x)
    return E.is_f32(x) and bool((hi + lo == x).all())


def _is_f16(x):
    x = np.asarray(x, dtype=np.float64)
    return (E.half(x) == x) & ((x == 0) | (np.abs(x) >= 2.0 ** -14))


def check_t2(net):
    """Returns the pool rays [32] that keep the f16 form; asserts the f16x3 form on every ray and the cap of a quarter."""
    K = len(net["rays"]["z"])
    ok16 = np.ones(POOL_RAYS, dtype=bool)
    for x in net["outs"]:
        assert _split_exact(x), "T2: a tangent activation is not hi + lo"
        ok16 &= _is_f16(x).all(axis=1).reshape(POOL_RAYS, K).all(axis=1)
    assert E.is_f32(net["G"]), "T2: d raw is no fp32 number"
    assert (~ok16).sum() <= POOL_RAYS // 4, f"T2: {int((~ok16).sum())} of {POOL_RAYS} rays fail the f16 form"
    return ok16


def check_t3(net):
    """sum_k |w_k dh_k| / q < 2^24 in every tangent GEMM, plain and over the hi / lo parts.  Returns the largest ratio."""
    worst = 0.0
    for name, w, x in net["acts"]:
        if not x.any():
            continue
        xh, xl = E.split(x)
        for parts in ([x], [xh, xl]):
            parts = [p for p in parts if p.any()]
            total = float((sum(np.abs(p) for p in parts) @ np.abs(w).T).max())
            q = E.quantum(w) * min(E.quantum(p) for p in parts)
            assert total < 2.0 ** 24 * q, f"T3: {name}: {total} on quantum {q}"
            worst = max(worst, total / q)
    return worst


def check_t4(ref):
    """At least a quarter of the case's rays have |J_c| > 100 bound_c, in every column that is not zero by rule."""
    J, b = ref["J"], ref["bound"]
    live = range(3) if ref["N"] == 1 else range(6)
    for c in live:
        seen = int((np.abs(J[:, c]) > 100.0 * b[:, c]).sum())
        assert 4 * seen >= J.shape[0], f"T4: N = {ref['N']}, column {COLS[c]}: {seen} of {J.shape[0]} rays visible"


def applies(mutant, net, case, ref, instance="f16x3"):
    """Whether the fault `mutant` changes anything an fp32 evaluation of `case` could show (see the head of this file)."""
    N = case["N"]
    if mutant in NEVER:
        return False
    if mutant in NET_MUTANTS:          # the fault changes d raw on some sample of the case (N = 1: d raw rgb)
        keep = np.flatnonzero(np.isfinite(case["mean"]))
        if N == 1:
            rows = _rows(net, case["ray"][keep], case["mean"][keep][:, None])
            return bool((_G(net, mutant)[rows][..., :3] != net["G"][rows][..., :3]).any())
        S = ref["samples"]
        rows = _rows(net, S["ray"], S["z"])
        return bool(((_G(net, mutant)[rows] != net["G"][rows]) & (S["dz"][..., None] > 0)).any())
    if N == 1:
        return False
    if mutant == "slot_off":       # the fault moves a sample that has density (before or after) and that the ray still sees
        S, M = ref["samples"], samples64(net, case, mutant)
        lit = (S["raw"][..., 3] > 0) | (M["raw"][..., 3] > 0)
        return bool(((S["z"] != M["z"]) & lit & (ref["T"] >= 0.01)).any())
    if mutant == "dz_open":
        return bool(ref["on_bound"])
    if mutant == "relu_sigma0":
        return bool(ref["sigma0"])
    if mutant == "reset64":
        return N > 64
    if mutant == "reset128":
        return N > 128
    if mutant == "reset_second":
        return instance == "f16" and N % GROUP["f16"] != 0 and N > GROUP["f16"] and case["mean"].shape[0] > 1
    if mutant == "white_dropped":
        return bool(case["white"]) and bool(ref["open_end"])
    # relu(sigma) ddist != 0 on a sample the ray still sees, at the near bound: at the far bound the samples behind it sit on the
    # same point with dist = 0 up to the last one, which is opaque exactly where sigma(6) > 0 -- the weight ddist moves stays
    # on one point, one colour and one depth (as between the two samples of N = 2)
    if mutant == "ddist_dropped":
        return bool(ref["ddist_live"])
    if mutant == "dT_new_T":           # a sample that changes dT (alpha dalpha != 0) in front of one that has opacity
        return bool(ref["dT_live"])
    return True


def check_t5(net, case, ref, instance="f16x3", mutants=MUTANTS):
    """Every mutant that applies moves some J entry by more than twice its bound.  Returns {mutant: worst move / bound}."""
    out = {}
    for mutant in mutants:
        if not applies(mutant, net, case, ref, instance):
            continue
        got = jacobian64(net, case, mutant=mutant, instance=instance)["J"]
        move = float((np.abs(got - ref["J"]) / ref["bound"]).max())
        assert move > 2.0, f"T5: {mutant} moves J by {move:.3g} of its bound only (N = {case['N']}, {net['name']}, pool {net['which']})"
        out[mutant] = move
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------
def means(N, step):
    """The depths m of a case's rays: 2 + std - s step puts the first unclipped grid sample at index s (a window of
    4 / step + 1 grid samples; the merged mean joins it where it lies in [2, 6])."""
    std = std_of(N, step)
    win = int(round((FAR - NEAR) / step))          # the window's last grid sample is s + win
    last = N - 2                                   # the last grid index
    starts = {0, last - win, -(win // 2), last - win // 2, last // 2 - win // 2, 1, last - win - 1}
    for B in range(64, N, 64):
        starts |= {B - win // 2, B - 1, B - win}
    for c in range(0, N, 64):
        if c + 20 + win < min(N, c + 64):
            starts.add(c + 20)
    out = []
    for s in sorted(starts):
        m = NEAR + std - s * step
        a0, a1 = m - std, m + std
        if a1 >= NEAR and a0 <= FAR:               # some sample stays inside
            out.append(m)
    out += [NEAR, FAR, 4.0, NEAR - step, FAR + step]          # the merged mean on a bound, inside, just outside
    if 2 * std < FAR - NEAR:                                   # every sample fits inside: five depths at which they all do
        lo, hi = NEAR + std, FAR - std
        out += [lo + step * round(k * (hi - lo) / (4 * step)) for k in range(5)]
    return np.array(sorted(set(out)), dtype=np.float64)


def allowed_rays(net, instance):
    """The pool rays an instance may use: all of them, for f16 those that keep T2's f16 form."""
    if "ok16" not in net:
        net["ok16"] = check_t2(net)
    return np.flatnonzero(net["ok16"]) if instance == "f16" else np.arange(POOL_RAYS)


def case_rays(net, instance, mean, N, offset, few=False):
    """A pool ray for every depth of `mean`.  d acc is -dT behind the last sample, ~1e-10 where that sample's sigma is
    positive (its alpha is 1), and nothing shows on a ray without density: slot i takes a ray whose last sample has sigma > 0
    where i % 3 == 2, and otherwise one whose last sample has sigma <= 0 and that has a positive sigma on some earlier sample
    with a step behind it (any ray where the pool has none), so that most of a case's rays show every column."""
    allowed = allowed_rays(net, instance)
    K = len(net["rays"]["z"])
    sg = net["raw"][:, 3].reshape(POOL_RAYS, K)[allowed]
    m = np.nan_to_num(mean, nan=4.0)
    if N == 1:
        return allowed[(offset + 5 * np.arange(len(mean))) % len(allowed)]
    z = place64(m, N, net["step"])[0]
    k = np.rint((z - NEAR) / net["step"]).astype(np.int64)
    sgk = sg[:, k]                                                        # [rays, R, N]
    lit = ((sgk[:, :, :-1] > 0) & (z[:, 1:] > z[:, :-1])[None]).any(axis=-1)
    open_ = (sgk[:, :, -1] <= 0) & lit
    closed = sgk[:, :, -1] > 0
    out = np.zeros(len(mean), dtype=np.int64)
    for i in range(len(mean)):
        first, second = (closed, open_) if i % 3 == 2 and not few else (open_, closed)
        cand = np.flatnonzero(first[:, i])
        if not len(cand):
            cand = np.flatnonzero(second[:, i])
        if not len(cand):
            cand = np.arange(len(allowed))
        out[i] = allowed[cand[(offset + 5 * (i // 3)) % len(cand)]]
    return out


def open_pairs(net, instance, N, limit=8):
    """Up to `limit` (depth, pool ray) pairs at which every sample lies inside [2, 6], the ray's last sample has sigma <= 0 and an
    earlier one sigma > 0: the rays that show d acc.  A network with little empty space (d2w128) has few of them at small N, and
    `case_rays` would meet them only by chance."""
    step, std = net["step"], std_of(N, net["step"])
    if 2 * std >= FAR - NEAR:
        return []
    allowed = allowed_rays(net, instance)
    sg = net["raw"][:, 3].reshape(POOL_RAYS, -1)[allowed]
    ms = NEAR + std + step * np.arange(int(round((FAR - NEAR - 2 * std) / step)) + 1)
    z = place64(ms, N, step)[0]
    sgk = sg[:, np.rint((z - NEAR) / step).astype(np.int64)]
    good = (sgk[:, :, -1] <= 0) & ((sgk[:, :, :-1] > 0) & (z[:, 1:] > z[:, :-1])[None]).any(axis=-1)
    pairs = [(ms[i], allowed[r]) for i in range(len(ms)) for r in np.flatnonzero(good[:, i])]
    pairs = pairs[:: max(1, -(-len(pairs) // limit))][:limit]
    return (pairs * 6)[:6] if 0 < len(pairs) < 6 else pairs          # (so few that they repeat: still a quarter of a case)


def _shows(ref):
    """T4 as a predicate"""
    try:
        check_t4(ref)
        return True
    except AssertionError:
        return False


def cases(net, instance):
    """The cases of one (network, instance): dicts N, white, ray [R] (pool rays), mean [R] (float64 values that are fp32
    numbers; NaN for the ray without a depth), kind ("main": every mean of `means`, the pairs of `open_pairs`, a NaN ray and an
    all-clipped ray; "count": the ray counts, with both where there are three rays or more)."""
    step = net["step"]
    out = []
    if instance == "single":
        z = net["rays"]["z"]
        for i, R in enumerate(SINGLE_COUNTS):
            m = z[(3 * np.arange(R) + i) % len(z)]
            out.append(dict(N=1, white=bool(i & 1), ray=case_rays(net, instance, m, 1, i), mean=m, kind="main"))
        return out
    for ni, N in enumerate(ALL_N):
        ms = means(N, step)
        pairs = open_pairs(net, instance, N)
        full = np.concatenate([ms[: len(ms) // 2], [np.nan, NEAR - std_of(N, step) - 1.0], ms[len(ms) // 2:]])
        ray = case_rays(net, instance, full, N, ni)
        if pairs:
            full = np.concatenate([full, [m for m, _ in pairs]])
            ray = np.concatenate([ray, [r for _, r in pairs]])
        for white in (True, False):
            out.append(dict(N=N, white=white, ray=ray, mean=full, kind="main"))
        mid = ms[np.argsort(np.abs(ms - 4.0), kind="stable")]          # the depths nearest the middle first
        for ci, R in enumerate(RAY_COUNTS):
            dead = () if R < 3 else (1, 2) if R == 3 else (1, R - 2)     # the NaN mean and the all-clipped one
            live = [i for i in range(R) if i not in dead]
            for shift in range(POOL_RAYS if R <= 5 else 1):
                m = mid[(shift + 3 * np.arange(R)) % len(mid)].copy()
                if dead:
                    m[dead[0]], m[dead[1]] = np.nan, FAR + std_of(N, step) + 1.0
                ray = case_rays(net, instance, m, N, ni + ci + shift, few=R <= 5)
                for i, at in enumerate(live[::3]):                       # every third live ray one of the pairs
                    if pairs:
                        m[at], ray[at] = pairs[(i + ci + shift) % len(pairs)]
                case = dict(N=N, white=bool((ci + ni) & 1), ray=ray, mean=m, kind="count")
                # T4 asks a case of one, two or three live rays to show every column on (nearly) each of them, and whether a
                # ray does is a matter of J against its bound, which no rule on sigma's signs foretells: the next depths and
                # rays until T4 holds.  (Tried instead: the rays with the most density, and |J_c| >= 1e-3 .. 1e-2 of the sum
                # of magnitudes; each left cases short of T4.)  The host test asserts T4 on what comes out.
                if R > 5 or _shows(jacobian64(net, case, instance=instance)):
                    break
            out.append(case)
    return out


def case_inputs(net, case):
    """(o, d, viewdirs [R, 3], mean [R]) as float32 arrays."""
    r = net["rays"]
    f = np.float32
    return r["o"][case["ray"]].astype(f), r["d"][case["ray"]].astype(f), r["viewdirs"][case["ray"]].astype(f), case["mean"].astype(f)


# ---- placement ------------------------------------------------------------------------------------------------------
def place64(m, N, step, mutant=None):
    """ns_place.h in float64 on finite means m [R]: (z [R, N] clipped, dz [R, N]).  z = sort(cat[m + linspace(-std, std, N - 1),
    m]) with the mean merged at its rank p = #{a_i < m}, also returned; dz = 1 where the unclipped depth lies in [2, 6], bounds
    included."""
    m = np.asarray(m, dtype=np.float64)
    std, steps = std_of(N, step), N - 1
    if steps <= 1:
        lin = np.array([-std])
    else:
        st = float(np.float32(2.0 * std) / np.float32(steps - 1))
        i = np.arange(steps)
        lin = np.where(i < steps // 2, -std + st * i, std - st * (steps - i - 1))
    a = m[:, None] + lin[None, :]
    p = (a < m[:, None]).sum(axis=1)
    if mutant == "slot_off":
        p = np.where(p > 0, p - 1, p + 1)
    j = np.arange(N)[None, :]
    src = np.clip(np.where(j < p[:, None], j, j - 1), 0, steps - 1)
    v = np.take_along_axis(a, src, axis=1)
    v = np.where(j == p[:, None], m[:, None], v)
    dz = ((v > NEAR) & (v < FAR)) if mutant == "dz_open" else ((v >= NEAR) & (v <= FAR))
    return np.clip(v, NEAR, FAR), dz.astype(np.float64), p


def _rows(net, ray, z):
    """Pool rows of rays `ray` [R] at depths z [R, N] (multiples of the pool's step in [2, 6])."""
    K = len(net["rays"]["z"])
    k = np.rint((z - NEAR) / net["step"]).astype(np.int64)
    assert (NEAR + k * net["step"] == z).all() and k.min() >= 0 and k.max() < K
    return ray[:, None] * K + k


def samples64(net, case, mutant=None, e_raw=None, e_draw=None):
    """Per sample of the finite-mean rays of `case`: z, dz, raw [R, N, 4] (r, g, b, sigma), draw = dz G, dist, ddist, and the
    rays' |d|; `keep`: the indices of those rays in the case.  e_raw, e_draw [P, 3]: what the kernel's raw_c and d raw_c / d z
    of a pool row may differ by from net["raw"] and net["G"] (default: nothing, the exact fields); returned per sample."""
    keep = np.flatnonzero(np.isfinite(case["mean"]))
    ray, m, N = case["ray"][keep], case["mean"][keep], case["N"]
    z, dz, rank = place64(m, N, net["step"], mutant)
    rows = _rows(net, ray, z)
    raw = net["raw"][rows]
    draw = _G(net, mutant)[rows] * dz[..., None]
    nrm = np.sqrt((net["rays"]["d"][ray] ** 2).sum(axis=1))
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((len(ray), 1), 1e10)], axis=1) * nrm[:, None]
    ddist = np.concatenate([dz[:, 1:] - dz[:, :-1], np.zeros((len(ray), 1))], axis=1) * nrm[:, None]
    if mutant == "ddist_dropped":
        ddist = np.zeros_like(ddist)
    if mutant == "ddist_last":
        ddist[:, -1] = -dz[:, -1] * nrm
    zero = np.zeros(rows.shape + (3,))
    return dict(keep=keep, ray=ray, mean=m, rank=rank, ray_d=net["rays"]["d"][ray], z=z, dz=dz, raw=raw, draw=draw, dist=dist, ddist=ddist, nrm=nrm,
                e_raw=zero if e_raw is None else e_raw[rows], e_draw=zero if e_draw is None else e_draw[rows] * dz[..., None])


# ---- the reference and the bound ------------------------------------------------------------------------------------
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def jacobian64(net, case, mutant=None, instance="f16x3", e_raw=None, e_draw=None):
    """The float64 reference of a case's finite-mean rays: dict J [R, 6] (d r, g, b, disp, depth, acc / d m), out [R, 6] (the
    maps themselves), bound [R, 6] (the error model of the head of this file), keep (their indices in the case), and the
    facts `applies` reads.  `mutant`: one of MUTANTS, a fault of the reference.  e_raw, e_draw: see samples64; they enter c,
    c (1 - c) and dc to first order, the slope of the sigmoid taken at its largest within e_raw (|sigmoid''| <= 0.1):
    e_c = E_SIG + (c (1 - c) + 0.1 e_raw) e_raw,  e_cc += |1 - 2c| (e_c - E_SIG) + (e_c - E_SIG)^2,  e_dc += (cc + e_cc) e_draw."""
    N, white = case["N"], case["white"]
    if N == 1:
        return _single64(net, case, mutant, e_raw, e_draw)
    S = samples64(net, case, mutant, e_raw, e_draw)
    R = len(S["ray"])
    sg, dsg = S["raw"][..., 3], S["draw"][..., 3]
    z, dz, dist, ddist = S["z"], S["dz"], S["dist"], S["ddist"]
    pos = (sg >= 0) if mutant == "relu_sigma0" else (sg > 0)
    rl = np.maximum(sg, 0.0)
    s = rl * dist
    e = np.exp(-s)
    alpha = 1.0 - e
    keep = 1.0 - alpha + 1e-10
    A, B = dist * dsg * pos, rl * ddist
    D = A + B
    dalpha = e * D
    c = _sigmoid(S["raw"][..., :3])
    cc = c * _sigmoid(-S["raw"][..., :3])          # c (1 - c), 1 - c without cancellation
    dc = cc * S["draw"][..., :3]
    # the error model's per-sample pieces
    e_exp = np.where(e > 0, e * (2.0 ** -23 * (1.0 + s / math.log(2.0)) + 8 * U * s), 0.0)
    e_exp = np.where(e < MIN_NORMAL, np.maximum(e_exp, e), e_exp)
    e_exp = np.where(s == 0, 0.0, e_exp)
    e_alpha = e_exp + np.minimum(U * np.abs(alpha), 2.0 * e)
    e_alpha = np.where(s == 0, 0.0, e_alpha)
    rho = np.where(s == 0, 1e-10, e_alpha / keep + 3 * U)
    rounds = (s != 0).astype(np.float64)                     # a factor that is not exactly 1 rounds the product once
    e_D = 9 * U * (np.abs(A) + np.abs(B)) + U * np.abs(D)
    e_dalpha = e_exp * np.abs(D) + e * e_D + U * np.abs(dalpha)
    e_c_raw = (cc + 0.1 * S["e_raw"]) * S["e_raw"]                  # 0 on the exact fields
    e_cc = E_SIG * np.abs(1.0 - 2.0 * c) + 2 * U * cc + np.abs(1.0 - 2.0 * c) * e_c_raw + e_c_raw ** 2
    e_dc = e_cc * np.abs(S["draw"][..., :3]) + U * np.abs(dc) + (cc + e_cc) * S["e_draw"]

    zero = np.zeros(R)
    T, dT, relT, e_dT = np.ones(R), zero.copy(), np.full(R, U), zero.copy()
    val = np.zeros((R, 5))          # r, g, b, depth, acc
    tan = np.zeros((R, 5))
    e_val, e_tan, a_val, a_tan = (np.zeros((R, 5)) for _ in range(4))
    group = GROUP[instance]
    # a sample whose dist and ddist are both 0 (between equal depths) has alpha = dalpha = w = dw = 0 and a factor
    # of exactly 1 + 1e-10: only the others are walked, the factors of the ones between applied as a power
    active = (dist != 0) | (ddist != 0)
    active[:, -1] = True
    k0 = 1.0 + 1e-10
    done = np.zeros(R, dtype=np.int64)         # samples already accounted for
    cols = [np.flatnonzero(active[r]) for r in range(R)]
    steps = max(len(x) for x in cols)
    idx = np.full((R, steps), -1, dtype=np.int64)
    for r, x in enumerate(cols):
        idx[r, :len(x)] = x
    ar = np.arange(R)
    resets = {"reset64": 64, "reset128": 128}
    for t in range(steps):
        j = idx[:, t]
        live = j >= 0
        jj = np.where(live, j, 0)
        gap = np.where(live, jj - done, 0)
        T = T * k0 ** gap
        dT = dT * k0 ** gap
        e_dT = e_dT * k0 ** gap
        relT = relT + gap * 1e-10 + U * ((jj // 64) - (done // 64)) * live
        if mutant in resets or mutant == "reset_second":
            if mutant in resets:
                at = np.full(R, resets[mutant])
            else:                      # the ray that begins inside a group: its state lost at the group's end
                first = (S["keep"] * N) % group
                at = np.where(first != 0, group - first, N + 1)
            hit = live & (done <= at) & (jj >= at) & (at > 0) & (at < N)
            T = np.where(hit, 1.0, T)
            dT = np.where(hit, 0.0, dT)
            val = np.where(hit[:, None], 0.0, val)
            tan = np.where(hit[:, None], 0.0, tan)
        g = lambda x: x[ar, jj]
        al, da, kp = g(alpha), g(dalpha), g(keep)
        ea, eda = g(e_alpha), g(e_dalpha)
        zz, zd = g(z), g(dz)
        w = al * T
        e_w = T * ea + np.abs(w) * (relT + U) + CB.TINY
        Tda, adT = T * da, al * dT
        dw = Tda + adT
        e_dw = T * eda + np.abs(Tda) * relT + al * e_dT + np.abs(dT) * ea + 2 * U * (np.abs(Tda) + np.abs(adT))
        x = np.concatenate([c[ar, jj], zz[:, None], np.ones((R, 1))], axis=1)                      # [R, 5]
        dx = np.concatenate([dc[ar, jj], zd[:, None], np.zeros((R, 1))], axis=1)
        e_x = np.concatenate([E_SIG + e_c_raw[ar, jj], np.zeros((R, 2))], axis=1)
        e_dx = np.concatenate([e_dc[ar, jj], np.zeros((R, 2))], axis=1)
        t1, t2 = x * dw[:, None], w[:, None] * dx
        e_t = e_x * np.abs(dw)[:, None] + x * e_dw[:, None] + np.abs(w)[:, None] * e_dx + np.abs(dx) * e_w[:, None] \
            + 2 * U * (np.abs(t1) + np.abs(t2))
        p = w[:, None] * x
        e_p = x * e_w[:, None] + np.abs(w)[:, None] * e_x + U * np.abs(p)
        lv = live[:, None]
        val = np.where(lv, val + p, val)
        tan = np.where(lv, tan + t1 + t2, tan)
        a_val = np.where(lv, a_val + np.abs(p), a_val)
        a_tan = np.where(lv, a_tan + np.abs(t1) + np.abs(t2), a_tan)
        e_val = np.where(lv, e_val + e_p + U * a_val * (p != 0), e_val)
        e_tan = np.where(lv, e_tan + e_t + U * a_tan * ((t1 != 0) | (t2 != 0)), e_tan)
        Tn = T * kp
        if mutant == "dT_new_T":
            dTn = dT * kp - Tn * da
        elif mutant == "keep_no_eps":
            dTn = dT * (1.0 - al) - Tda
        else:
            dTn = dT * kp - Tda
        e_dTn = kp * e_dT + np.abs(dT) * (ea + 3 * U * kp) + T * eda + np.abs(Tda) * relT + 2 * U * (np.abs(kp * dT) + np.abs(Tda))
        relTn = relT + g(rho) + U * g(rounds)
        T, dT, e_dT, relT = np.where(live, Tn, T), np.where(live, dTn, dT), np.where(live, e_dTn, e_dT), np.where(live, relTn, relT)
        done = np.where(live, jj + 1, done)

    J, out, bound = np.zeros((R, 6)), np.zeros((R, 6)), np.zeros((R, 6))
    dacc, e_dacc = tan[:, 4], e_tan[:, 4]
    if white and mutant != "white_dropped":
        J[:, :3] = tan[:, :3] - dacc[:, None]
        bound[:, :3] = e_tan[:, :3] + e_dacc[:, None] + U * np.abs(J[:, :3])
    else:
        J[:, :3], bound[:, :3] = tan[:, :3], e_tan[:, :3]
    out[:, :3] = val[:, :3] + ((1.0 - val[:, 4:5]) if white else 0.0)
    J[:, 4], bound[:, 4], out[:, 4] = tan[:, 3], e_tan[:, 3], val[:, 3]
    J[:, 5], bound[:, 5], out[:, 5] = dacc, e_dacc, val[:, 4]
    depth, acc, ddepth = val[:, 3], val[:, 4], tan[:, 3]
    e_depth, e_acc, e_ddepth = e_val[:, 3], e_val[:, 4], e_tan[:, 3]
    den = acc + 1e-10
    inv = 1.0 / den
    q = depth * inv
    rel_inv = e_acc * inv + 4 * U
    e_q = e_depth * inv + q * (rel_inv + U)
    dq = inv * (ddepth - q * dacc)
    e_dq = inv * (e_ddepth + np.abs(dacc) * e_q + q * e_dacc + 2 * U * (np.abs(ddepth) + np.abs(q * dacc))) + np.abs(dq) * (rel_inv + U)
    qm = np.maximum(q, 1e-10)
    disp = 1.0 / qm
    fac = np.where(q > 1e-10, 1.0, np.where(q == 1e-10, 1.0 if mutant == "disp_tie" else 0.5, 0.0))
    J[:, 3] = -disp * disp * dq * fac
    out[:, 3] = disp
    rel_disp = e_q / qm + 2 * U
    bound[:, 3] = disp * disp * e_dq * fac + np.abs(J[:, 3]) * (2 * rel_disp + 2 * U) \
        + np.where(np.abs(q - 1e-10) <= e_q, np.abs(disp * disp * dq), 0.0)
    bound = np.maximum(bound, DENORMAL_FLOOR)
    vis = dz * (dist != 0)
    Tfull = np.concatenate([np.ones((R, 1)), np.cumprod(keep, axis=1)[:, :-1]], axis=1)
    mag = np.concatenate([a_tan[:, :3] + a_tan[:, 4:5], (disp * disp * inv * (a_tan[:, 3] + q * a_tan[:, 4]))[:, None], a_tan[:, 3:5]], axis=1)
    return dict(J=J, out=out, bound=bound, mag=mag, keep=S["keep"], N=N,
                on_bound=(((z == NEAR) | (z == FAR)) & (dz > 0)).any(),
                sigma0=((sg == 0) & (dsg != 0) & (vis > 0)).any(), open_end=(sg[:, -1] <= 0).any(), ddist_live=((B != 0) & (Tfull >= 0.01) & (z < FAR))[:, :-2].any(),
                dT_live=((alpha * dalpha != 0)[:, :-1] & (np.cumsum((alpha != 0)[:, ::-1], axis=1)[:, ::-1] > 0)[:, 1:]).any(),
                T=Tfull, samples=S)


def _single64(net, case, mutant=None, e_raw=None, e_draw=None):
    """raw2outputs' N == 1 rule at z = m, unclipped, dz = 1: rgb = sigmoid(raw), d rgb = c (1 - c) d raw, everything else 0."""
    keep = np.flatnonzero(np.isfinite(case["mean"]))
    ray, m = case["ray"][keep], case["mean"][keep]
    rows = _rows(net, ray, m[:, None])[:, 0]
    raw, G = net["raw"][rows], _G(net, mutant)[rows]
    c = _sigmoid(raw[:, :3])
    R = len(ray)
    J, out, bound = np.zeros((R, 6)), np.zeros((R, 6)), np.zeros((R, 6))
    J[:, :3] = c * _sigmoid(-raw[:, :3]) * G[:, :3]
    out[:, :3], out[:, 3] = c, 1e10
    bound[:, :3] = 6 * U * np.abs(J[:, :3]) + np.abs(G[:, :3]) * 4 * U * c
    if e_raw is not None:
        cc = c * _sigmoid(-raw[:, :3])
        e_c = (cc + 0.1 * e_raw[rows]) * e_raw[rows]
        e_cc = np.abs(1.0 - 2.0 * c) * e_c + e_c ** 2
        bound[:, :3] += e_cc * np.abs(G[:, :3]) + (cc + e_cc + 4 * U * c) * e_draw[rows]
    bound = np.maximum(bound, DENORMAL_FLOOR)          # (d disp = d depth = d acc = 0 exactly)
    mag = np.zeros((R, 6))
    mag[:, :3] = c * _sigmoid(-raw[:, :3]) * net["Gabs"][rows][:, :3]
    return dict(J=J, out=out, bound=bound, mag=mag, keep=keep, N=1, on_bound=False, sigma0=False, open_end=False, ddist_live=False, dT_live=False, T=None,
                samples=None)


# ---- the primal maps under composite_bounds.py's comparator ---------------------------------------------------------
def primal_check(got, ref, white):
    """got [R, 6] (r, g, b, disp, depth, acc of the finite-mean rays, float64 of the kernel's fp32) against the float64
    reference under composite_bounds.py's comparator (check_maps).  Returns the worst |err| / bound."""
    S = ref["samples"]
    if S is None:
        c = ref["out"][:, :3]
        assert (np.abs(got[:, :3] - c) <= 4 * U * c + CB.TINY).all(), "one-sample rgb"
        assert (got[:, 4:] == 0).all() and (np.abs(got[:, 3] - 1e10) <= 1024.0).all(), "one-sample disp / depth / acc"
        return float((np.abs(got[:, :3] - c) / (4 * U * c + CB.TINY)).max())
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    maps = dict(rgb=f(got[:, :3]), disp=f(got[:, 3]), depth=f(got[:, 4]), acc=f(got[:, 5]))
    stats = CB.check_maps(maps, f(S["raw"]).float(), f(S["z"]).float(), f(S["ray_d"]).float(), None, white)
    return max(v[0] for v in stats.values())


# ---- an fp32 transcription of walk_samples / write_jacobian ---------------------------------------------------------
def walk_fp32(net, case):
    """ns_tangent.h's walk_samples and write_jacobian in torch fp32 (its exp, its sigmoid as 1 / (1 + exp(-x))) on the case's
    finite-mean rays: J [R, 6] as float64."""
    S = samples64(net, case)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    raw, draw, z, dz = f(S["raw"]), f(S["draw"]), f(S["z"]), f(S["dz"])
    d = f(net["rays"]["d"][S["ray"]])
    nrm = torch.sqrt(d[:, 2] * d[:, 2] + (d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0]))
    R, N = z.shape
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10)], 1) * nrm[:, None]
    ddist = torch.cat([dz[:, 1:] - dz[:, :-1], torch.zeros(R, 1)], 1) * nrm[:, None]
    tmul = lambda x, t: torch.where(t == 0, torch.zeros_like(t), x * t)
    one = torch.ones(R)
    T, dT = one.clone(), torch.zeros(R)
    val = [torch.zeros(R) for _ in range(5)]
    tan = [torch.zeros(R) for _ in range(5)]
    eps = torch.tensor(1e-10, dtype=torch.float32)
    for j in range(N):
        sg, di = raw[:, j, 3], dist[:, j]
        rl = torch.relu(sg)
        dsg = torch.where(sg <= 0, torch.zeros(R), draw[:, j, 3])
        ex = torch.exp(-rl * di)
        alpha = 1.0 - ex
        dalpha = tmul(ex, tmul(di, dsg) + tmul(rl, ddist[:, j]))
        w = alpha * T
        dw = tmul(T, dalpha) + tmul(alpha, dT)
        for k in range(3):
            ck = 1.0 / (1.0 + torch.exp(-raw[:, j, k]))
            dck = tmul(ck * (1.0 - ck), draw[:, j, k])
            val[k] = val[k] + w * ck
            tan[k] = tan[k] + (tmul(ck, dw) + tmul(w, dck))
        val[3] = val[3] + w * z[:, j]
        val[4] = val[4] + w
        tan[3] = tan[3] + (tmul(z[:, j], dw) + tmul(w, dz[:, j]))
        tan[4] = tan[4] + dw
        keep = (1.0 - alpha) + eps
        dT = tmul(keep, dT) - tmul(T, dalpha)
        T = T * keep
    J = torch.zeros(R, 6)
    for k in range(3):
        J[:, k] = tan[k] - tan[4] if case["white"] else tan[k]
    J[:, 4], J[:, 5] = tan[3], tan[4]
    inv = 1.0 / (val[4] + eps)
    q = val[3] * inv
    dq = tmul(inv, tan[3] - tmul(q, tan[4]))
    dqm = torch.where(q > eps, dq, torch.where(q == eps, 0.5 * dq, torch.zeros(R)))
    disp = 1.0 / torch.maximum(eps, q)
    J[:, 3] = -tmul(disp * disp, dqm)
    return J.double().numpy()
