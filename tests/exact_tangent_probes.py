"""The derivative of every embedding column in the depth-tangent render kernels (embed3_tan, ns_tangent.h) against float64.

Shared by tests/test_exact_field_probes_host.py (coverage, the reference against autograd, an fp32 transcription, the mutants)
and tests/test_gpu_exact_field_probes.py (nerf_mlp_x3_tan_kernel, nerf_mlp_x3_tan1_kernel, nerf_tan16_kernel).  Nothing here
calls the library.  On the identity networks of exact_tangent.py embed3_tan multiplies zeros; here it carries the Jacobian.

A tangent probe field is a probe field of exact_field_probes.py (routes layer0 and skip, shapes prod and d2w128) whose
alpha_linear is a bias alone, sigma = 1/2: an exact positive constant, d sigma = 0, so alpha, the transmittance and their
tangents are what exact_tangent.py's model already bounds.  The three rows of rgb_linear read the route's columns, three heads
a network, four networks a route.  The rays are pool A's of exact_tangent.py: every sample is a dyadic pool point, p = o + d z
exactly, and

    d raw_c / d z = sum_j w_j [e_j != 0] 2^l (cos, -sin)(2^l p_i) d_i          (an identity column: w_j d_i)

with the mask on the reference's own float64 activation: relu(+e_j) and relu(-e_j) are both closed at e_j == 0 only, which on
the pool are the sines at p_i = 0 (the kernels' sine of 0 is 0 as well: the host test asserts it of the transcription, and that
every other activation is at least 2^-15, eight times v_sin_f32's allowance, so that no kernel within its gate sees another
sign).

The error model is exact_tangent.py's with its two inputs per sample and colour channel:
    e_raw_c    the gate of exact_field_probes.py for the handle's operand type;
    e_draw_c = sum_j |w_j| [e_j != 0] 2^l |d_i| tau'_t + n_t U sum_j |w_j d e_j|         (n_t: exact_field_probes.py's head term)
tau', walking embed3_tan and TanOps<M>: the column's value is (Trig(level, c + 1) 2^level) pd_i.
    Trig<true> at the phase h = c + 1, two quarter turns for a cosine's derivative.  lo' = lo 2^level + h / 4 rounds at 1/2 to
    2^-24: 2^-25 of a revolution, pi U in the angle (h = 1: pi / 2 U; h = 0: nothing).  fract is exact for a >= 0 and leaves
    f in [0, 1); the first fold gives [-1/2, 1/2), and (..) + lo' lies in [-1/2 - |lo|, 1): NOT the [-1/2, 3/4) of the comment
    written for one quarter turn, and a negative lo goes below -1/2 by up to 2^-15 at h = 0.  The second fold takes (1/2, 1) to
    (-1/2, 0) and the third maps every f in [-1/2 - 2^-15, 1/2] to |g| <= 1/4: the series stays inside [-pi / 2, pi / 2].
    The roundings: for a < 0 with |a| < 1/2 v_fract_f32 returns 1 - |a| rounded to 2^-24 (pi U; the engine's comment calls it
    exact), the sum f + lo' then lies in (0, 1/2) (pi / 2 U); otherwise fract is exact and the sum in [1/2, 1) costs pi U.
    At worst pi + pi + pi / 2 = 7.9 U in the angle, times |cos theta|, plus the series' 1.8 U (exact_field_probes.py): 9.7 U,
    taken as 10 U.
    The factor 2^level is exact.  The product with pd_i rounds once: U (on the pools d is dyadic and it is exact).
    The tangent tile: f16x3 holds hi + lo, 2 U of the value; the f16 instance rounds to f16, 2^-11 of a value of up to
    512 |d| (no overflow: 512 is an f16 number), and its Trig<false> hands v_sin_f32 (2^-18) an argument with the same three
    roundings, 7.9 U.  Every later tangent layer copies the value: a one-hot row, a mask, the fold's +-1.
    tau' = 10 U + U + 2 U = 13 U (f16x3, the one-sample kernel)      tau' = 2^-11 + 2^-18 + 8 U + U (f16)
each times 2^l |d_i|; an identity column has l = 0 and no Trig: it is held to the same tau'.
No constant is fitted to a kernel; every ray is held, and J == 0 exactly for a NaN mean and an all-clipped ray.

Measured on an MI355X, worst |J - J64| / bound over every probe and case: f16x3 (nerf_mlp_x3_tan_kernel) 0.400 (prod, layer0,
N = 2, g), f16 (nerf_tan16_kernel) 0.297 (prod, N = 2), one sample per ray (nerf_mlp_x3_tan1_kernel) 0.245 (prod); the skip
route gives the layer0 route's figures.  The CPU transcription: 0.400, 0.297, 0.179.
"""

import numpy as np

import exact_field as E
import exact_field_probes as P
import exact_tangent as X

U = X.U
SIGMA = 0.5
SHAPES = ("prod", "d2w128")
ROUTES = ("layer0", "skip")
WHICH = "A"
INSTANCES = X.INSTANCES
DTYPE = {"f16x3": "f16x3", "f16": "f16", "single": "f16x3"}
TAU_TAN = {"f16x3": 13 * U, "f16": 2.0 ** -11 + 2.0 ** -18 + 9 * U}
MULTI_N = (2, 64)
RAYS = 32
NAN_AT, CLIPPED_AT = 5, 9
TANGENT_MUTANTS = ("no_scale", "primal_phase", "wrong_pd")
MIN_ACTIVATION = 2.0 ** -15


def probes():
    out = []
    for shape in SHAPES:
        for route in ROUTES:
            if route in P.routes_of(shape):
                out += [(shape, route, part) for part in range(-(-len(P.groups(route)) // 3))]
    return out


def d_embedding(pts, d, mutant=None):
    """d gamma(p) / d z [P, 63] in float64 for p = o + d z: d_i, then 2^l (cos, -sin)(2^l p_i) d_i, and the mask e_j != 0."""
    e = P.gamma64(pts.astype(np.float32), 10)
    out = np.zeros_like(e)
    for j in range(E.IN_PTS):
        level, phase, comp = P.column_info(j)
        di = d[:, (comp + 1) % 3] if mutant == "wrong_pd" else d[:, comp]
        if level < 0:
            out[:, j] = di
            continue
        a = pts[:, comp] * 2.0 ** level
        if mutant == "primal_phase":
            t = np.sin(a) if phase == 0 else np.cos(a)
        else:
            t = np.cos(a) if phase == 0 else -np.sin(a)
        out[:, j] = (1.0 if mutant == "no_scale" else 2.0 ** level) * t * di
    return out, e != 0


_cache = {}


def network(shape, route, part):
    """The tangent probe network with exact_tangent.py's tables on pool A: pool (the float64 embedding of the pool's points and
    view directions), raw, G = d raw / d z [P, 4], Gabs, rays, step; and dE, mask, scale (2^l |d_i| per row and column)."""
    key = (shape, route, part)
    if key in _cache:
        return _cache[key]
    net = dict(P.make_probe(shape, route, part, alpha_bias=SIGMA))
    pool, rays = X.make_tangent_pool(E.NETWORKS[shape]["seed"], WHICH)
    K = len(rays["z"])
    pts = pool[:, :3]
    assert E.is_f32(pts)
    x = np.concatenate([P.gamma64(pts.astype(np.float32), 10),
                        np.repeat(P.gamma64(rays["viewdirs"].astype(np.float32), 4), K, axis=0)], axis=1)
    d = np.repeat(rays["d"], K, axis=0)
    net.update(pool=x, points=pts, rays=rays, name=f"{shape}-{route}-{part}", which=WHICH, step=X.POOLS[WHICH]["step"], Gm={}, dirs=d)
    net["raw"] = E.chain(net, x)
    assert (net["raw"][:, 3] == SIGMA).all()
    net["G"], net["Gabs"], net["dE"], net["mask"] = tangent_table(net, None)
    lv = np.array([max(P.column_info(j)[0], 0) for j in range(E.IN_PTS)])
    comp = np.array([P.column_info(j)[2] for j in range(E.IN_PTS)])
    net["scale"] = 2.0 ** lv[None, :] * np.abs(d[:, comp])
    _cache[key] = net
    return net


def tangent_table(net, mutant):
    dE, mask = d_embedding(net["points"], net["dirs"], mutant)
    G, Gabs = np.zeros((dE.shape[0], 4)), np.zeros((dE.shape[0], 4))
    for c, cols, wts in net["heads"]:
        cols, wts = np.array(cols), np.array(wts)
        G[:, c] = (dE[:, cols] * mask[:, cols]) @ wts
        Gabs[:, c] = np.abs(dE[:, cols] * mask[:, cols]) @ np.abs(wts)
    return G, Gabs, dE, mask


def mutated(net, mutant):
    """A copy of the network whose tangent table carries the fault."""
    out = dict(net)
    out["G"] = tangent_table(net, mutant)[0]
    return out


def errors(net, instance):
    """(e_raw, e_draw) [P, 3] of the module docstring."""
    dtype = DTYPE[instance]
    e_raw = P.gate(net, net["pool"], dtype)[:, :3]
    e_draw = np.zeros_like(e_raw)
    n = P.HEAD_ROUNDINGS[dtype]
    for c, cols, wts in net["heads"]:
        cols, wts = np.array(cols), np.abs(np.array(wts))
        e_draw[:, c] = (net["scale"][:, cols] * net["mask"][:, cols]) @ wts * TAU_TAN[dtype] + n * U * net["Gabs"][:, c]
    return e_raw, e_draw


def cases(net, instance):
    """exact_tangent.py's case dicts: one batch of 32 rays per sample count and background; in the multi-sample ones a NaN
    mean and an all-clipped ray ride along, and the window of unclipped samples lies inside the ray."""
    z, step = net["rays"]["z"], net["step"]
    ray = np.arange(RAYS)
    if instance == "single":
        return [dict(N=1, white=False, ray=ray, mean=z[(3 * ray + 1) % len(z)].copy(), kind="main")]
    out = []
    for N in MULTI_N:
        std = X.std_of(N, step)
        if N == 2:
            m = X.NEAR + step * (1 + ray % 16)
        else:
            win = int(round((X.FAR - X.NEAR) / step))
            m = X.NEAR + std - (1 + (7 * ray) % (N - 3 - win)) * step
        m = m.astype(np.float64)
        m[NAN_AT], m[CLIPPED_AT] = np.nan, X.FAR + std + 1.0
        out += [dict(N=N, white=white, ray=ray, mean=m.copy(), kind="main") for white in (True, False)]
    return out


def jacobian64(net, case, instance):
    e_raw, e_draw = errors(net, instance)
    return X.jacobian64(net, case, instance="f16x3" if instance == "single" else instance, e_raw=e_raw, e_draw=e_draw)


# ---- an fp32 transcription of embed3_tan on top of exact_field_probes.py's Trig -------------------------------------
def transcription(net, instance):
    """A copy of the network whose raw and G tables are what a kernel of the instance forms: Trig in fp32 (Trig<false>: up to
    v_sin_f32's own error), the operand's rounding of the column and of its tangent, the mask on its own activation."""
    dtype = DTYPE[instance]
    precise = dtype == "f16x3"
    pts32 = net["points"].astype(np.float32)
    e = P.operand(np.concatenate([P.gamma32(pts32, 10, precise), net["pool"][:, E.IN_PTS:]], axis=1), dtype)
    dE = np.zeros((e.shape[0], E.IN_PTS))
    d = net["dirs"]
    for j in range(E.IN_PTS):
        level, phase, comp = P.column_info(j)
        if level < 0:
            dE[:, j] = d[:, comp]
        else:
            t = P._f32(P.trig32(pts32[:, comp], level, phase + 1, precise)) * 2.0 ** level
            dE[:, j] = P._f32(t * d[:, comp])
    dE = P.operand(dE, dtype)
    out = dict(net)
    out["raw"] = E.chain(net, e)
    G = np.zeros((e.shape[0], 4))
    for c, cols, wts in net["heads"]:
        cols, wts = np.array(cols), np.array(wts)
        G[:, c] = (dE[:, cols] * (e[:, cols] != 0)) @ wts
    out["G"] = G
    return out
