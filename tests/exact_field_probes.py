"""The radiance field's sines and cosines, column by column, against float64.

Shared by tests/test_exact_field_probes_host.py (coverage, the fold, the reference against the fp32 oracle, an fp32
transcription of to_rev / Trig<>, the mutants: all on the CPU) and tests/test_gpu_exact_field_probes.py (the HIP kernels).
Nothing here calls the library.

The networks of exact_field.py are fed pre-embedded rows or multiply every sine and cosine column by zero.  A probe field is
the opposite: a NeRF of one-hot rows that carries single embedding columns to `raw`, after part B of exact_depthnet.py.
For an embedding column j two hidden units, relu(+e_j) and relu(-e_j) (weight +-1, bias 0); every later hidden layer carries
them with one-hot rows of weight 1 (to another position of the layer each time); a head reads u+_j - u-_j = e_j of six
(some heads: five) columns with the weights PROBE_HEAD from {+-1, +-1/2}, neighbouring weights different.  The heads are
alpha_linear, the three rows of rgb_linear -- behind feature_linear rows u+_j - u-_j and view units relu(+-feature_j), so that
the folded views_linears.0 o feature_linear is a 0 / +-1 matrix (the host test holds it against ns_fold_nerf_views) -- and
the rows of output_linear where the network has no view directions.  A head without columns has weight zero: raw == 0 exactly.

Routes (`ROUTES`), every column of a route in exactly one head (`groups`: head g reads the columns g, g + G, g + 2 G, ..: for
the 63 point columns G = 11, neighbours two levels or one apart and on different components; for the 27 view columns G = 5):
  layer0   the 63 point columns through pts_linears.0
  skip     the 63 point columns through the embedding share of the layer behind the skip; layer 0 reads the raw coordinates
           only (and what it computes is read by nobody), so a sine can only have come from the per-wave stash
  views    the 27 view columns through views_linears.0
on the shapes `SHAPES` of exact_field.NETWORKS: prod (the generated streams), d2w128 (the 128-wide kernels; no skip),
d4w200out5 (no view directions, five outputs, skip (2,)).  A network holds four heads (five: d4w200out5; three: views), so a
route takes three networks (views: two): 19 packed handles per operand type.

Inputs.  `probe_points`: 321 fp32 points, one more than a 320-row group: full-mantissa points of the production geometry and up
to |p| = 8, components exactly 0, -0, 2^-20, negative and 8, and points within two ulp of a zero of every level's sine and
cosine.  `probe_dirs`: unit and non-unit view directions in runs of rays that share one, and neighbours that differ in
exactly one component, each component in turn; the pattern's period is 11 rays, so that with one sample per ray (321 rows)
and with the shapes (1, 1), (5, 7), (33, 31) a direction changes at a 16-sample tile boundary and inside a tile.  The rays form
takes the dyadic o, d, z of exact_field.make_ray_pool, whose o + d z is exact in fp32, fused or not.

Reference: exact_field.chain in float64 on `embedding64` of the fp32 inputs -- x, then sin and cos of 2^l x in float64 -- with
the ReLU masks on its own values.  The gate, per row and head with columns j and weights w_j:

    |raw - raw64| <= sum_j |w_j| s_j tau_t + n_t U sum_j |w_j e_j|            U = 2^-24

    s_j = 1 for a sine or cosine column; for an identity column max(1, |e_j|) under bf16 and f16, 1 otherwise.

    tau = 8 U for f32 and f16x3 (exact_depthnet.PROBE_TAU): Trig<true> (ns_mlp_engine.h), the walk of exact_depthnet.py's
    part B: the reduced argument's one rounding, pi U in the angle; the constant and the product, 1.7 U; the series'
    truncation 0.95 U; the Horner steps 1.8 U.  Part B leaves out the rounding of lo + h / 4 for the cosine (h = 1), a
    quarter U of a revolution, pi / 2 U in the angle.  It does not move the bound: the argument's error reaches the result
    times |cos theta|, theta the folded angle in [-pi / 2, pi / 2]; the truncation is (theta)^13 / 13!, 0.95 U at pi / 2 only,
    where cos theta = 0.  (3 pi / 2 + 0.78 theta) |cos theta| U + theta^13 / 13! + 1.8 U is largest at theta = 0: 6.5 U.
    Nor is v_fract_f32 exact for -1/2 < a < 0: it returns 1 - |a| rounded to 2^-24, pi U in the angle; the fold then leaves
    f - 1 in (-1/2, 0) and the sum with lo below 1/2 in magnitude (pi / 2 U, below 1/4: pi / 4 U), so the three roundings stay
    within pi + pi / 2 + pi / 4 = 5.5 U and the bound within 7.3 U.
    What differs from the DepthNet: nothing behind the column rounds.  relu(+-e_j) with weight +-1 and bias 0 is e_j or 0 in
    the fp32 accumulator; the k-major engine keeps it as it is, the split engine holds hi = fl16(e), lo = fl16(e - hi) and
    splitting hi + lo again returns hi and lo; the one-hot layers, feature_j = u+ - u- (one of them is 0) and the view units
    copy it.  An identity column costs f32 nothing and f16x3 2^-23 |x|, at most 8 U below 8 (8 itself is an f16 number).
    tau = 2^-8 + 2^-18 for bf16 and 2^-11 + 2^-18 for f16, exact_depthnet.PROBE_TAU as it stands: v_sin_f32's 2^-18 (part B)
    and the operand's rounding.  The DepthNet's walk counts two roundings of 2^-9 (2^-12), the column's and the activation's
    behind it.  Here relu(+-e) of a value that already is an operand number is that number, and so is every copy of it: ONE
    rounding, to nearest even.  It is at most 2^-9 (2^-12) for a sine or cosine, half an ulp below 1, but up to 2^-8 |x|
    (2^-11 |x|) for an identity column, half an ulp just above a power of two -- a first draft of this gate with
    tau = 2^-9 + 2^-18 failed the CPU transcription on exactly those columns (1.11 of it at y = 4.06) -- and an identity
    column reaches 8: max(1, |e_j|) times tau, as in part B.  tau is left at the one figure for both kinds of column.
    The head: the engine's fp32 accumulator adds at most six non-zero products w_j u_j to a zero bias, twelve on the split
    engine (w_hi u_hi and w_hi u_lo; w_lo = 0), each product exact: one rounding per addition, each at most U times the sum
    of magnitudes.  n = 6 (f32, bf16, f16), n = 12 (f16x3).  The rgb heads add nothing: every layer in front is a copy.
No constant is fitted to a kernel, and no row, column or ray is exempt.

Measured on an MI355X, worst |raw - raw64| / gate over every probe, row and head (points and rays forms, both runs; the
generic kernels and four and five tiles give the same figures): f32 0.204 (embed3; layer0 0.197, skip 0.183, views 0.204),
f16x3 0.200 (embedN_16, Trig<true>; views 0.167), bf16 0.554 (embed3_16, v_sin_f32; views 0.386), f16 0.588 (views 0.443).
The 16-bit figures are the operand's rounding of an identity column, 0.55 of its allowance, and are those of the CPU
transcription (0.554, 0.590), which spends nothing on v_sin_f32; the fp32 oracle on the CPU 0.181 on one host.
"""

import numpy as np
import torch

import exact_field as E

U = 2.0 ** -24
PROBE_HEAD = (1.0, -0.5, 0.5, -1.0, -0.5, 1.0)
PROBE_DTYPES = ("f32", "bf16", "f16", "f16x3")
PROBE_TAU = {"f32": 8 * U, "f16x3": 8 * U, "bf16": 2.0 ** -8 + 2.0 ** -18, "f16": 2.0 ** -11 + 2.0 ** -18}      # exact_depthnet.PROBE_TAU
HEAD_ROUNDINGS = {"f32": 6, "bf16": 6, "f16": 6, "f16x3": 12}
ROUNDED_DTYPES = ("bf16", "f16")
VSIN_ALLOWANCE = 2.0 ** -18
ROUTES = ("layer0", "skip", "views")
SHAPES = ("prod", "d2w128", "d4w200out5")
ROUTE_COLUMNS = {"layer0": E.IN_PTS, "skip": E.IN_PTS, "views": E.IN_VIEWS}
ROUTE_GROUPS = {"layer0": 11, "skip": 11, "views": 5}
POINT_ROWS = 321
RAY_SHAPES = E.RAY_SHAPES[:3]
MUTANT_ROWS = 64


# ---- columns --------------------------------------------------------------------------------------------------------
def column_info(j):
    """(level, phase, component) of column j of an embedding [x, sin x, cos x, sin 2x, ..]: level -1 for x itself, phase 0
    for a sine and 1 for a cosine."""
    if j < 3:
        return -1, 0, j
    k = j - 3
    return k // 6, (k % 6) // 3, k % 3


def column_of(level, phase, comp):
    return comp if level < 0 else 3 + 6 * level + 3 * phase + comp


def groups(route):
    """The heads of a route: head g reads the columns g, g + G, g + 2 G, ..."""
    n, G = ROUTE_COLUMNS[route], ROUTE_GROUPS[route]
    return [list(range(g, n, G)) for g in range(G)]


def routes_of(shape):
    cfg = E.NETWORKS[shape]
    return [r for r in ROUTES if (r != "skip" or cfg["skips"]) and (r != "views" or cfg["use_viewdirs"])]


def heads_per_network(shape, route):
    cfg = E.NETWORKS[shape]
    return cfg["output_ch"] if not cfg["use_viewdirs"] else 3 if route == "views" else 4


def probes():
    """Every probe network as (shape, route, part): part p holds the heads p n .. p n + n - 1 of the route."""
    out = []
    for shape in SHAPES:
        for route in routes_of(shape):
            n = heads_per_network(shape, route)
            out += [(shape, route, p) for p in range(-(-len(groups(route)) // n))]
    return out


# ---- the networks ---------------------------------------------------------------------------------------------------
def _pos(k, layer, W):
    """Where layer `layer` holds unit k: another position in every layer, spread over the 16-row and 32-column blocks."""
    return (37 * k + 16 * layer + 5) % W


_cache = {}


def make_probe(shape, route, part, alpha_bias=None):
    """The probe network as exact_field.chain and ops.pack_nerf take it: dict D, W, skips, use_viewdirs, output_ch, names,
    weights, biases, and heads: [(raw channel, columns, weights)] (the columns index the route's embedding).
    alpha_bias (exact_tangent_probes.py): alpha_linear is that bias alone, and a network holds three heads, the rows of rgb_linear."""
    key = (shape, route, part, alpha_bias)
    if key in _cache:
        return _cache[key]
    cfg = E.NETWORKS[shape]
    D, W, skips, views = cfg["D"], cfg["W"], tuple(cfg["skips"]), cfg["use_viewdirs"]
    assert route in routes_of(shape) and 37 % 2 and np.gcd(37, W) == 1
    n = heads_per_network(shape, route) if alpha_bias is None else 3
    mine = groups(route)[part * n:(part + 1) * n]
    assert mine
    if not views:
        channels = list(range(cfg["output_ch"]))
    elif route == "views" or alpha_bias is not None:
        channels = [0, 1, 2]
    else:
        channels = [3, 0, 1, 2]                    # alpha_linear first, then the rows of rgb_linear
    heads = [(channels[i], cols, PROBE_HEAD[:len(cols)]) for i, cols in enumerate(mine)]
    names = E.layer_names(D, views)
    width = {"pts0": E.IN_PTS}
    for i in range(1, D):
        width[f"pts{i}"] = W + E.IN_PTS if (i - 1) in skips else W
    width.update(feature=W, alpha=W, views=W + E.IN_VIEWS, rgb=W // 2, output=W)
    rows = {nm: W for nm in names}
    rows.update(alpha=1, views=W // 2, rgb=3, output=cfg["output_ch"])
    w = {nm: np.zeros((rows[nm], width[nm])) for nm in names}
    units = [(j, s) for _, cols, _ in heads for j in cols for s in (1.0, -1.0)]      # unit k = relu(s e_j)
    unit_of = {(j, s): k for k, (j, s) in enumerate(units)}
    assert len(units) <= W
    first = 0                                      # the layer that reads the embedding
    if route != "layer0":
        # layer 0 reads the raw coordinates only and the layers up to the skip copy it: nothing reads the result
        first = skips[0] + 1 if route == "skip" else None
        stop = D if first is None else first
        for m in range(W):
            w["pts0"][m, m % 3] = 1.0 if (m // 3) % 2 == 0 else -1.0
        for i in range(1, stop):
            off = E.IN_PTS if (i - 1) in skips else 0
            w[f"pts{i}"][np.arange(W), off + np.arange(W)] = 1.0
    if route != "views":
        for k, (j, s) in enumerate(units):
            w[f"pts{first}"][_pos(k, first, W), j] = s
        for i in range(first + 1, D):
            off = E.IN_PTS if (i - 1) in skips else 0
            for k in range(len(units)):
                w[f"pts{i}"][_pos(k, i, W), off + _pos(k, i - 1, W)] = 1.0
        at = lambda j, s: _pos(unit_of[j, s], D - 1, W)
    vunits = [(j, s) for c, cols, _ in heads if views and c < 3 for j in cols for s in (1.0, -1.0)]
    vat = {u: (29 * q + 3) % (W // 2) for q, u in enumerate(vunits)}
    assert len(vunits) <= W // 2 and len(set(vat.values())) == len(vunits)
    feat = {}
    for c, cols, wts in heads:
        for j, wj in zip(cols, wts):
            if not views:
                w["output"][c, at(j, 1.0)], w["output"][c, at(j, -1.0)] = wj, -wj
            elif c == 3:
                w["alpha"][0, at(j, 1.0)], w["alpha"][0, at(j, -1.0)] = wj, -wj
            else:
                if route == "views":
                    w["views"][vat[j, 1.0], W + j], w["views"][vat[j, -1.0], W + j] = 1.0, -1.0
                else:
                    f = feat.setdefault(j, (41 * len(feat) + 7) % W)
                    w["feature"][f, at(j, 1.0)], w["feature"][f, at(j, -1.0)] = 1.0, -1.0
                    w["views"][vat[j, 1.0], f], w["views"][vat[j, -1.0], f] = 1.0, -1.0
                w["rgb"][c, vat[j, 1.0]], w["rgb"][c, vat[j, -1.0]] = wj, -wj
    net = dict(D=D, W=W, skips=skips, use_viewdirs=views, output_ch=cfg["output_ch"] if not views else 4, names=names,
               weights=[w[nm] for nm in names], biases=[np.zeros(rows[nm]) for nm in names], heads=heads, route=route,
               shape=shape, part=part, columns="probe", remainder=None)
    if alpha_bias is not None:
        net["biases"][names.index("alpha")] = np.array([float(alpha_bias)])
    _cache[key] = net
    return net


def tensors(net):
    return E.tensors(net)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _near_zeros():
    """fp32 numbers within two ulp of a zero of sin(2^l x) and of cos(2^l x), every level, both signs."""
    out = []
    for l in range(10):
        for phase in (0, 1):
            for k in (1, 3 + 5 * l, 2 ** l + 1):
                x = np.float32((k + 0.5 * phase) * np.pi / 2.0 ** l)
                if abs(x) > 8:
                    continue
                s = np.float32(-1.0 if (k + l) % 2 else 1.0)
                out += [s * x, s * np.nextafter(x, np.float32(9)), s * np.nextafter(np.nextafter(x, np.float32(0)), np.float32(0))]
    return np.array(out, dtype=np.float32)


def probe_points():
    """[321, 3] float32."""
    rng = np.random.default_rng(4101)
    t = 2.0 ** -20
    special = np.array([[0, 0, 8], [8, -0.0, 0], [-8, t, 0], [-0.0, -8, t], [t, t, -8], [-7.5, 0, -t], [8, 8, 8], [0, 0, 0],
                        [-0.0, -0.0, -0.0], [-8, -8, -8], [t, -t, t], [-3.25, 0, 1], [1, 2, 4], [-0.5, -0.25, -2]], dtype=np.float32)
    z = _near_zeros()
    near = rng.uniform(-2.5, 2.5, size=(len(z), 3)).astype(np.float32)
    near[np.arange(len(z)), np.arange(len(z)) % 3] = z
    rest = POINT_ROWS - len(special) - len(near)
    assert rest >= 100
    body = np.concatenate([rng.uniform(-2.5, 2.5, size=(rest // 2, 3)), rng.uniform(-8, 8, size=(rest - rest // 2, 3))]).astype(np.float32)
    pts = np.concatenate([body[:40], special, near, body[40:]])
    assert pts.shape == (POINT_ROWS, 3) and pts.dtype == np.float32 and np.abs(pts).max() == 8
    return pts


DIR_PERIOD = 11


def probe_dirs(R):
    """[R, 3] float32 view directions, period 11 rays: a run of three rays that share a unit direction, three rays that each
    differ from the one before in exactly one component (0, 1, 2 in turn), a run of two non-unit ones, again one component
    at a time, and a new direction."""
    rng = np.random.default_rng(4102)
    out = np.zeros((R, 3), dtype=np.float32)
    for base in range(0, R, DIR_PERIOD):
        a = rng.standard_normal(3)
        a = (a / np.linalg.norm(a)).astype(np.float32)
        b = (rng.uniform(0.3, 2.0) * rng.standard_normal(3)).astype(np.float32)
        c = rng.uniform(-1, 1, size=3).astype(np.float32)
        block = [a, a, a]
        for i in range(3):
            nxt = block[-1].copy()
            nxt[i] = np.float32(nxt[i] + (0.37 if nxt[i] < 0 else -0.37))
            block.append(nxt)
        block += [b, b]
        for i in (2, 0):
            nxt = block[-1].copy()
            nxt[i] = np.float32(-nxt[i] + 0.21)
            block.append(nxt)
        block.append(c)
        assert len(block) == DIR_PERIOD
        blk = np.stack(block)[: R - base]
        out[base:base + len(blk)] = blk
    if R > 4:                                       # exact zeros, a negative zero and a large component ride along
        out[R - 1] = np.array([0.0, -0.0, 1.0], dtype=np.float32)
    return out


def one_component_changes(dirs):
    """For every ray: the component in which alone it differs from the ray before (-1: none or several)."""
    out = np.full(len(dirs), -1)
    diff = dirs[1:] != dirs[:-1]
    one = diff.sum(axis=1) == 1
    out[1:][one] = diff[one].argmax(axis=1)
    return out


def ray_pool(shape):
    """The dyadic rays of exact_field.make_ray_pool for a shape: dict o, d, z (float64 values that are fp32 numbers)."""
    return E.make_ray_pool(E.NETWORKS[shape]["seed"], True)[1]


def ray_inputs(shape, R, N):
    """(o [R, 3], d [R, 3], z [R, N], pts [R, N, 3]) as float32, o + d z exact."""
    pool = ray_pool(shape)
    ray, rows = E.ray_indices(R, N, seed=R)
    o, d = pool["o"][ray], pool["d"][ray]
    z = pool["z"].reshape(-1)[rows]
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    f = np.float32
    assert E.is_f32(pts) and ((o.astype(f)[:, None, :] + d.astype(f)[:, None, :] * z.astype(f)[..., None]).astype(np.float64) == pts).all()
    return o.astype(f), d.astype(f), z.astype(f), pts.astype(f)


def input_sets(shape):
    """name -> dict(form, pts [R, N, 3], dirs [R, 3], and for the rays form o, d, z): everything a probe of the shape is run on."""
    if ("inputs", shape) in _cache:
        return _cache["inputs", shape]
    out = _cache["inputs", shape] = {"points321": dict(form="points", pts=probe_points()[:, None, :], dirs=probe_dirs(POINT_ROWS))}
    flat = probe_points()
    for R, N in RAY_SHAPES:
        idx = (np.arange(R * N) * 7) % POINT_ROWS
        out[f"points{R}x{N}"] = dict(form="points", pts=flat[idx].reshape(R, N, 3), dirs=probe_dirs(R))
        o, d, z, pts = ray_inputs(shape, R, N)
        out[f"rays{R}x{N}"] = dict(form="rays", pts=pts, dirs=probe_dirs(R), o=o, d=d, z=z)
    return out


# ---- the reference --------------------------------------------------------------------------------------------------
def gamma64(x, levels):
    """[x, sin(2^0 x), cos(2^0 x), ..] in float64 of fp32 inputs (run_nerf_helpers.py:15-63)."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    x = x.astype(np.float64)
    parts = [x]
    for l in range(levels):
        parts += [np.sin(x * 2.0 ** l), np.cos(x * 2.0 ** l)]
    return np.concatenate(parts, axis=-1)


def embedding64(pts, dirs, use_viewdirs=True):
    """[R N, 90] (63 without view directions) of pts [R, N, 3] and dirs [R, 3]."""
    R, N = pts.shape[:2]
    e = gamma64(pts.reshape(-1, 3), 10)
    if use_viewdirs:
        e = np.concatenate([e, np.repeat(gamma64(dirs, 4), N, axis=0)], axis=1)
    return e


def route_columns(net, e):
    """The route's own columns of embedding rows e."""
    return e[:, E.IN_PTS:] if net["route"] == "views" else e[:, :E.IN_PTS]


def reference(net, e):
    """raw64 [M, C] of embedding rows e (float64): the literal chain, ReLU masks on its own values."""
    return E.chain(net, e)


def gate(net, e, dtype):
    """[M, C]: the allowance of the module docstring; 0 for a head without columns."""
    x = route_columns(net, e)
    out = np.zeros((e.shape[0], net["output_ch"]))
    for c, cols, wts in net["heads"]:
        cols, wts = np.array(cols), np.abs(np.array(wts))
        size = np.ones((e.shape[0], len(cols)))
        if dtype in ROUNDED_DTYPES:
            ident = cols < 3
            size[:, ident] = np.maximum(np.abs(x[:, cols[ident]]), 1.0)
        out[:, c] = (size @ wts) * PROBE_TAU[dtype] + HEAD_ROUNDINGS[dtype] * U * (np.abs(x[:, cols]) @ wts)
    return out


def worst(raw, raw64, allow):
    """(max |raw - raw64| / gate, (row, channel)); a NaN, or any difference where the gate is 0, counts as infinite."""
    raw = np.asarray(raw, dtype=np.float64).reshape(raw64.shape)
    err = np.abs(raw - raw64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(allow > 0, err / allow, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isnan(raw), np.inf, ratio)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


# ---- an fp32 transcription of to_rev and Trig<> (ns_mlp_engine.h) ---------------------------------------------------
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


C_HI = float(np.float32(0.15915493667125702))
C_LO = float(np.float32(6.4206382432985265e-09))
TWO_PI32 = float(np.float32(6.283185307179586))
SERIES = [float(np.float32(v)) for v in (-2.5052108385441720e-08, 2.7557319223985893e-06, -1.9841269841269841e-04,
                                         8.3333333333333332e-03, -1.6666666666666666e-01)]


def to_rev32(x):
    """(hi, lo) of x / (2 pi): every step rounded to fp32 once; the products of two fp32 numbers are exact in float64, so each
    fused multiply-add is formed exactly and rounded once."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    hi = _f32(x * C_HI)
    err = _f32(x * C_HI - hi)
    assert (err == x * C_HI - hi).all()
    lo = _f32(x * C_LO + err)
    return hi, lo


def trig32(x, level, h, precise):
    """Trig<precise>(x)(level, h) as float64 values: sin(2^level x + h pi / 2).  precise: the series, every step in fp32.
    Otherwise float64's sine of the fp32 reduced argument, in revolutions: what v_sin_f32 is handed; its own error (2^-18,
    VSIN_ALLOWANCE) is not modelled."""
    hi, lo = to_rev32(x)
    scale = 2.0 ** level
    a = hi * scale
    # v_fract_f32: a - floor(a) rounded once and kept below 1.  Exact for a >= 0 and for a <= -1/2; a small negative a leaves
    # 1 - |a|, which [1/2, 1) holds to 2^-24 only
    f = np.minimum(_f32(a - np.floor(a)), 1.0 - 2.0 ** -24)
    assert ((f >= 0) & (f < 1)).all()
    assert (f == a - np.floor(a))[(a >= 0) | (a <= -0.5)].all()
    lo = _f32(lo * scale + 0.25 * h)
    if not precise:
        return np.sin(2.0 * np.pi * _f32(f + lo))
    f = _f32(np.where(f >= 0.5, f - 1.0, f) + lo)
    slack = 2.0 ** -14                      # |lo| <= 2^-24 2^9: a negative lo takes f below -1/2 by that much, and the fold below still holds
    assert ((f >= -0.5 - slack) & (f <= 1.0)).all()
    f = np.where(f > 0.5, f - 1.0, f)
    assert ((f >= -0.5 - slack) & (f <= 0.5)).all()
    g = np.where(f > 0.25, 0.5 - f, np.where(f < -0.25, -0.5 - f, f))
    assert (_f32(g) == g).all() and (np.abs(g) <= 0.25).all()
    t = _f32(g * TWO_PI32)
    t2 = _f32(t * t)
    p = SERIES[0]
    for c in SERIES[1:]:
        p = _f32(p * t2 + c)
    return _f32(_f32(p * t2) * t + t)


def gamma32(x, levels, precise):
    """gamma64's columns by the transcription."""
    x = np.asarray(x, dtype=np.float32)
    parts = [x.astype(np.float64)]
    for l in range(levels):
        parts += [trig32(x, l, 0, precise), trig32(x, l, 1, precise)]
    return np.concatenate(parts, axis=-1)


def embedding32(pts, dirs, precise, use_viewdirs=True):
    R, N = pts.shape[:2]
    e = gamma32(pts.reshape(-1, 3), 10, precise)
    if use_viewdirs:
        e = np.concatenate([e, np.repeat(gamma32(dirs, 4, precise), N, axis=0)], axis=1)
    return e


def operand(e, dtype):
    """Embedding rows as the engine of `dtype` holds them."""
    if dtype == "f32":
        return e
    if dtype == "f16x3":
        hi, lo = E.split(e)
        return hi + lo
    return E._round_to(e, torch.bfloat16 if dtype == "bf16" else torch.float16)


# ---- the mutants: faults of the embedding, one column at a time -----------------------------------------------------
COLUMN_MUTANTS = ("swapped", "level", "component", "zeroed")


def mutate_column(x3, e, j, kind):
    """The route's embedding columns e [M, n] of inputs x3 [M, 3] (float64) with column j wrong; None where `kind` does not apply
    (an identity column has no phase and no level)."""
    level, phase, comp = column_info(j)
    out = e.copy()
    trig = (np.sin, np.cos)
    n_levels = (e.shape[1] - 3) // 6
    if kind == "zeroed":
        out[:, j] = 0.0
    elif kind == "component":
        c2 = (comp + 1) % 3
        out[:, j] = x3[:, c2] if level < 0 else trig[phase](x3[:, c2] * 2.0 ** level)
    elif level < 0:
        return None
    elif kind == "swapped":
        out[:, j] = trig[1 - phase](x3[:, comp] * 2.0 ** level)
    elif kind == "level":
        l2 = level + 1 if level + 1 < n_levels else level - 1
        out[:, j] = trig[phase](x3[:, comp] * 2.0 ** l2)
    else:
        raise ValueError(kind)
    return out


def stash_exchanged(e):
    """Route skip: the two 32-column blocks of the embedded point come back from the stash exchanged (columns 0 .. 30 and
    32 .. 62; column 31 stays)."""
    out = e.copy()
    out[:, 0:31], out[:, 32:63] = e[:, 32:63], e[:, 0:31]
    return out


def stale_dirs(dirs):
    """The view direction of the previous ray, reused wherever exactly one component differs."""
    out = dirs.copy()
    ch = one_component_changes(dirs)
    for r in np.flatnonzero(ch >= 0):
        out[r] = dirs[r - 1]
    return out
