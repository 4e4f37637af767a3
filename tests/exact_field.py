"""Radiance fields on which every kernel must return one answer bit for bit.

Shared by tests/test_exact_field_host.py (the conditions below, the fold and the weight stream, on the CPU) and
tests/test_gpu_exact_field.py (the HIP kernels).  Nothing here calls the library.

The network is the reference's literal chain (run_nerf_helpers.py:67-134), not folded:

    h = x[:, :63];  for i in range(D): h = relu(pts_linears[i](h));  if i in skips: h = cat[x[:, :63], h]
    view directions:   alpha = alpha_linear(h);  feature = feature_linear(h)            (no activation)
                       hv = relu(views_linears.0(cat[feature, x[:, 63:]]));  raw = cat[rgb_linear(hv), alpha]
    otherwise:         raw = output_linear(h)

`make_exact_nerf` draws the weights so that, on a fixed pool of input rows, nothing is ever rounded:

    C1  every weight -- and every entry of the folded views_linears.0 o feature_linear the kernels run -- is a bf16 and an f16
        number;
    C2  every pool input and every post-ReLU activation on the pool is a bf16 and an f16 number;
    C3  in every layer and pool row, (sum_k |w_k a_k| + |b|) / q < 2^24, q the largest power of two that divides every term
        of the layer: every partial sum of any order is a multiple of q below 2^24 q, i.e. an fp32 number.  An fp32 FMA chain
        and an MFMA accumulator then hold the float64 sum at every step, in whatever order the engine walks k, and the
        float64 chain converted to fp32 is the only correct `raw`.  The folded evaluation is bounded the same way;
    C4  every hidden unit is positive on at least 10 % of the pool rows and zero on at least one, every permitted input
        column of every layer carries a nonzero weight, and no two neighbouring 16-row blocks hold the same biases;
    C5  zeroing any one 32-column input block or any one 16-row output block of any layer changes `raw` on some pool row.

C4 and C5 make a lost block, column or bias visible in `raw`; C1 - C3 make the comparison exact.  The conditions are the
functions `check_c1` .. `check_c5`; tests/test_exact_field_host.py asserts them for every entry of NETWORKS.

How the rows are drawn (`_draw_layer`), greedily, layer by layer and row by row.  A row is a few columns with coefficients
from {+-1/2, +-1, 2} and a bias from {-1, -1/2, 0, 1/2, 1}.  Every term of every sum is kept a multiple of one quantum q*
(half the quantum of the pool), so a coefficient 1/2 goes only to columns whose values are all multiples of 2 q*.  Row r is
seeded with the columns perm[r], perm[r + rows], ... of a permutation of the permitted columns, which covers every column,
starts up to 64 terms wide and is redrawn with half the terms until, on the whole pool, its activations are bf16 / f16
numbers, its sum of magnitudes stays below 0.9 * 2^12 q*, and it is positive on 10 % .. 35 % of the rows with values of at most
16 (layer 0, whose inputs are dense, is exempt from the upper limits: its rows keep all 63 terms).  Small, sparse
activations are what lets later rows stay wide: sums of many large terms would need more than 8 significant bits.  The last
resort, one term of weight 1 and no bias, copies an input column and always passes.  The bound 2^12 q* (not 2^24 q*) leaves
the 12 bits the remainder family below needs.  alpha_linear, rgb_linear and output_linear read every column with +-1, so
the layers in front of them also keep the pool-row sum of their activations below that bound; feature_linear takes +-1 and 2
and stays within 16, and a row of views_linears.0 is kept only if its folded row meets C1 and C3 as well.

`add_remainders(net, layer)` is the split-operand family for f16x3 and f32 handles: one layer's weights become
w (1 + 2^-12), i.e. hi = w and lo = w 2^-12 as f16 numbers.  That layer's inputs have no remainder (it exercises W_lo x_hi),
every later layer multiplies activations hi + lo by plain weights (W_hi x_lo), and W_lo x_lo, the term the engine drops, is
identically zero.  `check_remainders` asserts that, that every activation is hi + lo exactly, and C3 over the three products.
"""

import numpy as np
import torch

IN_PTS, IN_VIEWS = 63, 27
POOL_ROWS = 2048
RAY_POOL = (32, 64)                    # rays x samples of the pool of an "identity" network
COEFS = (-0.5, 0.5, -1.0, 1.0, 2.0)
COARSE = (-1.0, 1.0, 2.0)              # the coefficients that keep a column's quantum
COEFS_P = (0.3, 0.15, 0.3, 0.15, 0.1)  # how often a row draws each: negative on average, so that sums of activations stay small
COARSE_P = (0.6, 0.3, 0.1)
FULL = (-1.0, 1.0)                     # a row that reads every column (alpha, rgb, output): its terms keep one quantum and its
                                       # sum of magnitudes is the row sum of the activations
CANDIDATES = 16                        # rows tried at once on one choice of columns
AMAX, ACTIVE = 16.0, (0.10, 0.35)      # a hidden unit behind layer 0: its largest value and the share of the pool it is positive on
BIASES = (-1.0, -0.5, 0.0, 0.5, 1.0)
REMAINDER = 2.0 ** -12
ROW_COUNTS = (1, 15, 16, 17, 63, 64, 65, 79, 80, 81, 255, 256, 257, 319, 320, 321, 1300)
RAY_SHAPES = ((1, 1), (5, 7), (33, 31), (300, 64))

# name -> make_exact_nerf arguments: the table both test files walk
NETWORKS = {
    "prod": dict(D=8, W=256, skips=(4,), use_viewdirs=True, output_ch=4, seed=11),
    "d2w128": dict(D=2, W=128, skips=(), use_viewdirs=True, output_ch=4, seed=12),
    "d5w128s03": dict(D=5, W=128, skips=(0, 3), use_viewdirs=True, output_ch=4, seed=13),
    "d9w256": dict(D=9, W=256, skips=(4,), use_viewdirs=True, output_ch=4, seed=14),
    "d4w200out5": dict(D=4, W=200, skips=(2,), use_viewdirs=False, output_ch=5, seed=15),
    "d3w97": dict(D=3, W=97, skips=(), use_viewdirs=True, output_ch=4, seed=16),
}
COLUMNS = ("all", "identity")
REMAINDER_NETWORKS = ("prod", "d2w128")


def remainder_layers(name):
    """The layers that carry the remainders in turn: every point layer, the view layer, alpha and rgb."""
    return [f"pts{i}" for i in range(NETWORKS[name]["D"])] + ["views", "alpha", "rgb"]


# ---- number formats -------------------------------------------------------------------------------------------------
def _round_to(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype).double().numpy()


def half(a):
    """a (float64) rounded to f16, as float64."""
    return _round_to(a, torch.float16)


def fits16(a):
    """True where a is a bf16 and an f16 number, zero or normal in both."""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)                                    # |m| in [1/2, 1): 8 significant bits <=> 256 m is an integer
    m = m * 256.0
    return (m == np.rint(m)) & ((a == 0) | ((e >= -13) & (e <= 16)))


def quantum(a):
    """The largest power of two that divides every entry of a (inf for all zeros)."""
    a = np.abs(np.asarray(a, dtype=np.float64).ravel())
    a = a[a != 0]
    if a.size == 0:
        return np.inf
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    return float(np.min(low * 2.0 ** (e.astype(np.float64) - 53)))


def column_quanta(a):
    a = np.asarray(a)
    return np.array([quantum(a[:, k]) for k in range(a.shape[1])])


# ---- pools ----------------------------------------------------------------------------------------------------------
def make_pool(seed, use_viewdirs, rows=POOL_ROWS):
    """rows x 90 (63 without view directions) multiples of 1/2 in [-2, 2]."""
    rng = np.random.default_rng(seed)
    return rng.integers(-4, 5, size=(rows, IN_PTS + (IN_VIEWS if use_viewdirs else 0))).astype(np.float64) / 2


def make_ray_pool(seed, use_viewdirs, rays=RAY_POOL[0], samples=RAY_POOL[1]):
    """The pool of an "identity" network: row r * samples + n is sample n of ray r.  Columns 0..2 hold o + d z with o and z
    multiples of 1/4 (|o| <= 2, 1/4 <= z <= 4) and d from {0, +-1/2, +-1}: multiples of 1/8 of at most 6.  Columns 63..65
    hold the ray's view direction, multiples of 1/4 in [-1, 1], not normalised.  The other columns are those of `make_pool`:
    the kernels put sines and cosines there, which an identity network multiplies by zero.
    Returns (pool, dict(o, d, z, viewdirs))."""
    rng = np.random.default_rng(seed + 7919)
    pool = make_pool(seed, use_viewdirs, rays * samples)
    o = rng.integers(-8, 9, size=(rays, 3)).astype(np.float64) / 4
    d = rng.choice(np.array([0.0, 0.5, -0.5, 1.0, -1.0]), size=(rays, 3))
    d[np.all(d == 0, axis=1), 0] = 1.0
    z = rng.integers(1, 17, size=(rays, samples)).astype(np.float64) / 4
    v = rng.integers(-4, 5, size=(rays, 3)).astype(np.float64) / 4
    pts = o[:, None, :] + d[:, None, :] * z[:, :, None]
    pool[:, 0:3] = pts.reshape(-1, 3)
    if use_viewdirs:
        pool[:, IN_PTS:IN_PTS + 3] = np.repeat(v, samples, axis=0)
    return pool, dict(o=o, d=d, z=z, viewdirs=v)


# ---- the literal chain ----------------------------------------------------------------------------------------------
def layer_names(D, use_viewdirs):
    """pack_nerf's tensor order."""
    return [f"pts{i}" for i in range(D)] + (["feature", "alpha", "views", "rgb"] if use_viewdirs else ["output"])


def chain(net, x, weights=None, biases=None, keep=False):
    """The literal chain in float64 on rows x.  With keep: (raw, dict layer name -> (input, pre-activation))."""
    w = dict(zip(net["names"], net["weights"] if weights is None else weights))
    b = dict(zip(net["names"], net["biases"] if biases is None else biases))
    x = np.asarray(x, dtype=np.float64)
    pts, views = x[:, :IN_PTS], x[:, IN_PTS:]
    seen = {}

    def lin(name, inp):
        pre = inp @ w[name].T + b[name]
        if keep:
            seen[name] = (inp, pre)
        return pre

    h = pts
    for i in range(net["D"]):
        h = np.maximum(lin(f"pts{i}", h), 0.0)
        if i in net["skips"]:
            h = np.concatenate([pts, h], axis=1)
    if net["use_viewdirs"]:
        alpha = lin("alpha", h)
        feature = lin("feature", h)
        hv = np.maximum(lin("views", np.concatenate([feature, views], axis=1)), 0.0)
        raw = np.concatenate([lin("rgb", hv), alpha], axis=1)
    else:
        raw = lin("output", h)
    return (raw, seen) if keep else raw


def fold_views(net, weights=None, biases=None):
    """views_linears.0 o feature_linear in float64: ([W/2, W + 27], [W/2]) on cat[h, dirs]."""
    w = dict(zip(net["names"], net["weights"] if weights is None else weights))
    b = dict(zip(net["names"], net["biases"] if biases is None else biases))
    W = net["W"]
    wv = w["views"]
    return np.concatenate([wv[:, :W] @ w["feature"], wv[:, W:]], axis=1), wv[:, :W] @ b["feature"] + b["views"]


def kernel_layers(net, x=None):
    """The layers as the kernels run them -- the point layers, alpha, the folded view layer, rgb (or output) -- each as
    (name, weights, bias, input on the rows x (default: the pool), relu)."""
    x = net["pool"] if x is None else x
    _, seen = chain(net, x, keep=True)
    w = dict(zip(net["names"], net["weights"]))
    b = dict(zip(net["names"], net["biases"]))
    out = [(f"pts{i}", w[f"pts{i}"], b[f"pts{i}"], seen[f"pts{i}"][0], True) for i in range(net["D"])]
    if net["use_viewdirs"]:
        wf, bf = fold_views(net)
        h = seen["alpha"][0]
        out.append(("alpha", w["alpha"], b["alpha"], h, False))
        out.append(("views", wf, bf, np.concatenate([h, np.asarray(x)[:, IN_PTS:]], axis=1), True))
        out.append(("rgb", w["rgb"], b["rgb"], seen["rgb"][0], False))
    else:
        out.append(("output", w["output"], b["output"], seen["output"][0], False))
    return out


def folded_chain(net, x):
    """`raw` through `kernel_layers`: float64, the view layer folded."""
    res = {}
    for name, w, b, inp, relu in kernel_layers(net, x):
        res[name] = inp @ w.T + b
    if net["use_viewdirs"]:
        hv = np.maximum(res["views"], 0.0)
        w = dict(zip(net["names"], net["weights"]))
        b = dict(zip(net["names"], net["biases"]))
        return np.concatenate([hv @ w["rgb"].T + b["rgb"], res["alpha"]], axis=1)
    return res["output"]


def input_blocks(net, name):
    """The 32-column blocks of a layer's input, per segment of its concatenation, as (first column, end)."""
    W, D = net["W"], net["D"]
    x = [(0, 32), (32, IN_PTS)]

    def hidden(off, n):
        return [(off + k, off + min(k + 32, n)) for k in range(0, n, 32)]

    if name == "pts0":
        return x
    if name.startswith("pts"):
        return x + hidden(IN_PTS, W) if (int(name[3:]) - 1) in net["skips"] else hidden(0, W)
    if name == "views":
        return hidden(0, W) + [(W, W + IN_VIEWS)]
    if name == "rgb":
        return hidden(0, W // 2)
    return hidden(0, W)               # feature, alpha, output


def permitted_columns(net, name):
    """The input columns of a layer that may carry a weight: all of them, or with columns="identity" only the raw
    coordinates among the columns of the embedded input."""
    K = dict(zip(net["names"], net["weights"]))[name].shape[1]
    if net["columns"] == "all":
        return np.arange(K)
    W = net["W"]
    if name == "pts0":
        return np.arange(3)
    if name.startswith("pts") and (int(name[3:]) - 1) in net["skips"]:
        return np.concatenate([np.arange(3), np.arange(IN_PTS, IN_PTS + W)])
    if name == "views":
        return np.concatenate([np.arange(W), np.arange(W, W + 3)])
    return np.arange(K)


# ---- the generator --------------------------------------------------------------------------------------------------
class _Unfit(Exception):
    pass


def _draw_layer(rng, inp, rows, permitted, relu, qstar, sbound, *, tbound=None, coarse_only=False, full=False, accept=None,
                sparse=True, start=64, limit=None, one_seed=False):
    """One layer on the pool input `inp` [P, K]: (weights [rows, K], bias [rows], pre-activations [P, rows]).
    sbound: the bound on a row's sum of magnitudes; tbound: on the pool-row sum of the layer's activations (a layer that full
    rows read); coarse_only: no coefficient 1/2; full: every row reads every permitted column with +-1; sparse: a hidden unit
    stays within AMAX and ACTIVE; start: the widest row; limit: the largest |pre-activation| of a layer without ReLU;
    accept(columns, coefficients, bias): a further condition on a row; one_seed: a row is seeded with one column even where
    there are more columns than rows."""
    P, K = inp.shape
    # the trial rows are evaluated in fp32 on the transposed pool: every value that passes the bounds below is exact there
    # (a multiple of q* below 2^24 q*), and the conditions are asserted afterwards in float64 (check_c1 .. check_c5)
    inp_t = np.ascontiguousarray(inp.T, dtype=np.float32)
    abs_t = np.abs(inp_t)
    fine = column_quanta(inp)[permitted] < 2 * qstar      # columns that take no coefficient 1/2
    perm = rng.permutation(len(permitted))
    everything = np.arange(len(permitted))
    w = np.zeros((rows, K))
    bias = np.zeros(rows)
    pre_all = np.zeros((P, rows))
    total = np.zeros(P, dtype=np.float32)
    widest = start

    def attempt(seeds, n, coarse, copy):
        cols = seeds
        if n > len(seeds):
            free = np.ones(len(permitted), dtype=bool)
            free[seeds] = False
            cols = np.concatenate([seeds, rng.choice(everything[free], size=n - len(seeds), replace=False)])
        c = permitted[cols]
        # CANDIDATES rows on these columns at once: coefficients [CANDIDATES, n], one bias each
        if full:
            coef = rng.choice(FULL, size=(CANDIDATES, len(cols)))
        elif coarse:
            coef = rng.choice(COARSE, size=(CANDIDATES, len(cols)), p=COARSE_P)
        else:
            coef = rng.choice(COEFS, size=(CANDIDATES, len(cols)), p=COEFS_P)
            bad = fine[cols][None, :] & (np.abs(coef) < 1)
            coef[bad] = rng.choice(COARSE, size=int(bad.sum()), p=COARSE_P)
        bval = rng.choice(BIASES, size=CANDIDATES)
        if copy:
            coef, bval = np.ones((1, 1)), np.zeros(1)
        coef32 = coef.astype(np.float32)
        ok = (np.abs(coef32) @ abs_t[c]).max(axis=1) + np.abs(bval) <= sbound
        if not ok.any():
            return None
        pre = coef32 @ inp_t[c] + bval.astype(np.float32)[:, None]
        if limit is not None and not copy:
            ok &= np.abs(pre).max(axis=1) <= limit
        if relu:
            act = np.maximum(pre, 0.0)
            share = (act > 0).mean(axis=1)
            ok &= (share >= ACTIVE[0]) & (share < 1.0)
            if sparse and not copy:
                ok &= (share <= ACTIVE[1]) & (act.max(axis=1) <= AMAX)
            if tbound is not None and not copy:
                ok &= ((total[None, :] + act).max(axis=1) <= tbound) & (act.mean(axis=1) <= 0.45 * tbound / rows)
            for j in np.flatnonzero(ok):
                ok[j] = fits16(act[j]).all()
        for j in np.flatnonzero(ok):
            if accept is None or accept(c, coef[j], float(bval[j])):
                return c, coef[j], float(bval[j]), pre[j].astype(np.float64)
        return None

    for r in range(rows):
        if full:
            seeds = np.arange(len(permitted))
        elif len(perm) >= rows and not one_seed:
            seeds = perm[r::rows]
        else:
            seeds = perm[[r % len(perm)]]
        n = max(len(seeds), min(start, len(permitted)))
        coarse, stuck, got = coarse_only, 0, None
        while got is None:
            for _ in range(3):
                got = attempt(seeds, n, coarse, False)
                if got is not None:
                    break
            if got is not None:
                break
            if n > len(seeds):
                n = max(len(seeds), n // 2)
                continue
            stuck += 1
            if len(seeds) == 1 and stuck >= 3:          # the last resort: copy the seeded column
                got = attempt(seeds, 1, True, True)
                if got is None:
                    raise _Unfit("a column cannot be copied")
            coarse = True
            if stuck > 40:
                raise _Unfit("a forced row does not fit")
        c, coef, bval, pre = got
        if relu and tbound is not None:
            total += np.maximum(pre, 0.0)
        w[r, c] = coef
        bias[r] = bval
        pre_all[:, r] = pre
        start = min(widest, max(2 * n, 2))
    return w, bias, pre_all


def make_exact_nerf(D, W, skips, use_viewdirs, output_ch, seed, columns="all", pool=None):
    """The reference-order weight and bias lists that ops.pack_nerf takes (float64 arrays whose values are fp32 numbers) and
    the float64 `raw` of the literal chain on the pool, as a dict: D, W, skips, use_viewdirs, output_ch, columns, names,
    weights, biases, pool, raw, rays (the ray pool's o, d, z, viewdirs; None for columns="all").

    pool: [P, 90] (63 without view directions) exactly representable rows; default `make_pool(seed)` for columns="all",
    `make_ray_pool(seed)` for columns="identity"."""
    assert columns in COLUMNS and all(0 <= s < D - 1 for s in skips)
    rays = None
    if pool is None:
        if columns == "all":
            pool = make_pool(seed, use_viewdirs)
        else:
            pool, rays = make_ray_pool(seed, use_viewdirs)
    pool = np.asarray(pool, dtype=np.float64)
    net = dict(D=D, W=W, skips=tuple(skips), use_viewdirs=bool(use_viewdirs), output_ch=output_ch if not use_viewdirs else 4,
               columns=columns, names=layer_names(D, use_viewdirs), pool=pool, rays=rays, remainder=None)
    qstar = quantum(pool) / 2
    # identity networks run no remainder family: their sums only need to stay fp32-exact
    sbound = 0.9 * (2.0 ** 12 if columns == "all" else 2.0 ** 22) * qstar
    tbound = sbound - 1.0             # a full row takes +-1: its sum of magnitudes is the row sum of its inputs, plus a bias
    shapes = {"pts0": IN_PTS}
    for i in range(1, D):
        shapes[f"pts{i}"] = W + IN_PTS if (i - 1) in skips else W
    shapes.update(feature=W, alpha=W, views=W + IN_VIEWS, rgb=W // 2, output=W)
    net["weights"] = [np.zeros((1, shapes[n])) for n in net["names"]]       # placeholders for permitted_columns
    for attempt in range(20):
        rng = np.random.default_rng([seed, attempt, COLUMNS.index(columns)])
        try:
            ws, bs = {}, {}
            pts, views = pool[:, :IN_PTS], pool[:, IN_PTS:]
            h = pts
            for i in range(D):
                name = f"pts{i}"
                tight = i == D - 1
                ws[name], bs[name], pre = _draw_layer(rng, h, W, permitted_columns(net, name), True, qstar, sbound,
                                                      tbound=tbound if tight else None, sparse=i > 0)
                h = np.maximum(pre, 0.0)
                if i in skips:
                    h = np.concatenate([pts, h], axis=1)
            if use_viewdirs:
                ws["alpha"], bs["alpha"], _ = _draw_layer(rng, h, 1, np.arange(W), False, qstar, sbound, full=True)
                # feature_linear and the feature columns of views_linears.0 take +-1 and 2 only: the folded entries stay small
                ws["feature"], bs["feature"], feat = _draw_layer(rng, h, W, np.arange(W), False, qstar, sbound, coarse_only=True,
                                                                 start=8, limit=AMAX)
                vin = np.concatenate([feat, views], axis=1)
                hin, wfeat, bfeat = np.abs(np.concatenate([h, views], axis=1)), ws["feature"], bs["feature"]

                def folded_ok(c, coef, bval):           # the row of views_linears.0 o feature_linear: C1 and C3
                    row = np.zeros(W + IN_VIEWS)
                    row[c] = coef
                    wf = np.concatenate([row[:W] @ wfeat, row[W:]])
                    return bool(fits16(wf).all()) and float((hin @ np.abs(wf)).max()) + abs(row[:W] @ bfeat + bval) <= sbound

                wv, bv, pre = _draw_layer(rng, vin, W // 2, permitted_columns(net, "views"), True, qstar, sbound,
                                          tbound=tbound, accept=folded_ok, sparse=False)
                ws["views"], bs["views"] = wv, bv
                hv = np.maximum(pre, 0.0)
                ws["rgb"], bs["rgb"], _ = _draw_layer(rng, hv, 3, np.arange(W // 2), False, qstar, sbound, full=True)
            else:
                ws["output"], bs["output"], _ = _draw_layer(rng, h, output_ch, np.arange(W), False, qstar, sbound, full=True)
            break
        except _Unfit:
            continue
    else:
        raise RuntimeError("make_exact_nerf: no network fits the conditions; change the generator, not the conditions")
    net["weights"] = [ws[n] for n in net["names"]]
    net["biases"] = [bs[n] for n in net["names"]]
    net["raw"] = chain(net, pool)
    return net


def add_remainders(net, layer):
    """A copy of `net` whose layer `layer` ("pts<i>", "views", "alpha", "rgb", "output") has the weights w (1 + 2^-12); the
    biases stay.  "views" means views_linears.0 alone: feature_linear stays plain, so the folded layer is F (1 + 2^-12)."""
    assert net["remainder"] is None and layer in net["names"] and layer != "feature"
    out = dict(net)
    out["weights"] = [w * (1.0 + REMAINDER) if n == layer else w for n, w in zip(net["names"], net["weights"])]
    out["remainder"] = layer
    out["raw"] = chain(out, out["pool"])
    return out


# ---- the conditions -------------------------------------------------------------------------------------------------
def is_f32(a):
    a = np.asarray(a, dtype=np.float64)
    return bool((a.astype(np.float32).astype(np.float64) == a).all())


def check_c1(net):
    """Every weight, folded view layer included, is a bf16 and an f16 number; every bias an fp32 number."""
    assert net["remainder"] is None
    for name, w, b, _, _ in kernel_layers(net):
        assert fits16(w).all(), f"C1: {name} has a weight that is no bf16 / f16 number"
        assert is_f32(b), f"C1: {name} has a bias that is no fp32 number"
    for name, w, b in zip(net["names"], net["weights"], net["biases"]):
        assert fits16(w).all() and is_f32(b), f"C1: {name}"
        assert set(np.unique(np.abs(w))) <= {0.0, 0.5, 1.0, 2.0} and set(np.unique(b)) <= set(BIASES), f"C1: {name} leaves the coefficient set"


def check_c2(net):
    """Every pool input and every post-ReLU activation on the pool is a bf16 and an f16 number."""
    assert fits16(net["pool"]).all(), "C2: pool"
    for name, w, b, inp, relu in kernel_layers(net):
        assert fits16(inp).all(), f"C2: an input of {name} is no bf16 / f16 number"


def split(a):
    """(hi, lo) = (half(a), half(a - hi))."""
    hi = half(a)
    return hi, half(np.asarray(a, dtype=np.float64) - hi)


def _c3_layer(name, w, b, inp, do_split):
    if do_split:
        (wh, wl), (xh, xl) = split(w), split(inp)
        prods = [(wh, xh), (wh, xl), (wl, xh)]
    else:
        prods = [(w, inp)]
    total = np.abs(b)[None, :]
    q = quantum(b)
    for ww, xx in prods:
        if not ww.any() or not xx.any():
            continue
        total = total + np.abs(xx) @ np.abs(ww).T
        q = min(q, quantum(ww) * quantum(xx))
    assert np.isfinite(q) and float(total.max()) < 2.0 ** 24 * q, f"C3: {name}: sum of magnitudes {float(total.max())} on quantum {q}"
    return float(total.max()) / q


def check_c3(net, do_split=False):
    """(sum_k |w_k a_k| + |b|) / q < 2^24 in every layer and pool row, for the literal chain and the folded view layer; with
    do_split over the three products of the split engine.  Returns the largest ratio."""
    worst = 0.0
    _, seen = chain(net, net["pool"], keep=True)
    for name, w, b in zip(net["names"], net["weights"], net["biases"]):
        worst = max(worst, _c3_layer(name, w, b, seen[name][0], False))
    for name, w, b, inp, _ in kernel_layers(net):
        worst = max(worst, _c3_layer(name + " (kernel)", w, b, inp, do_split))
    assert is_f32(net["raw"]), "C3: raw is no fp32 number"
    return worst


def check_c4(net):
    """Hidden units active on >= 10 % of the pool and zero somewhere; every permitted input column of every layer read;
    neighbouring 16-row blocks of biases differ."""
    _, seen = chain(net, net["pool"], keep=True)
    for name, w, b in zip(net["names"], net["weights"], net["biases"]):
        if name.startswith("pts") or name == "views":
            act = np.maximum(seen[name][1], 0.0)
            assert ((act > 0).mean(axis=0) >= 0.10).all(), f"C4: a unit of {name} is positive on less than 10 % of the pool"
            assert (act == 0).any(axis=0).all(), f"C4: a unit of {name} is never zero"
            blocks = [tuple(b[k:k + 16]) for k in range(0, len(b), 16)]
            assert all(x != y for x, y in zip(blocks, blocks[1:]) if len(x) == len(y)), f"C4: {name}: equal neighbouring bias blocks"
        cols = permitted_columns(net, name)
        assert (w[:, cols] != 0).any(axis=0).all(), f"C4: an input column of {name} has no weight"
        rest = np.setdiff1d(np.arange(w.shape[1]), cols)
        assert not w[:, rest].any(), f"C4: {name} reads a column outside the permitted ones"


def check_c5(net, rows=512):
    """Zeroing one 32-column input block, or one 16-row output block (weights and biases), of any layer changes raw on
    the first `rows` pool rows.  Input blocks without a permitted column (identity networks) are left out."""
    x = net["pool"][:rows]
    base = chain(net, x)
    for i, name in enumerate(net["names"]):
        w, b = net["weights"][i], net["biases"][i]
        cols = permitted_columns(net, name)
        for lo, hi in input_blocks(net, name):
            if not ((cols >= lo) & (cols < hi)).any():
                continue
            w2 = w.copy()
            w2[:, lo:hi] = 0
            ws = list(net["weights"])
            ws[i] = w2
            assert (chain(net, x, weights=ws) != base).any(), f"C5: input block {lo}..{hi} of {name} does not reach raw"
        for lo in range(0, w.shape[0], 16):
            w2, b2 = w.copy(), b.copy()
            w2[lo:lo + 16] = 0
            b2[lo:lo + 16] = 0
            ws, bs = list(net["weights"]), list(net["biases"])
            ws[i], bs[i] = w2, b2
            assert (chain(net, x, weights=ws, biases=bs) != base).any(), f"C5: output block {lo} of {name} does not reach raw"


def check_remainders(net):
    """The remainder family's conditions: the weights are fp32 numbers that split into two f16 numbers, every activation is
    hi + lo exactly, in every layer W_lo = 0 or x_lo = 0, the layer with the remainders sees W_lo != 0, every later
    hidden layer x_lo != 0, and C3 holds over the three products.  Returns the largest C3 ratio."""
    layer = net["remainder"]
    assert layer is not None
    order = [n for n, *_ in kernel_layers(net)]
    for name, w, b, inp, relu in kernel_layers(net):
        assert is_f32(w) and is_f32(b), f"{name}: not fp32"
        wh, wl = split(w)
        xh, xl = split(inp)
        assert (wh + wl == w).all(), f"{name}: a weight is not hi + lo"
        assert (xh + xl == inp).all(), f"{name}: an activation is not hi + lo"
        assert not wl.any() or not xl.any(), f"{name}: W_lo x_lo is not identically zero"
        if name == layer:
            assert (wh == w / (1.0 + REMAINDER)).all() and (wl == wh * REMAINDER).all() and wl.any() and not xl.any(), name
        else:
            assert not wl.any(), name
            # alpha and the view layer read the same activations: behind the point layers every layer sees remainders
            feeds = order.index(name) > order.index(layer) and not (layer == "alpha") and not (layer == "views" and name == "alpha")
            assert bool(xl.any()) == feeds, f"{name}: x_lo {'missing' if feeds else 'present'}"
    return check_c3(net, do_split=True)


# ---- what the GPU tests feed and expect -----------------------------------------------------------------------------
_cache = {}


def network(name, columns="all"):
    """The cached network of NETWORKS[name]."""
    key = (name, columns)
    if key not in _cache:
        _cache[key] = make_exact_nerf(columns=columns, **NETWORKS[name])
    return _cache[key]


def remainder_network(name, layer):
    key = (name, "all", layer)
    if key not in _cache:
        _cache[key] = add_remainders(network(name), layer)
    return _cache[key]


def tensors(net):
    """(weights, biases) as the fp32 torch tensors ops.pack_nerf takes."""
    return ([torch.from_numpy(w).float() for w in net["weights"]], [torch.from_numpy(b).float() for b in net["biases"]])


def row_indices(M, seed=0):
    """M pool rows by a fixed permutation (repeated beyond the pool's size)."""
    perm = np.random.default_rng(1000 + seed).permutation(POOL_ROWS)
    return perm[np.arange(M) % POOL_ROWS]


def ray_indices(R, N, seed=0):
    """For R rays of N <= 64 samples: (ray r's pool ray [R], its samples' pool rows [R, N])."""
    rng = np.random.default_rng(2000 + seed)
    rays, samples = RAY_POOL
    ray = rng.permutation(max(R, rays))[:R] % rays
    samp = np.stack([rng.permutation(samples)[:N] for _ in range(R)])
    return ray, ray[:, None] * samples + samp


def first_difference(got, want):
    """'' if equal as values (-0.0 == 0.0, NaN equals nothing), else the first differing (row, channel), the row's position
    in the tiles of the three engines, and both values."""
    got = got.reshape(-1, got.shape[-1])
    want = want.reshape(-1, want.shape[-1])
    if torch.equal(got, want):
        return ""
    bad = (got != want).nonzero()
    r, c = int(bad[0, 0]), int(bad[0, 1])
    return (f"{bad.shape[0]} of {got.numel()} values differ; first at row {r} channel {c} (row % 16, 64, 80, 320 = {r % 16}, {r % 64}, "
            f"{r % 80}, {r % 320}): got {float(got[r, c])!r}, expected {float(want[r, c])!r}")
