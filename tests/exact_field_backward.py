"""The field fit's backward pass on the exactly representable networks of tests/exact_field.py: one answer, bit for bit.

Shared by tests/test_exact_field_backward_host.py (the conditions below, the mutants and torch-CPU autograd, on the CPU) and
tests/test_gpu_exact_field_backward.py (autograd._nerf_layers_forward / _nerf_layers_backward, NerfFunction and NerfInputGrad on
both GEMM engines).  Nothing here calls the library.

`backward64` is the literal transposed chain of `exact_field.chain` in float64: from an integer `d raw` down to `d xe`, with
`dW = dy^T x` and `db = sum_m dy` of every Linear; the derivative of a ReLU is `pre > 0`.  The weights are from
{+-1/2, +-1, 2}, the activations on the pool are short dyadic numbers and `d raw` holds small integers, so every product of the
backward is a product of two dyadic numbers, and the conditions make every sum of them an fp32 number in any order:

    B1  every entry of `d raw`, of every saved activation (each Linear's input on the chosen rows) and of every weight is an fp32
        number with at most 8 significant bits (a bf16 and an f16 number: exact_field's C1 and C2 on these rows);
    B2  no pre-activation of a ReLU layer on the chosen rows lies in (0, q_layer), q_layer the quantum of the layer's terms: a
        pre-activation is a multiple of q_layer, so it is either at least q_layer or exactly <= 0, it is computed exactly in fp32
        (C3), and no mask can differ between fp32 and float64;
    B3  for every GEMM of the backward, (sum_k |a_ik b_kj|) / q < 2^24 in every output element, q the product of the two
        operands' quanta: every partial sum, in any order and through any split of k, is a multiple of q below 2^24 q, an fp32
        number.  The grad-input products that are summed into one tensor -- feature_linear's and alpha_linear's into `d_h`, layer
        0's and every skip layer's embedding share into `d xe` -- are bounded over the joined sum; `dW = dy^T x` (k = the rows)
        and `db` (x = 1) are bounded like any other product.  A condition, not a tolerance: where a case exceeded it the draw was
        thinned (THIN below), never the bound widened;
    B4  visibility: with at least BLOCK_ROWS rows every 16-row block of every `dW` and every 16-entry block of every `db` holds a
        nonzero entry (with fewer rows no gradient tensor is identically zero), `d xe` is not zero, and every mutant of MUTANTS
        changes at least one compared value on every case it applies to.

The float64 backward converted to fp32 is then the only correct `d xe`, `dW` and `db`, on either engine and through
ns_gemm_wgrad's split of the rows.  The conditions are the functions `check_b1` .. `check_b4`; the host test asserts them for
every case of the table (`chain_case` at CHAIN_M, `ray_case` at exact_field.RAY_SHAPES) the GPU test walks.

The cases.  On the "all" networks the chain runs on pool rows (`exact_field.row_indices`) at CHAIN_M row counts: 1024 | 1025 is
the first split of ns_gemm_wgrad, 17 and 257 leave partial tiles.  `d raw` is drawn from {-1, 0, 1}, at M = 4097 from {-2 .. 2}.
On the "identity" networks the public path embeds the points itself (exact_field.RAY_SHAPES): the sines and cosines carry zero
weights, so the forward, `d pts` (= the identity columns of `d xe`), every `db` and every `dW` column that multiplies an identity
or hidden input stay exact -- the conditions are asserted with the sine and cosine columns of the input set to zero, which leaves
exactly those products.  The `dW` columns of layer 0, of the layers behind a skip and of the view layer that multiply sines and
cosines are held to `ray_case`'s bound instead: against the float64 sum with float64 sines and cosines of the same fp32 points,
rows * 2^-24 * sum_m |dy x| (the order-independent bound of an fp32 sum, as in tests/test_gpu_wgrad.py) plus
train_kernels_reference.TRIG * sum_m |dy| for the encoding's own error (dy is exact).

Worst B3 figure (sum of magnitudes / quantum, as a power of two) per network over its cases, as the host test prints it:

    network       "all", M <= 1300    "all", M = 4097    "identity", RAY_SHAPES
    prod              2^20.63             2^23.00             2^23.56  (300 x 64, one full row of d raw per block of 16)
    d2w128            2^18.04             2^20.42             2^22.69  (300 x 64, dense)
    d5w128s03         2^18.68             2^21.22             2^23.14  (300 x 64, a quarter of the rows)
    d9w256            2^21.10             2^23.43             2^23.73  (33 x 31, dense; 300 x 64, one entry per block: 2^23.30)
    d4w200out5        2^17.45             2^19.88             2^21.65  (300 x 64, a quarter of the rows)
    d3w97             2^18.94             2^21.40             2^21.54  (300 x 64, a quarter of the rows)

The worst product is a `dW` (k runs over the rows: `dW pts1` on the "all" networks, `dW pts0` on the "identity" ones) everywhere
but on one to 35 rows of an "identity" network, where it is the joined sum into `d xe`.  The identity networks' activations are
larger (exact_field draws them against 2^22 q*, not 2^12 q*), which is why their 19200-row case is thinned (THIN).
"""

import numpy as np

import exact_field as E
import train_kernels_reference as T

CHAIN_M = (1, 17, 257, 1024, 1025, 1300, 4097)
WIDE_M = 4097                      # the chain's largest row count: d raw is drawn from {-2 .. 2}
BLOCK_ROWS = 257                   # from this row count on, B4 asks for a nonzero entry in every 16-row block
SLICE = 1024                       # rows of one split-K slice of ns_gemm_wgrad
LIMIT = 2.0 ** 24

# (network, columns, rows) -> make_draw's arguments where the dense draw exceeds B3 (its figure in front): the first rung of
# density 1/4, 1/16, 0 (one full row in every block of 16), one_channel that the float64 reference alone meets
THIN = {
    ("d3w97", "identity", 19200): dict(density=0.25),            # 2^24.05
    ("d4w200out5", "identity", 19200): dict(density=0.25),       # 2^24.13
    ("d5w128s03", "identity", 19200): dict(density=0.25),        # 2^25.61
    ("prod", "identity", 19200): dict(density=0.0),              # 2^28.02; 2^24.38 at 1/16
    ("d9w256", "identity", 19200): dict(one_channel=True),       # 2^28.70; 2^24.23 at 0
}

MASK_OFFSETS = {"mask_from_layer_above": 1, "mask_from_two_layers_above": 2, "mask_from_layer_below": -1}
MUTANTS = ("sigma_not_accumulated", "sigma_after_mask", "skip_embedding_dropped", "skip_split_62", "skip_split_64",
           "mask_from_layer_above", "mask_from_two_layers_above", "mask_from_layer_below", "last_mask_skipped",
           "view_last_columns", "draw_contiguous_blocks", "dw_from_output", "db_last_row_missing", "dw_last_slice_missing",
           "output_ch_4")


def applies(mutant, net, M):
    """Whether a mutant is another computation than the chain on this network and row count at all."""
    view = net["use_viewdirs"]
    if mutant in ("sigma_not_accumulated", "sigma_after_mask", "view_last_columns"):
        return view
    if mutant == "draw_contiguous_blocks":
        return view and M > 1                      # one row is one block either way
    if mutant in ("skip_embedding_dropped", "skip_split_62", "skip_split_64"):
        return len(net["skips"]) > 0
    if mutant == "dw_last_slice_missing":
        return M % SLICE != 0
    if mutant == "output_ch_4":
        return not view and net["output_ch"] != 4
    return True


# ---- the transposed chain ---------------------------------------------------------------------------------------------------
def _product(pairs, label, trace):
    """sum of A @ B over the pairs; with a trace list, appends (label, worst sum of magnitudes / quantum of the joined sum)."""
    out = None
    for A, B in pairs:
        out = A @ B if out is None else out + A @ B
    if trace is not None:
        mag, q = 0.0, np.inf
        for A, B in pairs:
            if A.any() and B.any():
                mag = mag + np.abs(A) @ np.abs(B)
                q = min(q, E.quantum(A) * E.quantum(B))
        trace.append((label, float(np.max(mag)) / q if np.isfinite(q) else 0.0))
    return out


def backward64(net, x, draw, mutant=None, trace=None, keep_dy=(), forward=None):
    """The literal transposed chain in float64 on rows x [M, 90 or 63] with d raw = draw [M, C].
    Returns dict(raw [M, C], dxe [M, 63], dW, db: layer name -> array, dy: layer name -> [M, N] for the names in keep_dy).
    mutant: one of MUTANTS, a wrong chain.  trace: a list that receives one (label, B3 figure) per GEMM of the backward.
    forward: `exact_field.chain(net, x, keep=True)` where the caller has it already."""
    assert mutant is None or mutant in MUTANTS
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(draw, dtype=np.float64)
    M, D, W, skips = x.shape[0], net["D"], net["W"], net["skips"]
    raw, seen = E.chain(net, x, keep=True) if forward is None else forward
    assert g.shape == raw.shape
    w = dict(zip(net["names"], net["weights"]))
    dW, db, dys = {}, {}, {}

    def wgrad(name, dy):
        xin, pre = seen[name]
        if name in keep_dy:
            dys[name] = dy
        if mutant == "dw_from_output" and pre.shape[1] == xin.shape[1]:
            xin = np.maximum(pre, 0.0) if (name.startswith("pts") or name == "views") else pre
        dyw = dy
        if mutant == "dw_last_slice_missing" and M % SLICE:
            dyw, xin = dy[:M // SLICE * SLICE], xin[:M // SLICE * SLICE]
        dW[name] = _product([(dyw.T, xin)], f"dW {name}", trace)
        dyb = dy[:-1] if mutant == "db_last_row_missing" else dy
        db[name] = _product([(dyb.T, np.ones((dyb.shape[0], 1)))], f"db {name}", trace)[:, 0]

    def mask(j):                                   # relu' of trunk layer j
        if mutant == "last_mask_skipped" and j == D - 1:
            return 1.0
        k = min(max(j + MASK_OFFSETS.get(mutant, 0), 0), D - 1)
        return seen[f"pts{k}"][1] > 0

    if net["use_viewdirs"]:
        g_rgb, g_sigma = g[:, :3], g[:, 3:4]
        if mutant == "draw_contiguous_blocks":
            g_rgb, g_sigma = g.reshape(-1)[:3 * M].reshape(M, 3), g.reshape(-1)[3 * M:].reshape(M, 1)
        wgrad("rgb", g_rgb)
        d_hv = _product([(g_rgb, w["rgb"])], "dx rgb", trace) * (seen["views"][1] > 0)
        wgrad("views", d_hv)
        wv = w["views"][:, -W:] if mutant == "view_last_columns" else w["views"][:, :W]
        d_feat = _product([(d_hv, wv)], "dx views", trace)
        wgrad("feature", d_feat)
        wgrad("alpha", g_sigma)
        if mutant == "sigma_not_accumulated":
            d_h = (d_feat @ w["feature"]) * mask(D - 1)
        elif mutant == "sigma_after_mask":
            d_h = (d_feat @ w["feature"]) * mask(D - 1) + g_sigma @ w["alpha"]
        else:
            d_h = _product([(d_feat, w["feature"]), (g_sigma, w["alpha"])], "dx feature + alpha", trace) * mask(D - 1)
    else:
        if mutant == "output_ch_4":
            g4 = np.zeros_like(g)
            g4[:, :4] = g.reshape(-1)[:4 * M].reshape(M, 4)
            g = g4
        wgrad("output", g)
        d_h = _product([(g, w["output"])], "dx output", trace) * mask(D - 1)

    to_xe = []                                     # the products that are summed into d xe
    for i in range(D - 1, -1, -1):                 # d_h: the gradient of layer i's pre-activation
        name = f"pts{i}"
        wgrad(name, d_h)
        wi = w[name]
        if i == 0:
            to_xe.append((d_h, wi))
        elif (i - 1) in skips:                     # layer i read cat[xe, h_{i-1}]
            emb, hid = wi[:, :E.IN_PTS], wi[:, E.IN_PTS:]
            if mutant == "skip_split_62":
                emb = np.concatenate([wi[:, :62], np.zeros((W, 1))], axis=1)
                hid = wi[:, 62:62 + W]
            elif mutant == "skip_split_64":
                hid = np.concatenate([wi[:, 64:], np.zeros((W, 1))], axis=1)
            if mutant != "skip_embedding_dropped":
                to_xe.append((d_h, emb))
            d_h = _product([(d_h, hid)], f"dx {name}", trace) * mask(i - 1)
        else:
            d_h = _product([(d_h, wi)], f"dx {name}", trace) * mask(i - 1)
    dxe = _product(to_xe, "dx xe", trace)
    return dict(raw=raw, dxe=dxe, dW=dW, db=db, dy=dys)


def compared(res, public=None):
    """What the GPU test compares exactly, as one dict name -> float64 array.  public: the "identity" network of a case of the
    public path, which returns d pts = the identity columns of d xe and is exact in `exact_columns` of every dW only."""
    out = {"raw": res["raw"], "d xe": res["dxe"] if public is None else res["dxe"][:, :3]}
    for name, a in res["dW"].items():
        out[f"dW {name}"] = a if public is None else a[:, exact_columns(public, name)]
        out[f"db {name}"] = res["db"][name]
    return out


def rejected(ref, other, public=None):
    """True where the comparison of the GPU test -- equality of every compared fp32 value -- tells `other` from `ref`."""
    a, b = compared(ref, public), compared(other, public)
    return any(a[k].shape != b[k].shape or (a[k].astype(np.float32) != b[k].astype(np.float32)).any() for k in a)


# ---- d raw ------------------------------------------------------------------------------------------------------------------
def make_draw(net, M, seed, density=1.0, wide=False, one_channel=False):
    """An integer d raw [M, C] from {-1, 0, 1} ({-2 .. 2} with wide).  A share `density` of the rows is nonzero, and one row of
    every block of 16 holds no zero (in the last block the last row), so every channel is nonzero on some row; no channel sums to
    zero (alpha_linear's db is that sum).  density 0 leaves those rows alone.  one_channel, the thinnest draw: the one nonzero
    row of a block holds one nonzero entry, the channels taking turns."""
    rng = np.random.default_rng([seed, M, 77])
    C = net["output_ch"]
    top = 2 if wide else 1
    g = rng.integers(-top, top + 1, size=(M, C)).astype(np.float64)
    g[rng.random(M) >= (0.0 if one_channel else density)] = 0.0
    full = rng.choice(np.array([v for v in range(-top, top + 1) if v != 0], dtype=np.float64), size=(M, C))
    for k, lo in enumerate(range(0, M, 16)):
        r = lo + int(rng.integers(0, min(16, M - lo)))
        if lo + 16 >= M:
            r = M - 1                              # the last row carries a gradient: a sum that stops short of it is wrong
        if one_channel:
            g[r, k % C] = full[r, k % C]
        else:
            g[r] = full[r]
    for c in range(C):
        if g[:, c].sum() == 0:
            r = int(np.flatnonzero(g[:, c])[0])
            g[r, c] = -g[r, c]
    assert (g.sum(axis=0) != 0).all()
    return g


# ---- the conditions ---------------------------------------------------------------------------------------------------------
def check_b1(net, x, draw, forward=None):
    """d raw, every Linear's input on the rows x, and every weight: fp32 numbers with at most 8 significant bits."""
    assert E.fits16(draw).all() and (draw == np.rint(draw)).all(), "B1: d raw"
    _, seen = E.chain(net, x, keep=True) if forward is None else forward
    for name, wt in zip(net["names"], net["weights"]):
        assert E.fits16(wt).all(), f"B1: a weight of {name}"
        assert E.fits16(seen[name][0]).all(), f"B1: an input of {name} has more than 8 significant bits"


def check_b2(net, x, forward=None):
    """Every ReLU layer's pre-activation on the rows x is a multiple of the quantum of its terms: none lies in (0, q)."""
    _, seen = E.chain(net, x, keep=True) if forward is None else forward
    for name, wt, b in zip(net["names"], net["weights"], net["biases"]):
        if not (name.startswith("pts") or name == "views"):
            continue
        inp, pre = seen[name]
        q = min(E.quantum(wt) * E.quantum(inp), E.quantum(b))
        assert np.isfinite(q) and (pre / q == np.rint(pre / q)).all(), f"B2: {name}: a pre-activation is no multiple of {q}"
        assert not ((pre > 0) & (pre < q)).any(), f"B2: {name}: a pre-activation in (0, {q})"
        assert E.is_f32(pre), f"B2: {name}: a pre-activation is no fp32 number"


def check_b3(net, x, draw, forward=None):
    """(sum_k |a b|) / q < 2^24 for every GEMM of the backward.  Returns (the worst figure, its GEMM's label)."""
    trace = []
    res = backward64(net, x, draw, trace=trace, forward=forward)
    assert {t[0] for t in trace} >= {f"dW {n}" for n in net["names"]} | {f"db {n}" for n in net["names"]} | {"dx xe"}
    label, worst = max(trace, key=lambda t: t[1])
    assert worst < LIMIT, f"B3: {label}: sum of magnitudes / quantum = 2^{np.log2(worst):.2f}"
    for k, a in compared(res).items():
        assert E.is_f32(a), f"B3: {k} is no fp32 number"
    return worst, label


def check_b4(net, x, draw, ref=None, forward=None):
    """Every gradient tensor is visible in every 16-row block, and every applicable mutant is rejected."""
    M = x.shape[0]
    ref = backward64(net, x, draw, forward=forward) if ref is None else ref
    assert ref["dxe"].any(), "B4: d xe is zero"
    for name in net["names"]:
        dw, b = ref["dW"][name], ref["db"][name]
        assert dw.any() and b.any(), f"B4: a gradient of {name} is zero"
        if M >= BLOCK_ROWS:
            for lo in range(0, dw.shape[0], 16):
                assert dw[lo:lo + 16].any(), f"B4: rows {lo}.. of dW {name} are zero"
                assert b[lo:lo + 16].any(), f"B4: entries {lo}.. of db {name} are zero"
    public = net if net["columns"] == "identity" else None
    for mutant in MUTANTS:
        if applies(mutant, net, M):
            other = backward64(net, x, draw, mutant=mutant, forward=forward)
            assert rejected(ref, other, public), f"B4: the comparison does not see {mutant}"


# ---- the table both test files walk ------------------------------------------------------------------------------------------
_cases = {}


def _draw_for(name, columns, M, net):
    key = (name, columns, M)
    return make_draw(net, M, seed=E.NETWORKS[name]["seed"], wide=M == WIDE_M and columns == "all", **THIN.get(key, {}))


def chain_case(name, M):
    """dict(net, x [M, 90 or 63], draw [M, C], ref = backward64) of an "all" network on M pool rows, cached."""
    key = (name, "all", M)
    if key not in _cases:
        net = E.network(name, "all")
        x = net["pool"][E.row_indices(M, seed=M)]
        draw = _draw_for(name, "all", M, net)
        _cases[key] = dict(net=net, x=x, draw=draw, ref=backward64(net, x, draw))
    return _cases[key]


def trig_layers(net):
    """The layers whose input holds sines and cosines: name -> (first column, end, which input: "pts" or "views")."""
    out = {"pts0": (3, E.IN_PTS, "pts")}
    for s in net["skips"]:
        out[f"pts{s + 1}"] = (3, E.IN_PTS, "pts")
    if net["use_viewdirs"]:
        out["views"] = (net["W"] + 3, net["W"] + E.IN_VIEWS, "views")
    return out


def ray_case(name, R, N):
    """An "identity" network on R rays of N samples, cached: dict(net, ray [R], rows [R, N], pts [R, N, 3], viewdirs [R, 3] or
    None, x (the pool rows with the sine and cosine columns set to zero), draw [R N, C], ref = backward64 on x, trig: layer name ->
    (first column, end, float64 dW of those columns on float64 sines and cosines, its bound))."""
    key = (name, "identity", (R, N))
    if key not in _cases:
        net = E.network(name, "identity")
        ray, rows = E.ray_indices(R, N, seed=R)
        x = net["pool"][rows.reshape(-1)].copy()
        x[:, 3:E.IN_PTS] = 0.0
        x[:, E.IN_PTS + 3:] = 0.0
        M = R * N
        draw = _draw_for(name, "identity", M, net)
        layers = trig_layers(net)
        ref = backward64(net, x, draw, keep_dy=tuple(layers))
        pts = x[:, :3]
        views = x[:, E.IN_PTS:E.IN_PTS + 3]
        enc = {"pts": T.posenc64(pts.astype(np.float32), 10)[:, 3:]}
        if net["use_viewdirs"]:
            enc["views"] = T.posenc64(views.astype(np.float32), 4)[:, 3:]
        trig = {}
        for lname, (lo, hi, which) in layers.items():
            dy = ref["dy"][lname]
            mag = np.abs(dy).T @ np.abs(enc[which])
            bound = M * T.U * mag + T.TRIG * np.abs(dy).sum(axis=0)[:, None]
            trig[lname] = (lo, hi, dy.T @ enc[which], bound)
        ref["dy"] = {}
        _cases[key] = dict(net=net, ray=ray, rows=rows, pts=pts.reshape(R, N, 3),
                           viewdirs=net["rays"]["viewdirs"][ray] if net["use_viewdirs"] else None, x=x, draw=draw, ref=ref,
                           trig=trig)
    return _cases[key]


def exact_columns(net, name):
    """The columns of dW `name` that the public path must return exactly: all but the sine and cosine columns."""
    K = dict(zip(net["names"], net["weights"]))[name].shape[1]
    keep = np.ones(K, dtype=bool)
    if name in trig_layers(net):
        lo, hi, _ = trig_layers(net)[name]
        keep[lo:hi] = False
    return keep


def first_difference(got, want, what):
    """'' if the fp32 tensors are equal as values, else the tensor's name, the first differing (row, column) and both values."""
    if got.shape != want.shape:
        return f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    g2 = got.reshape(-1, got.shape[-1]) if got.dim() > 1 else got.reshape(-1, 1)
    w2 = want.reshape(-1, want.shape[-1]) if want.dim() > 1 else want.reshape(-1, 1)
    diff = E.first_difference(g2, w2)
    return f"{what}: {diff}" if diff else ""
