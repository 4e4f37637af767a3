"""The DepthNet's training pass (autograd.DepthNetFunction) on the exactly representable networks of tests/exact_depthnet.py:
z and every weight and bias gradient against the float64 transposed chain, entry by entry, each under a derived bound.

Shared by tests/test_exact_depthnet_backward_host.py (the conditions below, torch autograd in float64 and in fp32, and the
mutants, on the CPU) and tests/test_gpu_exact_depthnet_backward.py (DepthNet.forward under autograd and z.backward on the HIP
GEMMs).  Nothing here calls the library.

The pass is the literal, un-folded chain (depth_net.py:117-169): three affine branches on cat[h, e] (layer 0 on cat[e, e]), the
LeakyReLU trunk on cat[h_o, h_d, h_x, e_o, e_d, e_x], a sigmoid head and z = near (1 - s) + far s.  On the networks and rays of
exact_depthnet every forward sum is exact in fp32 (D1 - D4, D3 for the literal chain), every sine and cosine column has weight
zero, no ordinary unit is negative and a chain unit is one exact product: every saved activation and every mask is the float64
one.  What is left to round is the sigmoid, and the sums of the backward; `reference64` carries both as a running pair
(value, error) down the transposed chain.

The cases (`cases(name)`; the table both test files walk).  TRAIN_NETWORKS: "prod" ([256] x 10, exact_depthnet's own: branch K
of 319 and 382, the 64-k trips), "w256n2" (the same widths two layers deep: see LOOSE below), "w128n2", "w40n3" (widths that
are no multiple of 32: K = 103, 166, 372, N = 40 tails in every GEMM) and "w24n1" (n = 1: no `bufs` layer, the branches write
straight into y0), seed 31.  Rays are pool rows through
exact_depthnet.ray_indices; dz holds integers from {-2 .. 2}, some of them zero, the last row's never: dz (far - near) is exact.
    main head   every row count of ROWS (1, 31, 32, 33, 127, 128, 129, 1024, 1025, 1300; on "prod" 1, 33, 1024, 1300) at radius 3,
                the (near, far) pairs of exact_depthnet.NEAR_FAR in turn; radius 2 (its 36 rays, repeated) at 33 and 129 rows
                ("prod": 33) under both pairs.
    chain heads every "chain<c>" and "chain<c>s" at one small row count (1, 31, 32, 33 in turn; "prod": 33) on rays on which
                the chain is not zero and the head's sum is within UNSATURATED = 8 (s (1 - s) >= 3.3e-4: a saturated ray carries
                the sigmoid's error and no gradient), and at one row count from 127 on (in turn; every fourth at radius 2); on
                "prod" two heads only take a large count (1024 and 1300).  The last ray of a chain head's case is the chosen one
                whose sum is nearest zero, so that "the last ray" of the mutants is one with a gradient.  Under the main head no gradient reaches a chain unit, so these heads
                are what runs the 0.01 branch of `dact`, in the sub-block of every trunk layer that chain c passes through.
                Under a chain head the three branches' gradients are identically zero (a sign unit reads the direct columns
                alone): the bound there is 0, and the comparison asks for zeros (-0.0 passes).

The bound.  U = 2^-24, gamma(k) = k U / (1 - k U).
    z       exact_depthnet.gate(near, far) as it stands: the head's sum is exact.
    g       the head's gradient g = dz (far - near) s (1 - s) is formed as g0 = dz (far - near) (exact), then y (1 - y) and the
            product: three roundings, 3 U s (1 - s) |g0| (k roundings of relative size U / (1 + U) stay below k U for k <= 3).  s
            itself is off by gemm_tile_reference.sigmoid_bound(v), which moves s (1 - s) by |1 - 2 s| of it:
                E_g = |g0| (|1 - 2 s| sigmoid_bound + 3 U s (1 - s)).
    product C = A B^T of length K, A off by at most E_A elementwise, B exact:
                E_C = E_A |B|^T + gamma(K + 1) (|A| + E_A) |B|^T,
            the order-independent bound of an fp32 sum (tests/test_gpu_wgrad.py): any tree over K products has at most K - 1
            additions on a path, and each product rounds once.  The grad-input products (K = the width, or 1 under the head),
            every dW = dy^T x (K = the rays) and every db (B = 1) use it.
    dact    one multiply by 1 or fl32(0.01): E' = slope (E + U (|c| + E)).
    sines and cosines: the embeddings' identity columns are the pool's integers, exact; a sine or cosine column is off by
            train_kernels_reference.TRIG = 4 U, so a dW column that multiplies one adds TRIG sum_m (|dy| + E_dy).
    Weights, identity columns and saved activations carry no error (D1 - D3).  The activation derivative is read from the
    activation's OUTPUT, as the epilogue does: y > 0 ? 1 : fl32(0.01); an ordinary unit that is exactly 0 on a ray takes 0.01.

The conditions, asserted on the CPU for every case:
    V1  no trunk pre-activation on the chosen rays lies within its layer's quantum of zero on the wrong side: an ordinary unit is
        0 or at least one quantum of its terms, an fp32 number that the activation hands on unchanged; a chain unit is an fp32
        number and its activation is the f32 rule's.  No mask can differ between fp32 and float64.
    V2  for every trunk layer and every chain (one per 16-row sub-block), under one of the chain's two heads on some case, an
        entry moves by more than two bounds when that layer's negative-branch slope is 1, and when it is 0.
    V3  under the main head no gradient tensor is identically zero; from 257 rays on every 16-row block of every dW and db
        holds an entry above two bounds.
    Every mutant of MUTANTS, another computation `reference64` can be switched to, moves some compared entry by more than two
    bounds on every case on which it differs from the chain at all; `must_apply` lists where it has to differ.

LOOSE: where the bound cannot be sharp.  An ordinary row of exact_depthnet's trunk is eight +-1/2, +-1 coefficients and a
correction of up to 16 on twelve basis units, drawn so that the unit hits its target: through the transposed chain the values
cancel and the sums of magnitudes do not.  An order-independent bound has to follow the magnitudes, so max |ref| / bound falls
by a factor of three to eight per layer on the way down: on "prod", ten trunk and ten branch layers deep, the main head's
gradients are 75 to 3000 bounds large from the head down to cat_layers.10, about one bound at cat_layers.4, a tenth at
cat_layers.0 and 1e-4 to 1e-5 at the branches' first layers (values near 1e10 under bounds near 1e14).  There the comparison
still holds z, the upper trunk, every chain head's trunk gradients (one nonzero column per layer: nothing cancels), the exact
zeros and NaN, but it cannot see a branch gradient that is lost: V3's second half and the two mutants that only zero a part of
a branch dW (LOOSE_MUTANTS) are not asked of "prod"; the host test prints how often they go unseen (11 times: on the main head's six
cases, one of them but for a single ray).  Every other mutant is rejected on "prod" too.  "w256n2" is there for what "prod" was to reach and so
cannot: the same 256-wide GEMMs (branch K of 319 and 382, grad-input K = 256: the 64-k trips) at a depth of two, where every
16-row block of every tensor holds an entry above 22 bounds and every condition and mutant is asserted.

Departures from the issue that asked for this file.
    * "prod" is LOOSE (above) and "w256n2" was added; the small chain cases take unsaturated rays and put the least saturated
      one last (the table above): with the last ray saturated, "db without the last ray" moved nothing by two bounds.
    * The float64 comparison with torch autograd runs oracle.nerf_oracle.depthnet_forward with torch.nn.functional.leaky_relu
      replaced by the f32 rule as an autograd function (v > 0 ? v : fl32(fl32(0.01) v), derivative from the output with
      fl32(0.01)): torch's own float64 leaky_relu multiplies by the double 0.01, 2e-8 off in relative terms, and leaves the
      product unrounded, which 1e-12 of the magnitudes sees under every chain head and at every ordinary unit that is 0.  The
      fp32 stand-in is the oracle untouched.
    * The TRIG term and gamma's factor are taken on |dy| + E_dy, not |dy|: the rigorous form; the difference is of order U^2.
    * Chain heads do not run at every row count, nor every (radius, near, far) at every row count: the table above is what a
      few seconds per test hold; every row count runs under the main head, every chain head at a small and a large count.
    * "slope from the layer's input sign with >= at zero" and the two `dact_ref` mutants are the chain itself where no unit with
      a gradient is exactly 0 (one ray, say): they are asked to be rejected wherever they differ at all.

Measured, worst |err| / bound per network (z's gate included): the fp32 oracle on the CPU (torch autograd) / the HIP pass on an
MI355X, over all cases; and how sharp the bound is: max |ref| / bound per 16-row block of a tensor, the least and the largest
block over the tensors of the main head's cases from 257 rays on, as the host test prints them.

    network    fp32 oracle, CPU       HIP pass, MI355X       least / largest block of max |ref| / bound
               z      gradients       z      gradients       all tensors           trunk and head alone (least)
    prod       0.234  0.106           0.234  0.106           1.14e-5 / 3.0e3       0.0118
    w256n2     0.249  0.271           0.249  0.271           22.2 / 3.1e3          38.4
    w128n2     0.249  0.184           0.249  0.184           46.1 / 3.0e3          62.6
    w40n3      0.238  0.289           0.238  0.289           54.4 / 2.8e3          110
    w24n1      0.234  0.171           0.234  0.171           69.9 / 3.7e3          69.9

The two columns agree to the digits shown: the worst entries are products of one or a few terms (one ray, or a chain's single
column), whose only error is the sigmoid's, and the device's expf and the host's round s alike there.  No entry needed a wider
bound than derived, on either side.
"""

import numpy as np
import torch

import exact_depthnet as X
import exact_field as E
import gemm_tile_reference as G
import train_kernels_reference as T

U = X.U
SLOPE32 = X.SLOPE32
SEED = 31
ROWS = (1, 31, 32, 33, 127, 128, 129, 1024, 1025, 1300)
PROD_ROWS = (1, 33, 1024, 1300)
SMALL_ROWS = (1, 31, 32, 33)
LARGE_ROWS = (127, 128, 129, 1024, 1025, 1300)
UNSATURATED = 8.0                  # |v| of a chain head's few rays: s (1 - s) >= 3.3e-4
BLOCK_ROWS = 257                   # from this row count on, V3 asks for an entry above two bounds in every 16-row block
TRAIN_NETWORKS = {X.PROD: None, "w256n2": (256, 2), "w128n2": (128, 2), "w40n3": (40, 3), "w24n1": (24, 1)}      # None: exact_depthnet.network
LOOSE = (X.PROD,)                  # where the bound outgrows the gradient down the chain: see the module docstring
LOOSE_MUTANTS = ("layer0_second_half_missing", "branch_e_columns_missing")

MUTANTS = ("branches_exchanged", "dact_from_above", "dact_from_below", "slope_from_input_ge", "scale_dropped",
           "sigmoid_derivative_dropped", "layer0_second_half_missing", "trunk_window_plus_1", "trunk_window_minus_1",
           "dh_rotated", "branch_e_columns_missing", "db_last_ray_missing", "dw_last_32_rays_missing", "branch_slot_below")
BRANCH_MUTANTS = ("branches_exchanged", "layer0_second_half_missing", "trunk_window_plus_1", "trunk_window_minus_1", "dh_rotated",
                  "branch_e_columns_missing", "branch_slot_below")

_nets = {}


def network(name):
    if name not in _nets:
        if TRAIN_NETWORKS[name] is None:
            _nets[name] = X.network(name)
        else:
            width, n = TRAIN_NETWORKS[name]
            _nets[name] = X.make_exact_depthnet([width] * n, [width] * n, SEED)
        assert len(set(_nets[name]["hidden"]) | set(_nets[name]["cat"])) == 1 and len(_nets[name]["hidden"]) == len(_nets[name]["cat"])
    return _nets[name]


def gamma(k):
    return k * U / (1 - k * U)


def param_names(net):
    """The parameters in autograd.depthnet_params' order: [weight, bias] of the origin, direction and intersection branches, the
    trunk, the head."""
    n = len(net["cat"])
    mods = ([f"origin_layers.{i}" for i in range(n)] + [f"direction_layers.{i}" for i in range(n)]
            + [f"intersection_layers.{i}" for i in range(n)] + [f"cat_layers.{2 * i}" for i in range(n)] + ["to_depth.0"])
    return [m + s for m in mods for s in (".weight", ".bias")]


# ---- the forward, as saved for the backward ---------------------------------------------------------------------------------
_pool_trunk = {}


def pool_head_sum(net, head):
    """[P]: a head's sum on every pool ray."""
    if id(net) not in _pool_trunk:
        _pool_trunk[id(net)] = X.trunk(net, "f32", X.pool()["x12"])
    return X.head_sum(net, head, _pool_trunk[id(net)])


def forward64(net, rays):
    """What DepthNetFunction saves, in float64, on the pool rows `rays`: dict(emb: the three embeddings with float64 sines and
    cosines, x_in[b][i]: branch b layer i's input cat[h, e], y0: the trunk's input, seen: exact_depthnet.trunk's (input, pre,
    output) per trunk layer, trig_in[b][i] / trig_y0: which columns of those inputs hold sines and cosines)."""
    P = X.pool()
    x12 = P["x12"][rays]
    n, width = len(net["cat"]), net["cat"][0]
    emb = [T.posenc64(P["o"][rays], 10), T.posenc64(P["d"][rays], 10), T.posenc64(P["x"][rays], 10)]
    ident = X.embed_identity(x12)
    x_in, trig_in, hs, at = [], [], [], 0
    for b in range(3):
        dim = X.BRANCH_DIM[b]
        e, eid = emb[b], ident[:, at:at + dim]
        assert (e[:, X.BRANCH_ID[b]] == eid[:, X.BRANCH_ID[b]]).all()
        tr = np.ones(dim, dtype=bool)
        tr[X.BRANCH_ID[b]] = False
        h, hid, ins, trs = e, eid, [], []
        for i, (w, bias) in enumerate(zip(net["branch_w"][b], net["branch_b"][b])):
            ins.append(np.concatenate([h, e], axis=1))
            trs.append(np.concatenate([tr if i == 0 else np.zeros(h.shape[1], dtype=bool), tr]))
            h = hid = np.concatenate([hid, eid], axis=1) @ w.T + bias          # the sines and cosines carry zero weights (D2)
        x_in.append(ins)
        trig_in.append(trs)
        hs.append(h)
        at += dim
    y0 = np.concatenate(hs + emb, axis=1)
    trig_y0 = np.ones(y0.shape[1], dtype=bool)
    trig_y0[:3 * width] = False
    trig_y0[3 * width + X.ID_COLS] = False
    last, seen = X.trunk(net, "f32", x12, keep=True)
    pre0 = X.literal_pre0(net, x12)
    assert (pre0 == seen[0][1]).all() and (np.concatenate(hs + [ident], axis=1) @ net["cat_w"][0].T + net["cat_b"][0] == pre0).all()
    return dict(emb=emb, x_in=x_in, trig_in=trig_in, y0=y0, trig_y0=trig_y0, seen=seen, last=last, n=n, width=width)


# ---- the transposed chain ---------------------------------------------------------------------------------------------------
def reference64(net, head, rays, dz, near, far, radius, mutant=None, slope=None, bounds=True, forward=None):
    """The literal transposed chain in float64 on the pool rows `rays` with the upstream gradient dz [M, 1].
    Returns dict(z [M, 1], z_bound, grads: name -> (value, elementwise bound) in autograd.depthnet_params' order, mags: name ->
    each entry's sum of magnitudes, carried down the chain like the error, zero_hit: whether a unit that is exactly 0 met a
    nonzero gradient).  mutant: one of MUTANTS, another computation; slope = (layer, value): that trunk layer's negative-branch slope replaced; bounds=False: values only (the bounds are None)."""
    assert mutant is None or mutant in MUTANTS
    rays = np.asarray(rays)
    assert (X.pool()["radius"][rays] == radius).all()
    f = forward64(net, rays) if forward is None else forward
    n, width, seen = f["n"], f["width"], f["seen"]
    M = len(rays)
    dz = np.asarray(dz, dtype=np.float64).reshape(M, 1)
    names = param_names(net)
    vals, errs, mags = {}, {}, {}
    hit = [False]

    # a running quantity is (value, Q); Q = (error, sum of magnitudes), or None without bounds
    def prod(A, Q, B):                                 # C = A B (B exact, the sum over A's columns)
        C = A @ B
        if Q is None:
            return C, None
        EA, MA = Q
        aB = np.abs(B)
        return C, ((EA + gamma(A.shape[1] + 1) * (np.abs(A) + EA)) @ aB, MA @ aB)

    def wgrad(slot, dy, Q, x, trig):
        dyw, xw = dy, x
        if mutant == "dw_last_32_rays_missing":
            dyw, xw = dy[:max(M - 32, 0)], x[:max(M - 32, 0)]
        dW = dyw.T @ xw
        dyb = dy[:-1] if mutant == "db_last_ray_missing" else dy
        db = dyb.sum(axis=0)
        EW = Eb = None
        if Q is not None:
            Edy, Mdy = Q
            S, ax = np.abs(dy) + Edy, np.abs(x)
            EW = (Edy + gamma(M + 1) * S).T @ ax
            if trig is not None:
                EW[:, trig] += T.TRIG * S.sum(axis=0)[:, None]
            Eb = Edy.sum(axis=0) + gamma(M + 1) * S.sum(axis=0)
            mags[names[2 * slot]], mags[names[2 * slot + 1]] = Mdy.T @ ax, Mdy.sum(axis=0)
        vals[names[2 * slot]], errs[names[2 * slot]] = dW, EW
        vals[names[2 * slot + 1]], errs[names[2 * slot + 1]] = db, Eb

    def dact(j, c, Q):                                 # times leaky'(output of trunk layer j)
        k = min(max(j + {"dact_from_above": 1, "dact_from_below": -1}.get(mutant, 0), 0), n - 1)
        out = seen[k][2]
        low = slope[1] if slope is not None and slope[0] == j else SLOPE32
        der = np.where(out > 0, 1.0, low)
        if mutant == "slope_from_input_ge":
            der = np.where(seen[j][1] >= 0, 1.0, low)
        hit[0] = hit[0] or bool(((seen[j][2] == 0) & (c != 0)).any())
        return c * der, None if Q is None else (der * (Q[0] + U * (np.abs(c) + Q[0])), der * Q[1])

    hw, _ = net["heads"][head]
    v = X.head_sum(net, head, f["last"]).reshape(M, 1)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-v))
    z = X.depth(v, near, far)
    g0 = dz * (1.0 if mutant == "scale_dropped" else far - near)
    sp = 1.0 if mutant == "sigmoid_derivative_dropped" else s * (1.0 - s)
    g = g0 * sp
    Q = None
    if bounds:
        sb = G.sigmoid_bound(torch.from_numpy(v)).numpy()
        Q = (np.abs(g0) * (np.abs(1.0 - 2.0 * s) * sb + 3 * U * s * (1.0 - s)), np.abs(g))
    wgrad(4 * n, g, Q, f["last"], None)
    d_y, Q = dact(n - 1, *prod(g, Q, hw))
    for i in range(n - 1, -1, -1):
        wgrad(3 * n + i, d_y, Q, f["y0"] if i == 0 else seen[i - 1][2], f["trig_y0"] if i == 0 else None)
        if i > 0:
            d_y, Q = dact(i - 1, *prod(d_y, Q, net["cat_w"][i]))
    full, Qfull = prod(d_y, Q, net["cat_w"][0])        # below trunk layer 0 the three branch outputs alone need a gradient
    off = {"trunk_window_plus_1": 1, "trunk_window_minus_1": -1}.get(mutant, 0)

    def window(a, k):                                  # branch k's columns of the grad-input product
        if off < 0:
            a = np.concatenate([np.zeros((M, 1)), a[:, :3 * width - 1]], axis=1)
        else:
            a = a[:, off:3 * width + off]
        return a[:, k * width:(k + 1) * width]

    for b in range(3):
        k = (b + 1) % 3 if mutant == "dh_rotated" else b
        d_h, Q = window(full, k), None if Qfull is None else (window(Qfull[0], k), window(Qfull[1], k))
        for i in range(n - 1, -1, -1):
            wgrad(b * n + i, d_h, Q, f["x_in"][b][i], f["trig_in"][b][i])
            name = names[2 * (b * n + i)]
            if mutant == "layer0_second_half_missing" and i == 0:
                vals[name] = np.concatenate([vals[name][:, :X.BRANCH_DIM[b]], np.zeros((width, X.BRANCH_DIM[b]))], axis=1)
            if mutant == "branch_e_columns_missing" and i >= 1:
                vals[name] = np.concatenate([vals[name][:, :width], np.zeros((width, X.BRANCH_DIM[b]))], axis=1)
            if i > 0:
                d_h, Q = prod(d_h, Q, net["branch_w"][b][i][:, :width])
    if mutant == "branches_exchanged":
        for i in range(2 * n):
            a, b2 = names[i], names[2 * n + i]
            vals[a], vals[b2] = vals[b2], vals[a]
    if mutant == "branch_slot_below":                  # layer i's gradient lands in layer i - 1's slot, the last slot keeps its own
        old = dict(vals)
        for b in range(3):
            for i in range(1, n):
                for t in (0, 1):
                    src, dst = names[2 * (b * n + i) + t], names[2 * (b * n + i - 1) + t]
                    if old[src].shape == old[dst].shape:
                        vals[dst] = old[src]
    return dict(z=z, z_bound=X.gate(near, far), grads={k: (vals[k], errs[k]) for k in names}, mags=mags, zero_hit=hit[0])


def rejected(ref, other):
    """True where the GPU test's comparison -- z within the gate, every gradient entry within its bound -- tells `other` from
    `ref` with a bound to spare: some entry differs by more than two bounds."""
    if (np.abs(other["z"] - ref["z"]) > 2 * ref["z_bound"]).any():
        return True
    return any((np.abs(other["grads"][k][0] - v) > 2 * bnd).any() for k, (v, bnd) in ref["grads"].items())


def differs(ref, other):
    return bool((other["z"] != ref["z"]).any()) or any((other["grads"][k][0] != v).any() for k, (v, _) in ref["grads"].items())


def must_apply(mutant, c):
    """Where a mutant has to be another computation than the chain (elsewhere it may be, and is rejected if it is)."""
    n, main = len(c["net"]["cat"]), c["head"] == "main"
    if c["name"] in LOOSE and mutant in LOOSE_MUTANTS:
        return False
    if mutant in ("sigmoid_derivative_dropped", "db_last_ray_missing", "dw_last_32_rays_missing"):
        return True
    if mutant == "scale_dropped":
        return c["far"] - c["near"] != 1
    if mutant in ("branch_e_columns_missing", "branch_slot_below"):
        return main and n >= 2
    if mutant in BRANCH_MUTANTS:
        return main
    if mutant in ("dact_from_above", "dact_from_below"):
        return n >= 2 and not main and c["R"] >= 31       # a chain's sign alternates from layer to layer
    return False                                          # slope_from_input_ge: where a unit with a gradient is exactly 0


def compare(got_z, got_grads, ref):
    """(verdicts: name -> train_kernels_reference.Verdict, worst ratio) of a pass's z [M, 1] and gradients (name -> array)
    against `reference64`'s result.  A bound of 0 asks for the value itself (-0.0 passes); NaN is rejected everywhere."""
    out = {"z": T.compare_bound(got_z, ref["z"], ref["z_bound"])}
    for k, (v, bnd) in ref["grads"].items():
        got = np.asarray(got_grads[k])
        assert got.shape == v.shape, (k, got.shape, v.shape)
        out[k] = T.compare_bound(got, v, bnd)
    return out, max(v.worst for v in out.values())


def failures(verdicts, ref):
    """'' or one line per tensor with rejected entries: how many, and the first's index, value, reference and bound."""
    lines = []
    for k, v in verdicts.items():
        if v.rejected.size:
            want, bnd = (ref["z"], np.full(ref["z"].shape, ref["z_bound"])) if k == "z" else ref["grads"][k]
            at = np.unravel_index(int(v.rejected[0]), want.shape)
            lines.append(f"{k}: {v.rejected.size} of {want.size} entries outside the bound, first at {tuple(int(a) for a in at)}: "
                         f"expected {want[at]!r} +- {np.broadcast_to(bnd, want.shape)[at]!r}")
    return "; ".join(lines)


# ---- the upstream gradient and the table of cases ---------------------------------------------------------------------------
def make_dz(R, seed):
    """Integers from {-2 .. 2} [R, 1]; the last row's is not zero, and from three rows on some entry is."""
    rng = np.random.default_rng([seed, R, 55])
    dz = rng.integers(-2, 3, size=(R, 1)).astype(np.float64)
    if R >= 3:
        dz[R // 2] = 0.0
    if dz[-1, 0] == 0:
        dz[-1, 0] = float(rng.choice([-2.0, -1.0, 1.0, 2.0]))
    return dz


def cases(name):
    """[(head, R, radius, near, far, seed)]: the table of the module docstring."""
    net = network(name)
    prod = name == X.PROD
    rows = PROD_ROWS if prod else ROWS
    out = []
    for k, R in enumerate(rows):
        out.append(("main", R, 3.0) + X.NEAR_FAR[k % 2] + (R,))
    for R in ((33,) if prod else (33, 129)):
        for near, far in X.NEAR_FAR:
            out.append(("main", R, 2.0, near, far, R + 1))
    chain_heads = [h for h in net["heads"] if h != "main"]
    for k, head in enumerate(chain_heads):
        near, far = X.NEAR_FAR[(k // 2) % 2]
        out.append((head, 33 if prod else SMALL_ROWS[k % 4], 3.0, near, far, 100 + k))
        if prod:
            if k in (0, 17):
                out.append((head, 1024 if k == 0 else 1300, 3.0, near, far, 200 + k))
        else:
            out.append((head, LARGE_ROWS[k % 6], 2.0 if k % 4 == 1 else 3.0, near, far, 200 + k))
    return out


_cases = {}


def case(name, key):
    """dict(net, head, R, radius, near, far, rays [R] (pool rows), dz [R, 1], forward, ref = reference64) of one row of
    `cases(name)`, cached."""
    if (name, key) not in _cases:
        head, R, radius, near, far, seed = key
        net = network(name)
        among = None
        if head != "main" and R < 100:                 # the chain is not zero, and the sigmoid not saturated: s (1 - s) > 2^-12
            v = pool_head_sum(net, head)
            among = (v != 0) & (np.abs(v) <= UNSATURATED)
        rays = X.ray_indices(R, radius, seed=seed, among=among)
        if head != "main":                             # the last ray is the chosen one whose sigmoid is furthest from saturation
            j = int(np.argmin(np.abs(pool_head_sum(net, head)[rays])))
            rays[[j, -1]] = rays[[-1, j]]
        dz = make_dz(R, seed)
        fwd = forward64(net, rays)
        ref = reference64(net, head, rays, dz, near, far, radius, forward=fwd)
        _cases[name, key] = dict(name=name, net=net, head=head, R=R, radius=radius, near=near, far=far, rays=rays, dz=dz, forward=fwd, ref=ref)
    return _cases[name, key]


def mutant_of(c, mutant=None, slope=None):
    return reference64(c["net"], c["head"], c["rays"], c["dz"], c["near"], c["far"], c["radius"], mutant=mutant, slope=slope,
                       bounds=False, forward=c["forward"])


# ---- the conditions ---------------------------------------------------------------------------------------------------------
def check_v1(c):
    """V1 on the case's rays."""
    net, seen = c["net"], c["forward"]["seen"]
    layers = X.kernel_layers(net)
    for l, ((w, b), (inp, pre, out)) in enumerate(zip(layers, seen)):
        ordn, special = np.array(net["ordinary"][l]), X.chain_units(net, l)
        cols = np.flatnonzero(w[ordn].any(axis=0))
        q = min(E.quantum(w[ordn][:, cols]) * E.quantum(inp[:, cols]), E.quantum(b[ordn]))
        p = pre[:, ordn]
        assert (p >= 0).all(), f"V1: an ordinary unit of layer {l} is negative"
        assert ((p == 0) | (p >= q)).all() and (p / q == np.rint(p / q)).all(), f"V1: layer {l}: a pre-activation within {q} of zero"
        assert (out[:, ordn] == p).all() and E.is_f32(pre), f"V1: layer {l}"
        for u in special:
            assert E.is_f32(out[:, u]) and (out[:, u] == X.leaky(pre[:, u], "f32")).all(), f"V1: chain unit {u} of layer {l}"
            assert ((pre[:, u] > 0) == (out[:, u] > 0)).all() and ((pre[:, u] < 0) == (out[:, u] < 0)).all()


def slope_rejections(c):
    """[n, 2] bool: whether the case rejects trunk layer l's negative-branch slope set to 1, and to 0 (V2's raw material)."""
    n = len(c["net"]["cat"])
    return np.array([[rejected(c["ref"], mutant_of(c, slope=(l, val))) for val in (1.0, 0.0)] for l in range(n)])


def block_sharpness(c):
    """name -> (least, largest) over the tensor's 16-row blocks of the block's max |ref| / bound (inf where the bound is 0 and
    the reference is not)."""
    out = {}
    for k, (v, bnd) in c["ref"]["grads"].items():
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(v == 0, 0.0, np.abs(v) / bnd)
        r = r.reshape(r.shape[0], -1).max(axis=1)
        blocks = [r[lo:lo + 16].max() for lo in range(0, len(r), 16)]
        out[k] = (float(min(blocks)), float(max(blocks)))
    return out


def check_v3(c):
    """V3 on a case of the main head."""
    assert c["head"] == "main"
    for k, (v, bnd) in c["ref"]["grads"].items():
        assert v.any(), f"V3: {k} is identically zero"
    if c["R"] >= BLOCK_ROWS and c["name"] not in LOOSE:
        for k, (least, _) in block_sharpness(c).items():
            assert least > 2.0, f"V3: a 16-row block of {k} holds no entry above two bounds ({least})"


def check_zeros(c):
    """Under a chain head the branches' gradients are exact zeros with bound 0; a dW row whose unit no ray drives is so too."""
    if c["head"] != "main":
        n = len(c["net"]["cat"])
        for k in param_names(c["net"])[:6 * n]:
            v, bnd = c["ref"]["grads"][k]
            assert not v.any() and not bnd.any(), f"{k} under {c['head']}"
    for k, (v, bnd) in c["ref"]["grads"].items():
        assert (bnd >= 0).all() and np.isfinite(bnd).all() and not ((bnd == 0) & (v != 0)).any(), k
