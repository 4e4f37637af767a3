"""DepthNets on which every forward kernel must return one head sum, and rays on which its ray-sphere arithmetic is exact.

Shared by tests/test_exact_depthnet_host.py (the conditions below, the fold, the fp32 oracle and the mutants, on the CPU) and
tests/test_gpu_exact_depthnet.py (the HIP kernels).  Nothing here calls the library.

The network is the reference's (depth_net.py:117-169): three affine branches on cat[h, gamma(.)] over the embeddings of o, d
and the six sphere-intersection coordinates, the LeakyReLU trunk on cat[h_o, h_d, h_x, e_o, e_d, e_x], to_depth, a sigmoid,
z = near (1 - s) + far s.  The kernels run it folded (ns_pack.hip: the branches composed into trunk layer 0) and form their
inputs themselves from (o, d); `make_exact_depthnet` draws weights, and `pool` picks rays, so that nothing up to the head's
sum is ever rounded -- except where this file rounds it too.

The rays.  Integer origins in [-6, 6]^3, integer directions in {-2..2}^3 without 0, sphere_radius 3.  `exact_rays` evaluates
the kernels' formula (ns_depthnet.hip:51-58) in float64 and in float32 and keeps a ray if every intermediate -- the three
products, b, |o|^2, |o|, c, a, the discriminant, its root, both t, the six coordinates -- is the same number in both, |o|, the
root and both t invert exactly, and the coordinates are bf16 and f16 numbers: 2964 rays, 516 distinct coordinate tuples, 124
directions; all their coordinates are integers.  The pool is one ray per tuple, and the 36 tuples that radius 2, the
production value, leaves: 552 rays.  The test relies on the device's sqrtf and division being correctly rounded (the build has
no fast-math flag); a perfect square that came back inexact would fail it, and would be a finding.  Eight more rays miss both
spheres exactly: their z is NaN, and only theirs.

The conditions, on the pool, for every operand type:

    D1  every trunk and head weight and bias, and every entry of the folded front (F, fb) as ns_fold_depthnet_front returns it,
        is a bf16 and an f16 number; the library's fold is the float64 fold `fold64`, exactly;
    D2  layer 0 reads the 12 identity columns of the embedding alone (o, d, the six coordinates), each directly and through its
        branch; every sine and cosine column has weight exactly zero;
    D3  C3 of exact_field.py: in every layer and on every ray (sum_k |w_k a_k| + |b|) / q < 2^24, on the activations as the
        operand type forms them (below), over the three products for split operands, and for the literal unfolded chain too;
    D4  every ordinary unit is positive on at least 10 % of the pool and zero on some ray, never negative; neighbouring
        16-row blocks hold different biases; every chain unit is negative on 10 % and positive on 10 %;
    D5  zeroing any 32-column input block or any 16-row output block of any layer, or exchanging two neighbouring bias blocks,
        moves z on some ray by more than twice the gate;
    D6  one quantum q of the main head's sum moves z by at least 16 gates on every ray: (far - near) s (1 - s) q >= 16 gate.
        With D5 a wrong term is a failure, not sigmoid saturation.  A chain head's sum is one product that spans a factor of
        a hundred between a ray's two branches, so no scale holds every ray off saturation: there q is 2^-13 of the sum, and
        D6 is asked of a quarter of the pool under the better of the head's two scales; that every sub-block's mutant moves
        z by more than twice the gate is asserted outright (`check_chains_cover`).

LeakyReLU's slope is no dyadic number, so a negative sum leaves the activation with a full mantissa.  The reference applies
each kernel's rule as a rounding function (`leaky`) behind an exact sum:

    f32     v > 0 ? v : fl32(0.01f v)                                    (to_blocks, ns_mlp_engine.h)
    bf16    the same product in fp32, then round-to-nearest-even to bf16  (convert_piece16)
    f16     x = fl16(v), then max(x, fl16(0x211f x))                     (Mma16F16::leaky2: packed multiply and max)
    f16x3   a = the fp32 rule, hi = fl16(a), lo = fl16(a - hi); the next layer sees hi + lo   (convert_piece16x3)
    f16m    the f16x3 rule in layers 0 .. NS_F16M_SPLIT_LAYERS - 1, the last of them handing on hi alone; the f16 rule from there on

and a negative sum is allowed in chain units only.  A sign unit is SIGN o_j + SIGN2 o_j' (two terms, an exact sum: an affine
function of integer coordinates takes both signs on one coordinate only, so it is no wider); from it on, one single-term row
per layer, weight -2^j and bias 0, reads the chain unit of the layer before: one product of two representable numbers is exact
in float64, so the reference models every step, roundings included.  The sign alternates from layer to layer, so in every
layer the chain unit is negative on part of the pool; -2^j is chosen per layer so that the largest |value| stays in
[2^14, 2^15) (a fixed 2^7 would grow a hundredfold every second layer), which keeps every value, and every split remainder,
zero or a normal f16 number (`check_chain_range`, numpy's float16).  Ordinary units never read a chain unit.  A chain reaches z
through a head that reads its last unit alone, at two scales ("chain<c>", "chain<c>s": the rays on which the last unit is
negative are a hundred times smaller); one network is packed once per head.  Every head runs at every ray count and at
both radii, a chain head's launches of fewer than a hundred rays on rays where the chain is not zero.  Chain c runs through sub-block c of every layer,
so across the heads every 16-row sub-block of every trunk layer takes its negative branch on a value that reaches z: the
host test drops that branch, and swaps the two slopes, sub-block by sub-block, and the comparison rejects each (a swapped
slope, 2^-12 off, only where a 16-bit rounding does not follow: not for bf16, nor in f16m's split layers).

Ordinary rows (`make_exact_depthnet`): while no unit is negative the trunk is affine on the pool, so a unit is given what it is
to be -- t . (o, d, x6) + bias, two to four coordinates, within [0, 120] in steps of 1/2 -- and a row that arrives there: eight
units of the layer before with coefficients from {+-1/2, +-1}, and on twelve basis units (the coordinates themselves, built
the same way) what their sum lacks of t.  `add_remainders` is exact_field's split-operand family: one layer's weights become
w (1 + 2^-12), on networks whose units stay at least 4 above zero and are one unit plus or minus one coordinate each.

Which network reaches which kernel (hidden_sizes are the branches'; W is the trunk padded to 128 or 256; "left over" is the
odd layer `if (l < a.n_layers)` of depthnet_ob16_kernel's two-layers-a-trip loop):

    network   cat_hidden_sizes        W    layers  trips, left over   f32                 bf16 / f16 / f16x3 (generic)      f16 / f16x3 production     f16m
    prod      [256] * 10              256  10      4, taken           depthnet_kernel<8>  ob16<8> (generic_kernels=1)       ob16<8, PROD> (default)    depthnet_mix_kernel<3>
    default   [128]*4 + [256]         256  5       2, not taken       depthnet_kernel<8>  ob16<8>
    ragged    [64, 16, 200, 256]      256  4       1, taken           depthnet_kernel<8>  ob16<8>
    w256n2    [256, 144]              256  2       0, taken           depthnet_kernel<8>  ob16<8>
    tiny      [96]                    128  1       0, not taken       depthnet_kernel<4>  ob16<4>
    w128n3    [128, 112, 128]         128  3       1, not taken       depthnet_kernel<4>  ob16<4>
    w128n2    [128, 128]              128  2       0, taken           depthnet_kernel<4>  ob16<4>

(ob16<NKB> is depthnet_ob16_kernel over Plain16<Mma16BF16>, Plain16<Mma16F16> and Split16: eleven instantiations with the two
PROD bodies and the mixed kernel.)  The remainder family runs on "prod" (f32, f16x3 on both bodies, f16m's three split
layers) and "w128n3" (f32, f16x3), one layer at a time, the head included.

The gate: |z - z64| <= 8 U max(|near|, |far|), U = 2^-24.  With D1 - D3 the head's sum v is the float64 value in every kernel,
so z differs by what the sigmoid and the mix round: e = expf(-v) up to 2 U relative (1 ulp), which s = 1 / (1 + e) sees as at
most 2 U e / (1 + e) <= 2 U relative; 1 + e half a U, the division half a U, 1 - s half a U of 1, the two products half a U
each of their size and the sum half a U of z: about 4 U max(|near|, |far|) in all, and a factor of two over it.
Measured, worst |z - z64| / gate over every case of tests/test_gpu_exact_depthnet.py on an MI355X: depthnet_kernel 0.258,
ob16 bf16 0.238, f16 0.239, f16x3 0.249, both PROD bodies and the mixed kernel 0.236; the fp32 oracle on the CPU
(oracle.nerf_oracle.depthnet_forward, torch's sigmoid): 0.258 on one host; the figure moves with torch's expf, so its test
holds the oracle to the derivation's 4 U, half the gate, and not to the figure.  Were the device's expf to need a wider
gate, it could grow to no more than twice the oracle's worst error, 0.52 of the present gate: the gate is wider than that
already and stays where the derivation puts it.

Part B, the 240 columns that part A gives weight zero.  A probe network is one branch layer and one trunk layer of one-hot
rows: hidden unit j is embedding column j (times -1 for some columns that take both signs), for the columns with an odd index
in their embedding through the branch and the fold's product, for the others through the direct skip; F stays a 0 / +-1
matrix, which the host test holds against ns_fold_depthnet_front.  The head reads the six columns g, g + 42, .., g + 210 with
the weights PROBE_HEAD from {+-1, +-1/2} (six weights cannot all differ; neighbours do, and the six columns lie in different
embeddings and levels): 42 heads, every column in one.  At a 128-wide trunk the same groups sit on six trunks of 42 units.
The rays (`probe_rays`) are the production geometry at radius 2 with |o| about 4, and rays with components exactly 0,
negative, 2^-20 and of magnitude 8 in o and in d; three miss and stay NaN; near = 0, far = 1.  The reference is the float64
chain on fp32 inputs with the operand type's slope constant and no other rounding; the six intersection coordinates are the
kernels' own fp32 numbers (`kernel_x6`: their rounding at level 9 is worth 2^9 of it in the argument, and is not what is
under test; the host test feeds the fp32 oracle's own coordinates to the same reference).  The gate:

    |z - z64| <= (1/4) sum_j |w_j| tau_t + 4 U                      (1/4: the sigmoid's largest slope; 4 U: the head, part A)

    with, for bf16 and f16 alone, max(1, |e_j|) tau_t in place of tau_t for an identity column j (`probe_reference`).

    tau = 8 U for f32 and f16x3, Trig<true> (ns_mlp_engine.h:428-453), walking the code: x / (2 pi) is a two-float product and
    fract(2^l hi) is exact, so the reduced argument f + lo is off by its one rounding, half a U of a revolution: pi U in the
    angle; the constant 6.2831855f and the product g * 6.2831855f cost 0.28 U + 0.5 U of an angle of at most pi / 2: 1.7 U with
    the rounding of x itself carried through the series' slope; the degree-11 series truncated at pi / 2 leaves
    (pi / 2)^13 / 13! = 5.7e-8 = 0.95 U; the Horner steps and the last fused step about 1.8 U: 7.6 U in all, rounded up.
    An identity column (o, d, the six coordinates: up to 8 on these rays) costs f32 nothing: the k-major engine holds it as
    it is.  The split engine holds hi = fl16(x) and lo = fl16(x - hi): for 2^k <= |x| < 2^(k+1) the remainder is at most
    2^(k-11), where an f16 number's half-ulp is 2^(k-23), so hi + lo misses x by at most 2^-23 |x| = 2 U |x|: 4 U below 4
    and 8 U below 8, within tau as it stands, and the components that are 8 are f16 numbers (no factor for f16x3 either;
    the same count gives a sine or cosine U, inside the "rounded up").
    tau = 2^-8 + 2^-18 for bf16 and 2^-11 + 2^-18 for f16: the operand's rounding of the column and of the activation
    behind it (2^-9 and 2^-12 each), and 2^-18 for v_sin_f32, four times the "~1e-6" that ns_depthnet_ob16.hip's Split16
    states for it.  That rounding is relative, and the issue's tau counts it for a column within [-1, 1]; an identity
    column reaches 8 here, where an f16 operand is 2^-9 off and tau would fail a correct kernel.  So for these two operand
    types, and for identity columns only, tau is taken max(1, |e_j|) times; every sine and cosine column, of every operand
    type, is held to the tau of the table.

Measured on an MI355X, worst |z - z64| / gate over all 42 groups and 210 rays: f32 0.131 (embed3, embed6), f16x3 0.161
(embedN_16, Trig<true>), bf16 0.304, f16 0.360 (embedN_16, v_sin_f32); at the 128-wide trunks f32 0.131, f16 0.360; the fp32
oracle on the CPU 0.155 on one host (it moves with torch's sine and expf; its test holds it to the gate).  This catches a column delivered to the wrong slot, level, component or phase and any sign error in
the three embeddings and the packer's maps, and a precision loss of about 5e-6 in one column; it is no 1-ulp test of the sine.
f16m has no such shape and is covered by part A alone.
"""

import itertools

import numpy as np
import torch

import exact_field as E

U = 2.0 ** -24
EMB = 252                                   # cat[gamma(o), gamma(d), gamma(x6)]: 63 + 63 + 126 columns
ID_COLS = np.array([0, 1, 2, 63, 64, 65, 126, 127, 128, 129, 130, 131])      # o, d, the six intersection coordinates
BRANCH_ID = (np.arange(3), np.arange(3), np.arange(6))                       # the identity columns of each branch's embedding
BRANCH_DIM = (63, 63, 126)
BRANCH_AT = (0, 3, 6)                       # where each branch's identity columns start among the 12
F16M_SPLIT_LAYERS = 3                       # NS_F16M_SPLIT_LAYERS (tests/test_host_logic.py pins the header's value)
DTYPES = ("f32", "bf16", "f16", "f16x3", "f16m")
SLOPE32 = float(np.float32(0.01))           # 0.01f
SLOPE16 = float(np.float16(0.01))           # 0x211f
QSTAR = 0.5                                 # every ordinary term is a multiple of it: the pool holds integers
SBOUND = 0.9 * 2.0 ** 12 * QSTAR            # a row's sum of magnitudes: leaves the remainder family its 12 bits
SPREAD = 120.0                              # an ordinary unit's max - min on the pool: with its least value at 0 it lies in [0, 120], and
                                            # is a multiple of q*: 8 bits
BRANCH_LIMIT, BRANCH_ENTRY = 8.0, 4.0      # a branch unit on the pool; an entry of a branch's composed map
HEAD_MAX = 3.0                              # the main head's |sum| on the pool
SIGN, SIGN2 = 59.0 * 2.0 ** 6, 2.0 ** 9      # a sign unit is SIGN o_j + SIGN2 o_j', |o| <= 6: o_j gives the sign, and the 160 nonzero sums
                                            # have mantissas enough that the fp16 slope 0x211f and 0.01f, one fp16 number on a power of
                                            # two, round apart on many of them in every layer
CHAIN_TOP = 2.0 ** 15                       # a relay's weight -2^j brings the chain's largest |value| into [2^14, 2^15)
MARGIN = 4.0                                # the least value of an ordinary unit of a remainder base network
RADII = (3.0, 2.0)
NEAR_FAR = ((2.0, 6.0), (0.0, 1.0))
ORACLE_BOUND = 0.5                          # the fp32 oracle's |err| / gate on the CPU: the derivation's 4 U of the gate's 8 U
RAY_COUNTS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1300)

PROD = "prod"
# name -> (hidden_sizes, cat_hidden_sizes, seed); PROD's sizes are those of synthetic.SCENES["lego_synth"]["depth"]
NETWORKS = {
    PROD: ([256] * 10, [256] * 10, 21),
    "default": ([128] * 6, [128, 128, 128, 128, 256], 22),
    "ragged": ([48, 80], [64, 16, 200, 256], 23),
    "tiny": ([32], [96], 24),
    "w128n3": ([40, 24], [128, 112, 128], 25),
    "w128n2": ([24], [128, 128], 26),
    "w256n2": ([24], [256, 144], 27),
}
REMAINDER_NETWORKS = (PROD, "w128n3")
REMAINDER_DTYPES = ("f32", "f16x3", "f16m")


def remainder_layers(name, dtype):
    """The layers that carry the remainders in turn: every split layer of the operand type (the head is layer n)."""
    n = len(NETWORKS[name][1])
    return list(range(F16M_SPLIT_LAYERS)) if dtype == "f16m" else list(range(n + 1))


def dtypes_of(name):
    return DTYPES if name == PROD else DTYPES[:4]


# ---- the rays -------------------------------------------------------------------------------------------------------
def intersect(o, d, radius, dtype):
    """The kernels' ray-sphere arithmetic (ns_depthnet.hip:51-58) in `dtype`, every intermediate kept."""
    o, d = np.asarray(o, dtype=dtype), np.asarray(d, dtype=dtype)
    two, four, r = dtype(2), dtype(4), dtype(radius)
    s = dict(p0=d[:, 0] * o[:, 0], p1=d[:, 1] * o[:, 1], p2=d[:, 2] * o[:, 2])
    s["b"] = two * ((s["p0"] + s["p1"]) + s["p2"])
    s["on2"] = o[:, 2] * o[:, 2] + (o[:, 1] * o[:, 1] + o[:, 0] * o[:, 0])       # exact here, so the fused form equals it
    with np.errstate(invalid="ignore", divide="ignore"):
        s["on"] = np.sqrt(s["on2"])
        s["c"] = s["on"] * s["on"] - r * r
        s["aa"] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        s["disc"] = s["b"] * s["b"] - four * s["aa"] * s["c"]
        s["sq"] = np.sqrt(s["disc"])
        s["t0"] = (-s["b"] - s["sq"]) / (two * s["aa"])
        s["t1"] = (-s["b"] + s["sq"]) / (two * s["aa"])
    s["x"] = np.concatenate([o + s["t0"][:, None] * d, o + s["t1"][:, None] * d], axis=1)
    return s


def exact_rays(o, d, radius):
    """(keep, miss, x6): keep[r] where the kernels' formula gives one value at every intermediate in float64 and in float32
    -- an inexact root or quotient rounds differently at 53 and at 24 bits -- |o|, the root and both t are exact by the
    inverse operation as well, and the six coordinates are bf16 and f16 numbers; miss[r] where both precisions find a negative
    discriminant exactly."""
    a, b = intersect(o, d, radius, np.float64), intersect(o, d, radius, np.float32)
    same = np.ones(len(a["b"]), dtype=bool)
    for k in ("p0", "p1", "p2", "b", "on2", "on", "c", "aa", "disc"):
        same &= a[k] == b[k].astype(np.float64)
    miss = same & (a["disc"] < 0)
    keep = same & (a["disc"] >= 0)
    with np.errstate(invalid="ignore"):
        for k in ("sq", "t0", "t1"):
            keep &= a[k] == b[k].astype(np.float64)
        keep &= (a["x"] == b["x"].astype(np.float64)).all(axis=1)
        keep &= (a["on"] * a["on"] == a["on2"]) & (a["sq"] * a["sq"] == a["disc"])
        keep &= (a["t0"] * (2 * a["aa"]) == -a["b"] - a["sq"]) & (a["t1"] * (2 * a["aa"]) == -a["b"] + a["sq"])
        keep &= E.fits16(np.where(np.isfinite(a["x"]), a["x"], 1.0 / 3)).all(axis=1)
    return keep, miss, a["x"]


def all_exact_rays(radius):
    """Every integer ray (o in [-6, 6]^3, d in {-2..2}^3 without 0) that `exact_rays` keeps: (o, d, x6); and those that miss."""
    O = np.array(list(itertools.product(range(-6, 7), repeat=3)), dtype=np.float64)
    D = np.array([v for v in itertools.product(range(-2, 3), repeat=3) if any(v)], dtype=np.float64)
    o, d = np.repeat(O, len(D), axis=0), np.tile(D, (len(O), 1))
    keep, miss, x = exact_rays(o, d, radius)
    return (o[keep], d[keep], x[keep]), (o[miss], d[miss])


_pool = {}


def pool():
    """The pool: one ray for every distinct tuple of intersection coordinates at radius 3 (516) and at radius 2 (36), picked
    by a fixed permutation so that origins and directions vary, as a dict o, d, x [P, 3 / 3 / 6], radius [P], x12 [P, 12],
    and miss_o, miss_d [8, 3]: rays that miss both spheres."""
    if not _pool:
        parts = []
        for radius in RADII:
            (o, d, x), (mo, md) = all_exact_rays(radius)
            order = np.random.default_rng(int(radius)).permutation(len(o))
            _, first = np.unique(x[order], axis=0, return_index=True)
            idx = np.sort(order[first])
            parts.append((o[idx], d[idx], x[idx], np.full(len(idx), radius)))
            if radius == RADII[0]:
                pick = np.random.default_rng(99).permutation(len(mo))[:8]
                _pool.update(miss_o=mo[pick], miss_d=md[pick], counts=(len(o), len(idx), len(np.unique(d, axis=0))))
        o, d, x, radius = (np.concatenate(p) for p in zip(*parts))
        _pool.update(o=o, d=d, x=x, radius=radius, x12=np.concatenate([o, d, x], axis=1))
    return _pool


def ray_indices(R, radius, seed=0, among=None):
    """R pool rays of one radius, cyclically from a fixed permutation of them; of those that `among` [P] marks, if given."""
    own = np.flatnonzero((pool()["radius"] == radius) & (True if among is None else among))
    perm = np.random.default_rng(3000 + seed).permutation(own)
    return perm[np.arange(R) % len(perm)]


# ---- the operand types' activation rules ----------------------------------------------------------------------------
def f32r(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def f16r(a):
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def bf16r(a):
    """fp32, then round-to-nearest-even to bf16 (tests/test_exact_depthnet_host.py holds it against torch's conversion)."""
    x = np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))
    bits = x.view(np.uint32).astype(np.uint64)
    bits = ((bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return np.where(np.isnan(x), np.nan, bits.view(np.float32).astype(np.float64))


def layer_rules(dtype, n_layers):
    """The rule each trunk layer's output is formed by."""
    if dtype == "f16m":
        kx = F16M_SPLIT_LAYERS
        return ["x3"] * (kx - 1) + ["x3hi"] + ["f16"] * (n_layers - kx)
    return [{"f32": "f32", "bf16": "bf16", "f16": "f16", "f16x3": "x3"}[dtype]] * n_layers


def leaky(pre, rule, slope32=SLOPE32, slope16=SLOPE16):
    """LeakyReLU of exact sums `pre` as the operand type forms it: a rounding function (the table in the module docstring)."""
    pre = np.asarray(pre, dtype=np.float64)
    if rule == "f16":
        x = f16r(pre)
        return np.maximum(x, f16r(slope16 * x))
    with np.errstate(invalid="ignore"):
        a = np.where(pre > 0, pre, f32r(slope32 * pre))
    if rule == "f32":
        return a
    if rule == "bf16":
        return bf16r(a)
    hi = f16r(a)
    return hi if rule == "x3hi" else hi + f16r(a - hi)


# ---- the generator --------------------------------------------------------------------------------------------------
def _blocks(width):
    return [(s, min(s + 16, width)) for s in range(0, width, 16)]


def _plan(cat, chains):
    """Where the hand-made units sit.  Chain c runs through sub-block min(c, last) of every layer from the first one that has
    more than c sub-blocks on; twelve basis units per layer are the coordinates themselves on the pool (o_j + 6, d_j + 2, x_j + 3 >= 0), at the end of rows
    as wide as any other.
    Returns (chain[c] = dict layer -> unit, basis[l] = 12 units)."""
    taken = [set() for _ in cat]
    chain = []
    n_chains = max(len(_blocks(w)) for w in cat) if chains else 0
    for c in range(n_chains):
        start = next(l for l, w in enumerate(cat) if len(_blocks(w)) > c)
        units = {}
        for l in range(start, len(cat)):
            lo, hi = _blocks(cat[l])[min(c, len(_blocks(cat[l])) - 1)]
            u = next(lo + (c + l + k) % (hi - lo) for k in range(hi - lo) if lo + (c + l + k) % (hi - lo) not in taken[l])
            taken[l].add(u)
            units[l] = u
        chain.append(units)
    basis = []
    for l, w in enumerate(cat):
        free = [u for u in range(w) if u not in taken[l]]
        step = max((len(free) - 5) // 12, 1)
        pick = free[:12] if step == 1 else free[(7 * l) % 5::step][:12]     # spread over the layer's sub-blocks
        assert len(pick) == 12, "a trunk layer needs room for the twelve basis units beside its chain units"
        taken[l].update(pick)
        basis.append(pick)
    return chain, basis


BASIS_OFFSET = np.array([6.0] * 3 + [2.0] * 3 + [3.0] * 6)
TARGET_COEFS = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


def _target(rng, x12, coefs=TARGET_COEFS):
    """What an ordinary unit is on the pool, up to its bias: t . (o, d, x6), two to four coordinates with coefficients from
    TARGET_COEFS, its max - min on the pool within SPREAD."""
    while True:
        t = np.zeros(12)
        k = int(rng.integers(2, 5))
        t[rng.choice(12, size=k, replace=False)] = rng.choice(coefs, size=k)
        v = x12 @ t
        if v.max() - v.min() <= SPREAD and len(np.unique(v)) > 4:
            return t


def _draw_branch(rng, b, hidden, x12):
    """One affine branch on cat[h, e] (depth_net.py:136-156): sparse rows of +-1 and 2 over the units before and the identity
    columns of the embedding, every unit within BRANCH_LIMIT on the pool and every entry of the composed map within
    BRANCH_ENTRY.  Returns (weights, biases, map [H, n_id], constant [H])."""
    ids, dim = BRANCH_ID[b], BRANCH_DIM[b]
    e = np.zeros((len(x12), dim))
    e[:, ids] = x12[:, BRANCH_AT[b]:BRANCH_AT[b] + len(ids)]
    ws, bs = [], []
    h, A, c = e, np.zeros((dim, len(ids))), np.zeros(dim)
    A[ids, np.arange(len(ids))] = 1.0
    for size in hidden:
        inp = np.concatenate([h, e], axis=1)
        nh = h.shape[1]
        permitted = np.concatenate([np.arange(nh) if h is not e else ids, nh + ids])
        Aprev, cprev = A, c

        def small(cols, coef, bval, Aprev=Aprev, nh=nh, ids=ids):
            row = np.zeros(len(ids))
            for k, v in zip(cols, coef):
                row += v * (Aprev[k] if k < nh else np.eye(len(ids))[k - nh])
            return bool(np.abs(row).max() <= BRANCH_ENTRY)

        w, bias, pre = E._draw_layer(rng, inp, size, permitted, False, QSTAR, SBOUND, coarse_only=True, start=4,
                                     limit=BRANCH_LIMIT, accept=small, one_seed=True)
        ws.append(w)
        bs.append(bias)
        A = w[:, :nh] @ Aprev + w[:, nh:][:, ids]
        c = w[:, :nh] @ cprev + bias
        h = pre
    return ws, bs, A, c


def make_exact_depthnet(hidden_sizes, cat_hidden_sizes, seed, chains=True, margin=0.0):
    """A DepthNet whose every sum on the pool is exact (D1 - D6 of the module docstring), as a dict:
    hidden, cat, branch_w / branch_b (three lists), cat_w / cat_b (the literal trunk, layer 0 on cat[h_o, h_d, h_x, e_o, e_d, e_x]),
    heads (name -> (weights [1, C], bias [1]): "main" and two per chain), chain, basis, ordinary (per layer, the units that
    are no chain units), margin, remainder (None).

    The trunk is affine on the pool as long as no unit is negative, so an ordinary unit can be given what it is to be there --
    a target t . (o, d, x6) + bias of small spread (`_target`) -- and a wide row that arrives at it: `terms` units of the layer
    before with random coefficients, and on the twelve basis units what their sum lacks of t.  Its bias puts its least value
    on the pool at `margin`.  In a remainder base network (margin > 0) a unit is one unit of the layer before plus or minus one
    coordinate, and a basis unit a copy: the biases a remainder is carried through then add up instead of multiplying, so that
    no unit comes near zero, and the sums keep 12 bits free."""
    hidden, cat = list(hidden_sizes), list(cat_hidden_sizes)
    x12 = pool()["x12"]
    assert (x12.min(axis=0) == -BASIS_OFFSET).all()
    chain, basis = _plan(cat, chains)
    HL = hidden[-1]
    terms, coefs = (1, (1.0,)) if margin else (8, (-1.0, -0.5, 0.5, 1.0))
    for attempt in range(20):
        rng = np.random.default_rng([seed, attempt])
        try:
            br = [_draw_branch(rng, b, hidden, x12) for b in range(3)]
        except E._Unfit:
            continue
        break
    else:
        raise RuntimeError("make_exact_depthnet: no branch fits the conditions; change the generator, not the conditions")
    hb = [x12[:, BRANCH_AT[b]:BRANCH_AT[b] + len(BRANCH_ID[b])] @ br[b][2].T + br[b][3] for b in range(3)]
    inp = np.zeros((len(x12), 3 * HL + EMB))
    inp[:, :3 * HL] = np.concatenate(hb, axis=1)
    inp[:, 3 * HL + ID_COLS] = x12
    A = np.zeros((3 * HL, 12))                      # the branches' composed maps: h = A (o, d, x6) + cst
    for b in range(3):
        A[b * HL:(b + 1) * HL, BRANCH_AT[b]:BRANCH_AT[b] + len(BRANCH_ID[b])] = br[b][2]
    cst = np.concatenate([br[b][3] for b in range(3)])
    cat_w, cat_b, ordinary, grad = [], [], [], []
    act = None
    for l, width in enumerate(cat):
        special = {units[l] for units in chain if l in units}
        K = inp.shape[1] if l == 0 else cat[l - 1]
        W, B, g = np.zeros((width, K)), np.zeros(width), np.zeros((width, 12))
        if l == 0:
            sources, gsrc = np.arange(3 * HL), A
            fix = 3 * HL + ID_COLS                  # the columns that hold the coordinates themselves
        else:
            sources = np.array([u for u in ordinary[l - 1] if u not in basis[l - 1]], dtype=int)
            gsrc, fix = grad[l - 1], np.array(basis[l - 1])
        order = rng.permutation(len(sources)) if len(sources) else np.zeros(0, dtype=int)
        src = inp if l == 0 else act
        row = 0
        for u in range(width):
            if u in special:
                continue
            for _ in range(200):
                t = np.eye(12)[basis[l].index(u)] if u in basis[l] else _target(rng, x12)      # a basis unit: one coordinate
                n = min(terms, len(sources)) if not (margin and u in basis[l]) else 0
                cols = np.zeros(0, dtype=int)
                if n:
                    first = sources[order[row % len(order)]]             # every unit of the layer before is read by some row
                    rest = rng.choice(sources[sources != first], size=n - 1, replace=False) if n > 1 else np.zeros(0, dtype=int)
                    cols = np.concatenate([[first], rest]).astype(int)
                c = rng.choice(coefs, size=len(cols))
                if margin and len(cols):                  # a remainder base: the unit before, plus or minus one coordinate
                    c = np.ones(1)
                    t = gsrc[cols[0]] + rng.choice([-1.0, 1.0]) * np.eye(12)[rng.integers(12)]
                    v = x12 @ t
                    if v.max() - v.min() > 90 or len(np.unique(v)) <= 4:
                        continue
                lack = t - c @ gsrc[cols] if len(cols) else t
                literal = -(c @ cst[cols]) if l == 0 else 0.0         # layer 0: what the branches' constants add to the folded bias
                if not (E.fits16(lack).all() and np.abs(lack).max() <= 16 and abs(literal) <= 64):
                    continue
                low = float((src[:, cols] @ c + src[:, fix] @ lack).min())      # the bias is margin - low: a 16-bit number
                if E.fits16(np.array([margin - low, margin - low - literal])).all():
                    break
            else:
                raise RuntimeError("make_exact_depthnet: a row does not fit; change the generator, not the conditions")
            W[u, cols] = c
            W[u, fix] += lack
            g[u] = t
            row += 1
        rows = np.array([u for u in range(width) if u not in special], dtype=int)
        if len(rows):
            pre = src @ W[rows].T
            B[rows] = margin - pre.min(axis=0)                            # every ordinary unit: least value `margin`
        for c, units in enumerate(chain):
            if l not in units:
                continue
            u, j = units[l], c % 3
            if l - 1 in units:                                      # a relay: one term, -2^j, no bias
                top = np.abs(act[:, units[l - 1]]).max()
                W[u, units[l - 1]] = -2.0 ** np.floor(np.log2(CHAIN_TOP / top * (1 - 2.0 ** -20)))
            else:                                                   # a sign unit: SIGN o_j + SIGN2 o_j'
                W[u, fix[j]], W[u, fix[(j + 1) % 3]] = SIGN, SIGN2
                B[u] = 0.0 if l == 0 else -(SIGN * BASIS_OFFSET[j] + SIGN2 * BASIS_OFFSET[(j + 1) % 3])
        cat_w.append(W)
        cat_b.append(B)
        grad.append(g)
        ordinary.append([u for u in range(width) if u not in special])
        act = leaky(src @ W.T + B, "f32")
    net = dict(hidden=hidden, cat=cat, branch_w=[b[0] for b in br], branch_b=[b[1] for b in br], cat_w=cat_w, cat_b=cat_b,
               chain=chain, basis=basis, ordinary=ordinary, margin=margin, remainder=None, heads={})
    # the main head: every ordinary unit of the last layer (a remainder base: two of every 16-row block) with +-2^-e, centred
    last = np.array(ordinary[-1])
    if margin:
        last = np.concatenate([rng.choice(np.intersect1d(last, np.arange(lo, hi)), size=2, replace=False) for lo, hi in _blocks(cat[-1])])
    sign = rng.permutation(np.where(np.arange(len(last)) % 2 == 0, 1.0, -1.0))
    s = act[:, last] @ sign
    centre = np.rint((s.max() + s.min()) / 2)
    e = int(np.ceil(np.log2(max(np.abs(s - centre).max(), 1.0) / (HEAD_MAX - 0.5))))
    hw = np.zeros((1, cat[-1]))
    hw[0, last] = sign * 2.0 ** -e
    hb = -float(bf16r(np.array([centre * 2.0 ** -e]))[0])            # a 16-bit number near the centre
    net["heads"]["main"] = (hw, np.array([hb]))
    # chain c alone, at two scales: the rays on which its last unit is positive reach |v| in (2, 4) through "chain<c>"; those
    # on which it is negative there, a hundred times smaller, through "chain<c>s", whose weight is 64 times larger
    for c, units in enumerate(chain):
        top = np.abs(act[:, units[len(cat) - 1]]).max()
        for tag, scale in (("", 1.0), ("s", 64.0)):
            hw = np.zeros((1, cat[-1]))
            hw[0, units[len(cat) - 1]] = (1.0 if c % 2 else -1.0) * scale * 2.0 ** np.floor(np.log2(4.0 / top * (1 - 2.0 ** -20)))
            net["heads"][f"chain{c}{tag}"] = (hw, np.zeros(1))
    return net


def add_remainders(net, layer):
    """exact_field.add_remainders on the DepthNet: a copy of a remainder base network (margin > 0, no chains) whose trunk layer
    `layer` (len(cat): the main head) has the weights w (1 + 2^-12); the biases stay."""
    assert net["remainder"] is None and net["margin"] > 0 and not net["chain"] and 0 <= layer <= len(net["cat"])
    out = {k: v for k, v in net.items() if k != "_kernel_layers"}
    if layer == len(net["cat"]):
        hw, hb = net["heads"]["main"]
        out["heads"] = {"main": (hw * (1.0 + E.REMAINDER), hb)}
    else:
        out["cat_w"] = [w * (1.0 + E.REMAINDER) if l == layer else w for l, w in enumerate(net["cat_w"])]
    out["remainder"] = layer
    return out


# ---- the reference --------------------------------------------------------------------------------------------------
def fold64(net):
    """The three affine branches composed with cat_layers.0 in float64: (F [C0, 252], fb [C0]) on cat[e_o, e_d, e_x]."""
    HL, w0 = net["hidden"][-1], net["cat_w"][0]
    F, fb = w0[:, 3 * HL:].copy(), net["cat_b"][0].copy()
    at = 0
    for b in range(3):
        dim = BRANCH_DIM[b]
        A, c = np.eye(dim), np.zeros(dim)                 # h = A e + c, starting from h = e
        for w, bias in zip(net["branch_w"][b], net["branch_b"][b]):
            nh = A.shape[0]
            A, c = w[:, :nh] @ A + w[:, nh:], w[:, :nh] @ c + bias
        wb = w0[:, b * HL:(b + 1) * HL]
        F[:, at:at + dim] += wb @ A
        fb += wb @ c
        at += dim
    return F, fb


def kernel_layers(net):
    """The trunk as the kernels run it: [(weights on the 12 identity columns / the units before, bias)], layer 0 folded."""
    if "_kernel_layers" not in net:
        F, fb = fold64(net)
        net["_kernel_layers"] = [(F[:, ID_COLS], fb)] + [(w, b) for w, b in zip(net["cat_w"][1:], net["cat_b"][1:])]
    return list(net["_kernel_layers"])


def embed_identity(x12):
    """[R, 252] with the identity columns filled and zeros where the sines and cosines belong (their weights are zero)."""
    e = np.zeros((len(x12), EMB))
    e[:, ID_COLS] = x12
    return e


def literal_pre0(net, x12):
    """cat_layers.0's pre-activation through the literal chain: the branches layer by layer, then cat[h_o, h_d, h_x, e]."""
    e = embed_identity(x12)
    hs, at = [], 0
    for b in range(3):
        eb = e[:, at:at + BRANCH_DIM[b]]
        h = eb
        for w, bias in zip(net["branch_w"][b], net["branch_b"][b]):
            h = np.concatenate([h, eb], axis=1) @ w.T + bias
        hs.append(h)
        at += BRANCH_DIM[b]
    return np.concatenate(hs + [e], axis=1) @ net["cat_w"][0].T + net["cat_b"][0]


def trunk(net, dtype, x12, layers=None, act=None, keep=False, resume=None):
    """The last trunk layer's activations on rows x12 under the operand type's rules, in float64.  layers: the kernel layers
    to use instead of the network's (a mutant); act(l, pre, rule): the activation instead of `leaky`.  With keep: the list of
    (input, pre-activation, output) per layer as well.  resume = (l, a): start at layer l on its input a."""
    layers = kernel_layers(net) if layers is None else layers
    rules = layer_rules(dtype, len(layers))
    a, seen = np.asarray(x12, dtype=np.float64), []
    first = 0
    if resume is not None:
        first, a = resume
    for l, (w, b) in enumerate(layers):
        if l < first:
            continue
        with np.errstate(invalid="ignore", over="ignore"):        # (a mutant may overflow fp16 and go on with inf and NaN)
            pre = a @ w.T + b
            out = leaky(pre, rules[l]) if act is None else act(l, pre, rules[l])
        seen.append((a, pre, out))
        a = out
    return (a, seen) if keep else a


def head_sum(net, head, a):
    hw, hb = net["heads"][head]
    with np.errstate(invalid="ignore"):
        return np.where(hw[0] != 0, a * hw[0], 0.0).sum(axis=1) + hb[0]      # (an unread chain unit may hold anything)


def depth(v, near, far):
    """z = near (1 - s) + far s, s = 1 / (1 + exp(-v)), in float64."""
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-np.asarray(v, dtype=np.float64)))
    return near * (1.0 - s) + far * s


def gate(near, far):
    """8 U max(|near|, |far|): derived in the module docstring."""
    return 8 * U * max(abs(near), abs(far))


def reference(net, head, dtype, x12, near, far, **mutant):
    return depth(head_sum(net, head, trunk(net, dtype, x12, **mutant)), near, far)


# ---- the conditions -------------------------------------------------------------------------------------------------
def check_d1(net):
    """Every trunk and head weight and bias, and every entry of the folded front, is a bf16 and an f16 number."""
    assert net["remainder"] is None and not net["margin"]
    for l, (w, b) in enumerate(kernel_layers(net)):
        assert E.fits16(w).all() and E.fits16(b).all(), f"D1: layer {l}"
    F, fb = fold64(net)
    assert E.fits16(F).all() and E.fits16(fb).all(), "D1: the folded front"
    for w, b in zip(net["cat_w"], net["cat_b"]):
        assert E.fits16(w).all() and E.fits16(b).all(), "D1: the literal trunk"
    for name, (hw, hb) in net["heads"].items():
        assert E.fits16(hw).all() and E.fits16(hb).all(), f"D1: head {name}"


def check_d2(net):
    """Layer 0 reads the 12 identity columns alone, each of them directly and through its branch; the branches read no other."""
    F, _ = fold64(net)
    rest = np.setdiff1d(np.arange(EMB), ID_COLS)
    assert not F[:, rest].any() and F[:, ID_COLS].any(axis=0).all(), "D2: the folded front"
    HL, w0 = net["hidden"][-1], net["cat_w"][0]
    assert not w0[:, 3 * HL + rest].any() and w0[:, 3 * HL + ID_COLS].any(axis=0).all(), "D2: the direct columns"
    assert all(w0[:, b * HL:(b + 1) * HL].any() for b in range(3)), "D2: a branch is not read"
    for b in range(3):
        rest_b = np.setdiff1d(np.arange(BRANCH_DIM[b]), BRANCH_ID[b])
        for i, w in enumerate(net["branch_w"][b]):
            nh = w.shape[1] - BRANCH_DIM[b]
            assert not w[:, nh + rest_b].any() and (i > 0 or not w[:, rest_b].any()), f"D2: branch {b} layer {i} reads a trig column"


def chain_units(net, l):
    return sorted(units[l] for units in net["chain"] if l in units)


def _exact_rows(name, w, b, inp, do_split, special):
    """C3 of exact_field on the rows that are no chain units and the columns they read, and on every sign unit by itself; a
    relay's single product, and with do_split its two, must be fp32 numbers as they stand."""
    rows = np.array([r for r in range(w.shape[0]) if r not in special])
    worst = 0.0
    if len(rows):
        cols = np.flatnonzero(w[rows].any(axis=0))
        worst = E._c3_layer(name, w[rows][:, cols], b[rows], inp[:, cols], do_split)
    for r in special:
        k = np.flatnonzero(w[r])
        if len(k) != 1:                                   # a sign unit: an exact sum of its own quantum
            worst = max(worst, E._c3_layer(name, w[[r]][:, k], b[[r]], inp[:, k], do_split))
            continue
        parts = E.split(inp[:, k[0]]) if do_split else (inp[:, k[0]],)
        acc = b[r]
        for p in parts:
            acc = acc + w[r, k[0]] * p
            assert E.is_f32(acc), f"D3: {name}: chain unit {r} is no fp32 number"
    return worst


def check_d3(net, dtype, heads=None):
    """In every layer, on every pool ray and for the activations this operand type forms, every partial sum in any order is
    an fp32 number; so are the literal chain's (the fp32 oracle runs it).  Nothing but a chain unit is negative before its
    activation, and an ordinary unit's activation is what went in.  Returns the largest C3 ratio."""
    x12 = pool()["x12"]
    layers = kernel_layers(net)
    rules = layer_rules(dtype, len(layers))
    a, seen = trunk(net, dtype, x12, keep=True)
    worst = 0.0
    for l, ((w, b), (inp, pre, out)) in enumerate(zip(layers, seen)):
        special = chain_units(net, l)
        split = l > 0 and rules[l - 1] == "x3" or l == 0 and rules[0] in ("x3", "x3hi")
        worst = max(worst, _exact_rows(f"layer {l} ({dtype})", w, b, inp, split, special))
        ordn = net["ordinary"][l]
        assert (pre[:, ordn] >= 0).all(), f"D3: an ordinary unit of layer {l} is negative ({dtype})"
        if rules[l] != "f16" and rules[l] != "x3hi" or net["remainder"] is None:
            assert (out[:, ordn] == pre[:, ordn]).all(), f"D3: layer {l} rounds an ordinary unit ({dtype})"
        assert E.is_f32(pre), f"D3: layer {l} ({dtype})"
    for name in (heads or net["heads"]):
        hw, hb = net["heads"][name]
        special = [0] if name != "main" else []
        split = rules[-1] == "x3"
        worst = max(worst, _exact_rows(f"head {name} ({dtype})", hw, hb, a, split, special))
    if dtype == "f32":                                   # the literal chain: the branches and cat_layers.0 on what they read
        e = embed_identity(x12)
        hs, at = [], 0
        for bi in range(3):
            eb = e[:, at:at + BRANCH_DIM[bi]]
            h = eb
            for i, (w, bias) in enumerate(zip(net["branch_w"][bi], net["branch_b"][bi])):
                inp = np.concatenate([h, eb], axis=1)
                _exact_rows(f"branch {bi} layer {i}", w, bias, inp, False, [])
                h = inp @ w.T + bias
            hs.append(h)
            at += BRANCH_DIM[bi]
        inp = np.concatenate(hs + [e], axis=1)
        _exact_rows("cat_layers.0", net["cat_w"][0], net["cat_b"][0], inp, False, chain_units(net, 0))
        assert (inp @ net["cat_w"][0].T + net["cat_b"][0] == seen[0][1]).all(), "the fold is not the literal chain"
    return worst


def check_d4(net):
    """Every ordinary unit is positive on at least 10 % of the pool and zero somewhere; neighbouring 16-row blocks of biases
    differ; every chain unit takes both signs."""
    _, seen = trunk(net, "f32", pool()["x12"], keep=True)
    for l, ((w, b), (_, pre, _)) in enumerate(zip(kernel_layers(net), seen)):
        ordn = net["ordinary"][l]
        assert ((pre[:, ordn] > 0).mean(axis=0) >= 0.10).all(), f"D4: a unit of layer {l} is positive on less than 10 % of the pool"
        assert (pre[:, ordn] == net["margin"]).any(axis=0).all(), f"D4: a unit of layer {l} never reaches its least value"
        blocks = [tuple(b[k:k + 16]) for k in range(0, len(b), 16)]
        assert all(x != y for x, y in zip(blocks, blocks[1:]) if len(x) == len(y)), f"D4: layer {l}: equal neighbouring bias blocks"
        for u in chain_units(net, l):
            assert (pre[:, u] < 0).mean() >= 0.10 and (pre[:, u] > 0).mean() >= 0.10, f"D4: chain unit {u} of layer {l}"


def input_blocks(net, l):
    """The 32-column blocks of a kernel layer's input as indices into its columns (layer 0: the 12 identity columns by the
    K-block of the embedding they lie in: o, d, x)."""
    if l == 0:
        return [np.arange(0, 3), np.arange(3, 6), np.arange(6, 12)]
    K = net["cat"][l - 1]
    return [np.arange(k, min(k + 32, K)) for k in range(0, K, 32)]


def block_mutants(net):
    """Every (what, layer, kernel layers, head weights) with one 32-column input block or one 16-row output block of one
    layer, the head included, zeroed."""
    layers = kernel_layers(net)
    hw, hb = net["heads"]["main"]
    for l, (w, b) in enumerate(layers):
        for cols in input_blocks(net, l):
            w2 = w.copy()
            w2[:, cols] = 0
            yield f"input block {cols[0]} of layer {l}", l, layers[:l] + [(w2, b)] + layers[l + 1:], hw
        for lo, hi in _blocks(w.shape[0]):
            w2, b2 = w.copy(), b.copy()
            w2[lo:hi], b2[lo:hi] = 0, 0
            yield f"output block {lo} of layer {l}", l, layers[:l] + [(w2, b2)] + layers[l + 1:], hw
    for cols in input_blocks(net, len(layers)):
        h2 = hw.copy()
        h2[:, cols] = 0
        yield f"input block {cols[0]} of the head", len(layers) - 1, layers, h2


def swapped_bias_mutants(net):
    """(what, layer, kernel layers) with the biases of two neighbouring 16-row blocks of one layer exchanged."""
    layers = kernel_layers(net)
    for l, (w, b) in enumerate(layers):
        for (lo, hi), (lo2, hi2) in zip(_blocks(len(b)), _blocks(len(b))[1:]):
            if hi2 - lo2 == 16:
                b2 = b.copy()
                b2[lo:hi], b2[lo2:hi2] = b[lo2:hi2], b[lo:hi]
                yield f"bias blocks {lo}, {lo2} of layer {l}", l, layers[:l] + [(w, b2)] + layers[l + 1:]


def _z_main(net, dtype, a, hw, near_far):
    _, hb = net["heads"]["main"]
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(hw[0] != 0, a * hw[0], 0.0).sum(axis=1) + hb[0]
    return [depth(v, near, far) for near, far in near_far]


def check_d5(net, dtype="f32", near_far=NEAR_FAR):
    """Zeroing any block, or exchanging two neighbouring blocks of biases, changes z through the main head on some pool ray
    by more than the gate (twice the gate: the kernel's own rounding may take one)."""
    x12 = pool()["x12"]
    _, seen = trunk(net, dtype, x12, keep=True)
    hw0 = net["heads"]["main"][0]
    base = _z_main(net, dtype, seen[-1][2], hw0, near_far)
    mutants = list(block_mutants(net)) + [(what, l, layers, hw0) for what, l, layers in swapped_bias_mutants(net)]
    for what, l, layers, hw in mutants:
        a = trunk(net, dtype, x12, layers=layers, resume=(l, seen[l][0]))
        for z, z0, (near, far) in zip(_z_main(net, dtype, a, hw, near_far), base, near_far):
            with np.errstate(invalid="ignore"):        # (a mutant may overflow fp16: its NaN is a change like any other)
                same = bool((np.abs(z - z0) <= 2 * gate(near, far)).all())
            assert not same, f"D5: {what} does not reach z ({dtype}, near {near}, far {far})"


def head_quantum(net, head, dtype, a):
    """What one wrong term moves the head's sum by at least: the quantum of the main head's terms; for a chain head, on each
    ray, 2^-13 of the sum -- the two slopes differ by more (2^-12.2), and a lost negative branch by all of it."""
    hw, hb = net["heads"][head]
    if head == "main":
        cols = np.flatnonzero(hw[0])
        return min(E.quantum(hw[0, cols]) * E.quantum(a[:, cols]), E.quantum(hb))
    return np.abs(head_sum(net, head, a)) * 2.0 ** -13


def check_d6(net, dtype, near, far):
    """One quantum of the head's sum moves z by at least 16 gates: (far - near) s (1 - s) q >= 16 gate, for the main head on
    every pool ray; a chain is read at two scales, and under one of them on at least a quarter of the pool ."""
    a = trunk(net, dtype, pool()["x12"])

    def move(head):
        with np.errstate(over="ignore"):
            s = 1.0 / (1.0 + np.exp(-head_sum(net, head, a)))
        return (far - near) * s * (1 - s) * head_quantum(net, head, dtype, a)

    m = move("main")
    assert (m >= 16 * gate(near, far)).all(), f"D6: main ({dtype}): {float(m.min()) / gate(near, far)} gates"
    for c in range(len(net["chain"])):
        m = np.maximum(move(f"chain{c}"), move(f"chain{c}s"))
        assert (m >= 16 * gate(near, far)).mean() >= 0.25, f"D6: chain {c} ({dtype}) moves z on too few rays"


def check_chain_range(net, dtype):
    """Every chain value is finite and below 65504, and where an f16 engine holds it, it -- of a split value the hi part -- is
    zero or a normal f16 number (numpy's float16).  Returns the share of nonzero lo parts that are subnormal f16 numbers: a
    chain's values differ by the slope, a factor of a hundred, and by their mantissas' last bits, so some remainders fall
    below 2^-14; the split engine is built to carry those (ns_mlp_engine.h: "below ~1e-4 the lo half goes subnormal")."""
    rules = layer_rules(dtype, len(net["cat"]))
    _, seen = trunk(net, dtype, pool()["x12"], keep=True)
    tiny = float(np.finfo(np.float16).tiny)
    sub = total = 0
    for l in range(len(net["cat"])):
        for u in chain_units(net, l):
            out = seen[l][2][:, u]
            assert np.isfinite(out).all() and np.abs(out).max() < 65504, f"chain unit {u} of layer {l} ({dtype})"
            if rules[l] in ("f16", "x3", "x3hi"):
                hi = f16r(out)
                lo = f16r(out - hi)
                assert ((hi == 0) | (np.abs(hi) >= tiny)).all(), f"chain unit {u} of layer {l} ({dtype}): a subnormal value"
                assert (hi + lo == out).all(), f"chain unit {u} of layer {l} ({dtype}): not hi + lo"
                sub += int(((lo != 0) & (np.abs(lo) < tiny)).sum())
                total += int((lo != 0).sum())
    return sub / max(total, 1)


def chain_finals(net, dtype, seen, mutant=None):
    """The last layer's activation of every chain, [P, chains], from the sign units' sums in `seen` (a full `trunk` run) along
    the single-term rows: what `trunk` computes there, without the ordinary units, which no mutant below touches (they are
    never negative).  mutant = (kind, layer, first row, end): in those rows of that layer the negative branch is replaced by
    zero ("zero") or takes the other engine's slope ("slope": 0.01f where 0x211f belongs and the other way round)."""
    rules = layer_rules(dtype, len(net["cat"]))
    out = np.zeros((len(seen[0][0]), len(net["chain"])))
    for c, units in enumerate(net["chain"]):
        start = min(units)
        pre = seen[start][1][:, units[start]]
        for l in range(start, len(net["cat"])):
            if l > start:
                pre = net["cat_w"][l][units[l], units[l - 1]] * a
            a = leaky(pre, rules[l])
            if mutant is not None and mutant[1] == l and mutant[2] <= units[l] < mutant[3]:
                a = np.where(pre < 0, 0.0, a) if mutant[0] == "zero" else leaky(pre, rules[l], slope32=SLOPE16, slope16=SLOPE32)
        out[:, c] = a
    return out


def chain_head_sums(net, finals):
    """name -> the head's sum, for every chain head."""
    last = len(net["cat"]) - 1
    return {f"chain{c}{tag}": net["heads"][f"chain{c}{tag}"][0][0, units[last]] * finals[:, c]
            for c, units in enumerate(net["chain"]) for tag in ("", "s")}


def sub_block_mutants(net, dtype, kind):
    """(kind, layer, first row, end) for every 16-row sub-block of every trunk layer whose rule can show the mutant: a slope
    2^-12 off is below the 16-bit rounding of bf16 operands, and of the plain layers behind f16m's split ones."""
    rules = layer_rules(dtype, len(net["cat"]))
    for l, width in enumerate(net["cat"]):
        if kind == "slope" and (rules[l] == "bf16" or dtype == "f16m" and rules[l] != "f16"):
            continue
        for lo, hi in _blocks(width):
            yield kind, l, lo, hi


def check_chains_cover(net, dtype, kind, near_far=NEAR_FAR):
    """Across the head variants, every 16-row sub-block of every trunk layer takes its negative branch on a value that
    reaches z: the mutant of `sub_block_mutants` there moves some head's z by more than twice the gate."""
    _, seen = trunk(net, dtype, pool()["x12"], keep=True)
    finals = chain_finals(net, dtype, seen)
    last = len(net["cat"]) - 1
    assert all((finals[:, c] == seen[-1][2][:, units[last]]).all() for c, units in enumerate(net["chain"]))
    base = chain_head_sums(net, finals)
    for mutant in sub_block_mutants(net, dtype, kind):
        got = chain_head_sums(net, chain_finals(net, dtype, seen, mutant))
        for near, far in near_far:
            moved = max(np.abs(depth(got[h], near, far) - depth(base[h], near, far)).max() for h in base)
            assert moved > 2 * gate(near, far), f"sub-block {mutant[2]} of layer {mutant[1]} ({dtype}, {kind}): {moved / gate(near, far)} gates"


def check_remainders(net, dtype):
    """The remainder family: fp32 weights that split into two f16 numbers, W_lo x_lo identically zero on the split layers,
    the layer with the remainders sees W_lo, the split layers behind it x_lo, every activation handed on is hi + lo (or hi,
    where the rule says so) exactly, and D3 holds over the three products.  Returns the largest C3 ratio."""
    layer = net["remainder"]
    assert layer is not None
    layers = kernel_layers(net) + [net["heads"]["main"]]
    rules = layer_rules(dtype, len(layers) - 1)
    _, seen = trunk(net, dtype, pool()["x12"], keep=True)
    inputs = [s[0] for s in seen] + [seen[-1][2]]
    for l, ((w, b), inp) in enumerate(zip(layers, inputs)):
        assert E.is_f32(w) and E.is_f32(b), f"layer {l}: not fp32"
        wh, wl = E.split(w)
        assert (wh + wl == w).all(), f"layer {l}: a weight is not hi + lo"
        split_in = l == 0 or rules[l - 1] == "x3"           # this layer multiplies (hi, lo) inputs
        if dtype != "f32" and split_in:
            xh, xl = E.split(inp)
            assert (xh + xl == inp).all(), f"layer {l}: an activation is not hi + lo"
            assert not wl.any() or not xl.any(), f"layer {l}: W_lo x_lo is not identically zero"
            assert bool(xl.any()) == (l > layer), f"layer {l}: x_lo"
        assert bool(wl.any()) == (l == layer), f"layer {l}: W_lo"
    return check_d3(net, dtype, heads=["main"])


# ---- what the tests feed and expect ---------------------------------------------------------------------------------
_cache = {}


def network(name):
    if name not in _cache:
        hidden, cat, seed = NETWORKS[name]
        _cache[name] = make_exact_depthnet(hidden, cat, seed)
    return _cache[name]


def remainder_base(name):
    key = (name, "base")
    if key not in _cache:
        hidden, cat, seed = NETWORKS[name]
        _cache[key] = make_exact_depthnet(hidden, cat, seed + 100, chains=False, margin=MARGIN)
    return _cache[key]


def remainder_network(name, layer):
    key = (name, layer)
    if key not in _cache:
        _cache[key] = add_remainders(remainder_base(name), layer)
    return _cache[key]


def tensors(net, head):
    """(weights, biases) as the fp32 torch tensors ops.pack_depthnet takes: origin, direction and intersection layers,
    cat_layers.{0, 2, ..}, to_depth.0."""
    ws = [w for b in range(3) for w in net["branch_w"][b]] + list(net["cat_w"]) + [net["heads"][head][0]]
    bs = [v for b in range(3) for v in net["branch_b"][b]] + list(net["cat_b"]) + [net["heads"][head][1]]
    assert all(E.is_f32(a) for a in ws + bs)
    return [torch.from_numpy(w).float() for w in ws], [torch.from_numpy(b).float() for b in bs]


def state_dict(net, head):
    """The reference's state dict (depth_net.py:13-107) of a network with one of its heads, fp32."""
    ws, bs = tensors(net, head)
    n, m = len(net["hidden"]), len(net["cat"])
    names = ([f"origin_layers.{i}" for i in range(n)] + [f"direction_layers.{i}" for i in range(n)]
             + [f"intersection_layers.{i}" for i in range(n)] + [f"cat_layers.{2 * i}" for i in range(m)] + ["to_depth.0"])
    p = {}
    for k, w, b in zip(names, ws, bs):
        p[k + ".weight"], p[k + ".bias"] = w, b
    return p


def worst_ratio(z, z64, near, far):
    """(max |z - z64| / gate, its ray) over rays; a NaN on either side where the other has none counts as infinite."""
    z, z64 = np.asarray(z, dtype=np.float64).reshape(-1), np.asarray(z64, dtype=np.float64).reshape(-1)
    nan = np.isnan(z) | np.isnan(z64)
    ratio = np.where(nan, np.where(np.isnan(z) & np.isnan(z64), 0.0, np.inf), np.abs(np.where(nan, 0.0, z - z64)) / gate(near, far))
    r = int(np.argmax(ratio))
    return float(ratio[r]), r


# ---- part B: the sines and cosines, column by column ----------------------------------------------------------------
PROBE_GROUPS = 42                             # group g reads the columns g, g + 42, .., g + 210: every column lies in one group
PROBE_HEAD = (1.0, -0.5, 0.5, -1.0, -0.5, 1.0)         # from {+-1, +-1/2}: six weights cannot all differ, neighbours do
PROBE_DTYPES = ("f32", "bf16", "f16", "f16x3")
PROBE_NARROW_DTYPES = ("f32", "f16")          # one operand type of each engine at the 128-wide trunk
PROBE_TAU = {"f32": 8 * U, "f16x3": 8 * U, "bf16": 2.0 ** -8 + 2.0 ** -18, "f16": 2.0 ** -11 + 2.0 ** -18}
PROBE_ROUNDED_DTYPES = ("bf16", "f16")        # the operand types that round an identity column: see the gate's derivation
PROBE_RADIUS = 2.0


def probe_columns(g):
    return g + PROBE_GROUPS * np.arange(6)


def probe_units(which):
    """The embedding columns a probe trunk holds, one unit each: all 252 ("wide"), or those of the groups 7 n .. 7 n + 6
    (which = n, 0 .. 5: 42 units, a 128-wide trunk)."""
    if which == "wide":
        return np.arange(EMB)
    return np.sort(np.concatenate([probe_columns(g) for g in range(7 * which, 7 * which + 7)]))


def probe_sign(j):
    """-1 for every fifth column from level 2 on, whose sines and cosines take both signs on the rays (a unit that is negative
    on every ray would pass through the slope alone, at a hundredth of the sensitivity)."""
    at, n = (0, 3) if j < 63 else (63, 3) if j < 126 else (126, 6)
    return -1.0 if j % 5 == 0 and j - at >= n * 5 else 1.0


def make_probe(which):
    """One branch layer and one trunk layer of one-hot rows: hidden unit k is column units[k] of the embedding, times +-1.  The
    columns with an odd index within their embedding go through their branch (a unit that copies the column, from the first
    or the second half of cat[e, e] in turn) and so through the fold's product; the others through the direct skip.  Returns
    the weight and bias lists without the head, and the units."""
    units = probe_units(which)
    H = 64
    at = np.array([0, 63, 126, 252])
    bw = [np.zeros((H, 2 * dim)) for dim in BRANCH_DIM]
    w0 = np.zeros((len(units), 3 * H + EMB))
    used = [0, 0, 0]
    for k, j in enumerate(units):
        b = int(np.searchsorted(at, j, side="right") - 1)
        local = j - at[b]
        if local % 2:
            u = used[b]
            used[b] += 1
            bw[b][u, local + (BRANCH_DIM[b] if u % 2 else 0)] = 1.0
            w0[k, b * H + u] = probe_sign(j)
        else:
            w0[k, 3 * H + j] = probe_sign(j)
    assert max(used) <= H
    return bw + [w0], [np.zeros(H)] * 3 + [np.zeros(len(units))], units


def probe_tensors(which, g):
    """(weights, biases, hidden_sizes, cat_hidden_sizes) of the probe network whose head reads group g."""
    ws, bs, units = make_probe(which)
    hw = np.zeros((1, len(units)))
    for c, wgt in zip(probe_columns(g), PROBE_HEAD):
        hw[0, np.flatnonzero(units == c)[0]] = wgt
    ws, bs = ws + [hw], bs + [np.zeros(1)]
    return [torch.from_numpy(w).float() for w in ws], [torch.from_numpy(b).float() for b in bs], [64], [len(units)]


def probe_rays():
    """(o, d) as float32: 200 rays of the production geometry (|o| about 4, aimed near the centre of the radius-2 sphere), then
    rays with components that are exactly 0, negative, 2^-20 and of magnitude 8 (at level 9 an argument above 4000 rad), and
    three that miss."""
    rng = np.random.default_rng(77)
    o = rng.standard_normal((200, 3))
    o = 4.03 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = -o + 0.3 * rng.standard_normal((200, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    t = 2.0 ** -20
    so = [[0, 0, 8], [8, 0, 0], [-8, t, 0], [0, -8, t], [t, t, -8], [0, 0, 8], [-7.5, 0, t], [8, 8, 0], [0, 3, 0], [-8, -8, -8]]
    sd = [[0, 0, -1], [-1, t, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -8], [8, t, 0], [1, 0, 0], [0, 0, 1], [-1, 0, 0]]
    return (np.concatenate([o, so]).astype(np.float32), np.concatenate([d, sd]).astype(np.float32))


def kernel_x6(o, d, radius):
    """The six intersection coordinates as the kernels form them in fp32 (ns_depthnet.hip:51-58): every operation rounded to
    fp32 in the kernel's order, |o|^2 through its two fused multiply-adds."""
    o, d = np.asarray(o, dtype=np.float32), np.asarray(d, dtype=np.float32)
    f, r = np.float32, np.float32(radius)
    b = f(2) * ((d[:, 0] * o[:, 0] + d[:, 1] * o[:, 1]) + d[:, 2] * o[:, 2])
    o64 = o.astype(np.float64)
    inner = (o64[:, 1] * o64[:, 1] + (o[:, 0] * o[:, 0]).astype(np.float64)).astype(np.float32)
    on2 = (o64[:, 2] * o64[:, 2] + inner.astype(np.float64)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        on = np.sqrt(on2)
        c = on * on - r * r
        aa = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        sq = np.sqrt(b * b - f(4) * aa * c)
        t0, t1 = (-b - sq) / (f(2) * aa), (-b + sq) / (f(2) * aa)
    x = np.concatenate([o + t0[:, None] * d, o + t1[:, None] * d], axis=1)
    assert x.dtype == np.float32
    return x


def embedding64(o, d, x6):
    """cat[gamma(o), gamma(d), gamma(x6)] in float64 of fp32 inputs (run_nerf_helpers.py:15-63: x, then sin and cos of 2^l x)."""
    def gamma(x):
        x = np.asarray(x, dtype=np.float64)
        parts = [x]
        for l in range(10):
            parts += [np.sin(x * 2.0 ** l), np.cos(x * 2.0 ** l)]
        return np.concatenate(parts, axis=1)
    return np.concatenate([gamma(o), gamma(d), gamma(x6)], axis=1)


def probe_reference(e, g, dtype):
    """(z64, gate) of the probe of group g on embedding rows e: the float64 chain with the operand type's slope constant and
    no other rounding; the gate (1/4) sum_j |w_j| tau_t + 4 U, where for bf16 and f16 an identity column's tau_t is taken
    max(1, |e_j|) times: their rounding of the column is relative (derived in the module docstring)."""
    cols = probe_columns(g)
    u = e[:, cols] * np.array([probe_sign(j) for j in cols])
    slope = SLOPE16 if dtype == "f16" else SLOPE32
    with np.errstate(invalid="ignore"):
        a = np.where(u > 0, u, slope * u)
    w = np.array(PROBE_HEAD)
    z = depth(a @ w, 0.0, 1.0)
    size = np.ones(e[:, cols].shape)
    if dtype in PROBE_ROUNDED_DTYPES:
        identity = np.isin(cols, ID_COLS)
        size[:, identity] = np.maximum(np.abs(np.nan_to_num(e[:, cols[identity]])), 1.0)
    allow = 0.25 * (size @ np.abs(w)) * PROBE_TAU[dtype] + 4 * U
    return z, allow


def probe_worst(z, z64, allow):
    """(max |z - z64| / gate, its ray); a NaN on one side alone counts as infinite."""
    z, z64 = np.asarray(z, dtype=np.float64).reshape(-1), np.asarray(z64, dtype=np.float64).reshape(-1)
    nan = np.isnan(z) | np.isnan(z64)
    ratio = np.where(nan, np.where(np.isnan(z) & np.isnan(z64), 0.0, np.inf), np.abs(np.where(nan, 0.0, z - z64)) / allow)
    r = int(np.argmax(ratio))
    return float(ratio[r]), r
