"""The training step's small kernels (csrc/ns_train.hip: ns_act_forward, ns_act_backward, ns_colsum, ns_posenc_backward,
ns_points_backward, ns_adam_step, ns_adam_step_dev, ns_adam_step_multi_dev; csrc/ns_rays.hip: ns_posenc, ns_points_along_rays)
entry by entry against float64: seeded inputs, the float64 reference on the fp32 inputs, an fp32 oracle that mirrors the kernel's
arithmetic in numpy float32, the error model with its comparator, and fp32 mutants of the oracle.

Shared by tests/test_gpu_train_kernels.py (the HIP kernels) and tests/test_train_kernels_host.py (on the CPU: the generators meet
their conditions, the reference agrees with torch float64 autograd and a float64 torch.optim.Adam, the fp32 oracle is accepted on
every entry and every mutant below is rejected, so the bounds are tight enough to mean something).  Nothing here calls the
library.

A comparator returns Verdict(rejected, worst): the flat indices of the rejected entries -- none is forgiven, NaN must sit in the
same entries as in the reference, an infinite reference value must be met exactly -- and the worst |err| / bound over the others.

U = 2^-24 (half an ulp at 1).  The library is built with -ffp-contract=off: no multiply is fused with an add, so a statement of
the kernel is the same sequence of IEEE operations in numpy float32.  Round to nearest gives |fl(x) - x| <= U / (1 + U) |x|,
which is what lets k roundings in a row be bounded by k U with no second-order term for the k <= 3 used below.

Activations (act 0 none, 1 relu, 2 leaky 0.01f, 3 sigmoid).
    forward 0, 1, 2 and every backward are comparisons, selections and at most three IEEE multiplies / subtractions: bit for
    bit against the oracle (relu: v < 0 ? 0 : v, so -0 stays -0 and NaN stays NaN; leaky: v > 0 ? v : 0.01f v; backward from
    the activation OUTPUT y: relu' = y > 0, leaky' = y > 0 ? 1 : 0.01f, sigmoid' = y (1 - y); dy = dy * act').
    sigmoid forward 1 / (1 + expf(-v)) against float64:  |err| <= 6 U s + 2^-128 + 2^-149,  s = sigmoid(v).
      e = expf(-v) within 2 ulp is |de| <= 4 U e (+ 2^-149 where e is denormal), and d s / d e = -s^2 with s^2 e = s (1 - s) <= s:
      4 U s; the add and the IEEE divide round once each: 2 U s; a result in the denormal range rounds to a 2^-149 grid.
      The floor: expf(-v) overflows to +inf for -v > log(FLT_MAX) = 88.7228, and the kernel returns 1 / inf = 0 where the true
      value is anything below 1 / FLT_MAX = 2^-128.  (A floor of one denormal step alone, 2^-149, would not cover the stretch
      -103.3 < v < -88.72 of the kernel's own arithmetic; 2^-128 is the derived figure, a quarter of the 2^-126 in
      gemm_tile_reference.sigmoid_bound.)
    NaN in gives NaN out under every forward activation.
    Inputs: normal draws scaled by one of {1e-3, 1, 30, 200}; planted at the front (and again at the back, behind whatever a
    capped grid covers in its first pass): -88, NaN, +-0, +-inf, 88, +-104, +-2^-126 (n = 1 holds the -88 alone: both
    forward mutants differ there).

Column sums out[j] = sum_i X[i ld + j] (32 row lanes add rows rl, rl + 32, .. in order, then the 32 partials are added in order).
    (a) integers |x| <= 64, M <= 2^17: every partial sum is an integer below 2^23, exact in any order: bit for bit.
    (b) floats: |err| <= (ceil(M / 32) + 31) U sum_i |x_ij|: ceil(M / 32) - 1 roundings in a lane (the first add, to 0, is exact),
        31 in the final pass, two spare for the second-order terms.
    M = 0 gives zeros.  The pad columns j >= N of a row (ld > N) hold 1e30: a kernel that read one would be far off.
    The last row holds no zero (integers) or nothing below 1 in magnitude (floats), so dropping it shows in every column.

Positional encoding out = [x, sin(x 2^0), cos(x 2^0), .., sin(x 2^(L-1)), cos(x 2^(L-1))], blocks of d columns.  The argument
x 2^l is exact in fp32 (a power-of-two scale), so the reference forms it exactly and takes sin and cos in float64.
    forward: the identity block bit for bit; |err| <= TRIG = 4 U per trig entry (2 ulp at 1, the figure published for sinf and
      cosf over the full range).
    backward dx = g_0 + sum_l 2^l (cos_l g_s - sin_l g_c), g_s and g_c the gradients of band l's sin and cos entries:
      |err| <= (TRIG / U + 2) U sum_l 2^l (|g_s| + |g_c|) + (L + 2) U (|g_0| + sum_l 2^l (|cos_l g_s| + |sin_l g_c|))
      per band: the trig error TRIG |g|, one rounding per product (U |trig g| <= U |g|), one for the difference
      (U (|cos g_s| + |sin g_c|) <= U (|g_s| + |g_c|)), the scale by 2^l exact; then L roundings of the running sum, each at most
      U times the sum of the magnitudes, two spare.  At L = 10 and unit gradients that is about 6e-4.
    x uniform in [-2, 2]; planted 0, +-fp32(pi / 2) / 2^(L-1) (the top band at a zero of cos) and +-4.

Points pts = o + d z, dz = sum_c dpts_c d_c (z in [2, 6], the rest normal).
    forward |err| <= U (|d z| + |pts|): one rounding of the product, one of the sum (a fused multiply-add has only the second).
    backward (a + b) + c of three products: |err| <= 3 U sum_c |dpts_c d_c|.

Adam: m' = b1 m + (1 - b1) g,  v' = b2 v + (1 - b2) g g,  p' = p - (lr / bc1) (m' / (sqrt(v') / sqrt(bc2) + eps)),
bc = 1 - powf(b, t).  The reference takes lr, b1, b2, eps as the fp32 values the kernel receives and t as an integer;
1 - b is exact in fp32 for 0.5 <= b <= 1 (Sterbenz), so the reference uses it as is.
    m', v':  |err| <= 3 U (|b old| + |(1 - b) new|): two roundings on the path of the first term, two (m') or three (v') on the
      second.
    the update D = p' - p, with S = (lr / bc1) / denom and Am = |b1 m| + |(1 - b1) g| from the reference:
      |err| <= 3 U S Am (1 + REL) + REL S |m'| + U |p'|,      REL(t) = 9 U + r(b1, t) + r(b2, t) / 2
      3 U S Am: the error of m' carried through.  REL: v' is a sum of positive terms within 3 U, its square root within 1.5 U,
      then sqrtf, sqrtf(bc2), the quotient, the add of eps, m' / denom, lr / bc1 and the product round once each: 8.5 U, taken
      as 9 U; bc1 enters once and bc2 under a square root.  U |p'|: the rounding of the parameter itself.
      r(b, t) = ulp(b^t) / bc + U: powf taken within 1 ulp (no figure for the device's powf could be confirmed from the
      installed documentation; ns_adam_step evaluates it on the host, the other two entries on the device, and the updates of all
      three stayed inside the bound built on it at every t below), the subtraction from 1 exact while b^t >= 0.5 and one rounding below.  At t = 2 and
      b2 = 0.999f, r / 2 = 1.5e-5; at t = 100000 it is U.
    g = +-10^[-6, 4]; entries 6 mod 8 have g = 0, entries 7 mod 8 g = 0 and v = 0 (the denominator is eps alone); p is normal,
    every other one scaled by 1e-3 so that the parameter's own rounding does not hide the update's error.

Mutants (fp32 variants of the oracle; every one is rejected wherever it differs from the kernel's statement at all -- the
host test runs them at every case and names the cases where one is the identity):
    sigmoid without the negation; leaky slope 0.1.
    column sums with the last row dropped (not at M = 0); column N - 1 not written.
    posenc: sin and cos swapped in band 0; the frequency 2^(l+1) in the top band only (both need L >= 1); the backward without
      its factor 2^l (L >= 2: 2^0 = 1); the backward reading column c + 1 of band 0's sin gradients.
    points: d of ray r + 1 (R >= 2).
    Adam: eps inside the square root; bc2 without its sqrt and step t + 1 (t <= 1000: at t = 100000 both bias corrections
      are 1 in fp32 either way); lr_dev ignored; b1 and b2 swapped; the last table row skipped; elements at index >= 65536 of a
      tensor left unchanged.

Worst |err| / bound over the cases below: the fp32 oracle on the CPU / the HIP kernels on the MI355X.  The bit-for-bit
comparisons (activations but the sigmoid forward, integer column sums, the identity block, multi-tensor against per-tensor Adam,
lr_dev against the scalar) held with no entry rejected.
    sigmoid forward                         0.999 / 0.999   (at v = -88.72393, just below -88.7228: the result is 0, the true
                                                             value just under 2^-128; 0.63 on the CPU outside -104 < v < -88)
    column sums, floats                     0.133 / 0.133
    posenc forward                          0.255 / 0.253   (the device's worst sinf / cosf error: 1.011 U, i.e. within 1 ulp
                                                             at |x 2^l| <= 2048, against the 4 U allowed; at x = -1.8041589,
                                                             band 6)
    posenc backward                         0.339 / 0.313
    points forward / backward               0.996, 0.867 / 0.996, 0.867
    Adam: ns_adam_step, ns_adam_step_dev    0.995 / 0.995   (the update, where U |p'| dominates and |p'| sits just above a
                                                             power of two: half an ulp is then U |p'| itself; m' 0.65, v' 0.95)
          ns_adam_step_multi_dev, 70 rows   - / 0.988
  No kernel needed a rejected entry forgiven or a larger constant than derived above.
"""

from collections import namedtuple

import numpy as np

F32 = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -149
TRIG = 4 * U                     # sinf / cosf: 2 ulp at 1
SIGMOID_FLOOR = 2.0 ** -128 + TINY
POW_ULPS = 1.0                   # powf within 1 ulp
STRIDE_THRESHOLD = 65536         # ns_adam_step_multi_dev: 256 blocks x 256 threads, larger tensors take the grid-stride loop
EW_GRID = 4096 * 256             # the elementwise grid's cap in threads

Verdict = namedtuple("Verdict", "rejected worst")

# ---- the cases of the GPU tests (the host test runs the same) ---------------------------------------------------------------
ACT_SIZES = (1, 255, 256, 257, EW_GRID + 257)
COLSUM_M = (0, 1, 31, 32, 33, 1025)
COLSUM_N = (1, 31, 32, 33, 257)
COLSUM_PAD = (0, 5)                                                 # ld = N, and ld = N + 5: a column slice
POSENC_CASES = ((1, 1, 0), (7, 3, 10), (257, 6, 10), (33, 9, 4))
POSENC_FWD_STRIDE = (116509, 3, 1)                                  # M d (1 + 2 L) = 1048581 > EW_GRID
POSENC_BWD_STRIDE = (349527, 3, 1)                                  # M d = 1048581 > EW_GRID
POINTS_CASES = ((1, 1), (20, 4), (33, 64), (5, 65))
POINTS_FWD_STRIDE = (349527, 1)                                     # R N 3 = 1048581 > EW_GRID
POINTS_BWD_STRIDE = (16385, 64)                                     # R N = 1048640 > EW_GRID
ADAM_SIZES = (1, 255, 257, 65536, 65537, EW_GRID + 257)
ADAM_STEPS = (1, 2, 10, 1000, 100000)
# (n, t): every size, every step count; all step counts at the smallest size with a ragged block and all planted entries
ADAM_CASES = tuple(zip(ADAM_SIZES, (1, 2, 10, 1000, 100000, 2))) + tuple((257, t) for t in ADAM_STEPS if t != 10)
ADAM_TABLE_SIZES = (0, 1, 3, 256, 5100, 65537, 81664)
ADAM_TABLE_ROWS = 70
ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


# ---- comparators ------------------------------------------------------------------------------------------------------------
def compare_bits(got, want):
    """The entries whose fp32 bits differ (a NaN matches any NaN)."""
    got = np.ascontiguousarray(got, dtype=F32).ravel()
    want = np.ascontiguousarray(want, dtype=F32).ravel()
    assert got.shape == want.shape
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return Verdict(np.flatnonzero(~same), 0.0 if bool(same.all()) else float("inf"))


def compare_bound(got, ref, bound):
    """The entries of `got` outside ref +- bound (float64).  NaN must sit where the reference has it and nowhere else, an
    infinite reference value must be met exactly, and an entry with bound 0 exactly."""
    ref = np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape).ravel()
    got, ref = np.asarray(got, dtype=np.float64).ravel(), ref.ravel()
    assert got.shape == ref.shape == bound.shape
    nan_r, nan_g, inf_r = np.isnan(ref), np.isnan(got), np.isinf(ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        finite = ~nan_r & ~inf_r
        bad = (nan_r != nan_g) | (inf_r & (got != ref)) | (finite & ~(err <= bound))
        ratio = np.where(err == 0, 0.0, err / bound)
    ok = finite & ~bad
    return Verdict(np.flatnonzero(bad), float(ratio[ok].max()) if bool(ok.any()) else 0.0)


def merge(*verdicts):
    """One verdict for several outputs of one call: the indices are offset by output (1e9 apart) so that they stay readable."""
    rej = [v.rejected + k * 10 ** 9 for k, v in enumerate(verdicts)]
    return Verdict(np.concatenate(rej) if rej else np.zeros(0, dtype=np.int64), max([v.worst for v in verdicts] + [0.0]))


# ---- activations ------------------------------------------------------------------------------------------------------------
ACT_SCALES = (1e-3, 1.0, 30.0, 200.0)
ACT_PLANTED = np.array([-88.0, np.nan, 0.0, -0.0, np.inf, -np.inf, 88.0, 104.0, -104.0, 2.0 ** -126, -(2.0 ** -126)], dtype=F32)
LEAKY = F32(0.01)


def gen_act(n, seed):
    """Forward inputs: scaled normal draws with ACT_PLANTED at the front (as many as fit) and, from 2 x 11 entries on, at the back."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(F32) * np.array(ACT_SCALES, dtype=F32)[rng.integers(0, len(ACT_SCALES), n)]
    k = min(n, len(ACT_PLANTED))
    x[:k] = ACT_PLANTED[:k]
    if n >= 2 * len(ACT_PLANTED):
        x[-len(ACT_PLANTED):] = ACT_PLANTED
    return x


ACT_Y_PLANTED = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, 0.5, 2.0 ** -126], dtype=F32)


def gen_act_backward(n, seed):
    """(dy, y): y an activation output with a quarter exact zeros, negative values (leaky) and ACT_Y_PLANTED at both ends."""
    rng = np.random.default_rng(seed)
    dy = rng.standard_normal(n).astype(F32)
    y = rng.standard_normal(n).astype(F32)
    y[rng.random(n) < 0.25] = 0.0
    k = min(n, len(ACT_Y_PLANTED))
    y[:k] = ACT_Y_PLANTED[:k]
    if n >= 2 * len(ACT_Y_PLANTED):
        y[-len(ACT_Y_PLANTED):] = ACT_Y_PLANTED
    return dy, y


def act_forward32(x, act, mutant=None):
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        if act == 0:
            return x.copy()
        if act == 1:
            return np.where(x < 0, F32(0), x)
        if act == 2:
            return np.where(x > 0, x, (F32(0.1) if mutant == "leaky_slope" else LEAKY) * x)
        if act == 3:
            e = np.exp(x if mutant == "sigmoid_no_negation" else -x)
            return (F32(1) / (F32(1) + e)).astype(F32)
    raise ValueError(act)


def sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def sigmoid_bound(x):
    return 6 * U * np.nan_to_num(sigmoid64(x), nan=0.0) + SIGMOID_FLOOR


def compare_act_forward(got, x, act):
    if act == 3:
        return compare_bound(got, sigmoid64(x), sigmoid_bound(x))
    return compare_bits(got, act_forward32(x, act))


def act_backward32(dy, y, act, mutant=None):
    dy, y = np.asarray(dy, dtype=F32), np.asarray(y, dtype=F32)
    one = F32(1)
    with np.errstate(over="ignore", invalid="ignore"):
        if act == 0:
            return dy.copy()
        if act == 1:
            return dy * np.where(y > 0, one, F32(0))
        if act == 2:
            return dy * np.where(y > 0, one, F32(0.1) if mutant == "leaky_slope" else LEAKY)
        if act == 3:
            return dy * (y * (one - y))
    raise ValueError(act)


def compare_act_backward(got, dy, y, act):
    return compare_bits(got, act_backward32(dy, y, act))


# ---- column sums ------------------------------------------------------------------------------------------------------------
COLSUM_POISON = F32(1e30)


def gen_colsum(M, N, pad, seed, integers):
    """X [M, N + pad] fp32: integers in [-64, 64] or normal draws over two decades; pad columns hold 1e30; the last row is at
    least 1 in magnitude (no column's bound reaches 1 at these M, so a dropped last row shows in every column)."""
    rng = np.random.default_rng(seed)
    if integers:
        X = rng.integers(-64, 65, (M, N + pad)).astype(F32)
    else:
        X = (rng.standard_normal((M, N + pad)) * 10.0 ** rng.uniform(-1, 1, (M, N + pad))).astype(F32)
    if M and integers:
        X[-1][X[-1] == 0] = 1.0
    elif M:
        X[-1] = np.where(X[-1] < 0, X[-1] - 1, X[-1] + 1)
    X[:, N:] = COLSUM_POISON
    return X


def colsum64(X, N):
    return np.asarray(X, dtype=np.float64)[:, :N].sum(0)


def colsum_bound(X, N):
    M = X.shape[0]
    return (-(-M // 32) + 31) * U * np.abs(np.asarray(X, dtype=np.float64)[:, :N]).sum(0)


def colsum32(X, N, out_before=None, mutant=None):
    """The kernel's order: lane rl adds rows rl, rl + 32, ..; then the 32 partials in order, from 0."""
    X = np.asarray(X, dtype=F32)[:, :N]
    if mutant == "last_row_dropped":
        X = X[:-1]
    M = X.shape[0]
    trips = -(-M // 32)
    Xp = np.zeros((trips * 32, N), dtype=F32)              # (adding +0 changes nothing)
    Xp[:M] = X
    Xp = Xp.reshape(trips, 32, N)
    part = np.zeros((32, N), dtype=F32)
    for t in range(trips):
        part = part + Xp[t]
    out = np.zeros(N, dtype=F32)
    for k in range(32):
        out = out + part[k]
    if mutant == "last_column_not_written":
        out[N - 1] = out_before[N - 1]
    return out


def compare_colsum(got, X, N, integers):
    if integers:
        return compare_bits(got, colsum64(X, N).astype(F32))
    return compare_bound(got, colsum64(X, N), colsum_bound(X, N))


# ---- positional encoding ----------------------------------------------------------------------------------------------------
def gen_posenc(M, d, L, seed):
    """(x [M, d], de [M, d (1 + 2 L)]): x uniform in [-2, 2] with 0, +-fp32(pi / 2) / 2^(L-1) and +-4 planted at the front."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, (M, d)).astype(F32)
    top = F32(np.pi / 2) * F32(2.0 ** -(max(L, 1) - 1))
    planted = np.array([0.0, top, -top, 4.0, -4.0], dtype=F32)
    k = min(M * d, len(planted))
    x.reshape(-1)[:k] = planted[:k]
    de = rng.standard_normal((M, d * (1 + 2 * L))).astype(F32)
    return x, de


def _bands(x, L, dtype):
    """arg [L, M, d] = x 2^l, exact in either type."""
    x = np.asarray(x, dtype=dtype)
    return x[None] * np.array([2.0 ** l for l in range(L)], dtype=dtype).reshape(L, 1, 1)


def posenc64(x, L):
    M, d = x.shape
    out = np.empty((M, 1 + 2 * L, d), dtype=np.float64)
    out[:, 0] = x
    if L:
        arg = _bands(x, L, np.float64)
        out[:, 1::2] = np.sin(arg).transpose(1, 0, 2)
        out[:, 2::2] = np.cos(arg).transpose(1, 0, 2)
    return out.reshape(M, -1)


def posenc32(x, L, mutant=None):
    M, d = x.shape
    out = np.empty((M, 1 + 2 * L, d), dtype=F32)
    out[:, 0] = x
    if L:
        arg = _bands(x, L, F32)
        if mutant == "top_band_frequency":
            arg[L - 1] = arg[L - 1] * F32(2)
        s, c = np.sin(arg), np.cos(arg)
        if mutant == "sin_cos_swapped":
            s[0], c[0] = c[0].copy(), s[0].copy()
        out[:, 1::2] = s.transpose(1, 0, 2)
        out[:, 2::2] = c.transpose(1, 0, 2)
    return out.reshape(M, -1)


def compare_posenc(got, x, L):
    M, d = x.shape
    got = np.asarray(got, dtype=F32).reshape(M, -1)
    ident = compare_bits(got[:, :d], x)
    trig = compare_bound(got[:, d:], posenc64(x, L)[:, d:], TRIG)
    return merge(ident, trig)


def _grad_blocks(de, M, d, L, dtype):
    g = np.asarray(de, dtype=dtype).reshape(M, 1 + 2 * L, d)
    return g[:, 0], g[:, 1::2].transpose(1, 0, 2), g[:, 2::2].transpose(1, 0, 2)      # g_0 [M, d], g_s, g_c [L, M, d]


def posenc_backward64(x, de, L):
    """(dx, bound), float64."""
    M, d = x.shape
    g0, gs, gc = _grad_blocks(de, M, d, L, np.float64)
    dx, slope, mag = g0.copy(), np.zeros((M, d)), np.abs(g0)
    if L:
        arg = _bands(x, L, np.float64)
        f = np.array([2.0 ** l for l in range(L)]).reshape(L, 1, 1)
        sn, cs = np.sin(arg), np.cos(arg)
        dx = dx + (f * (cs * gs - sn * gc)).sum(0)
        slope = (f * (np.abs(gs) + np.abs(gc))).sum(0)
        mag = mag + (f * (np.abs(cs * gs) + np.abs(sn * gc))).sum(0)
    return dx, (TRIG / U + 2) * U * slope + (L + 2) * U * mag


def posenc_backward32(x, de, L, mutant=None):
    M, d = x.shape
    g0, gs, gc = _grad_blocks(de, M, d, L, F32)
    s = g0.copy()
    flat = np.asarray(de, dtype=F32).reshape(M, -1)
    for l in range(L):
        f = F32(2.0 ** l)
        arg = np.asarray(x, dtype=F32) * f
        sn, cs = np.sin(arg), np.cos(arg)
        g_s = gs[l]
        if mutant == "reads_next_column" and l == 0:
            g_s = flat[:, d + 1:2 * d + 1]                  # the sin block of band 0, one column on
        term = cs * g_s - sn * gc[l]
        s = s + (term if mutant == "no_frequency_factor" else f * term)
    return s


def compare_posenc_backward(got, x, de, L):
    ref, bound = posenc_backward64(x, de, L)
    return compare_bound(got, ref, bound)


# ---- points along rays ------------------------------------------------------------------------------------------------------
def gen_points(R, N, seed):
    """(o [R, 3], d [R, 3], z [R, N] in [2, 6], dpts [R, N, 3])."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, 3)).astype(F32), rng.standard_normal((R, 3)).astype(F32),
            rng.uniform(2, 6, (R, N)).astype(F32), rng.standard_normal((R, N, 3)).astype(F32))


def _next_ray(d, mutant):
    return np.roll(d, -1, axis=0) if mutant == "next_ray_d" else d


def points64(o, d, z):
    """(pts [R, N, 3], bound)."""
    o, d, z = (np.asarray(a, dtype=np.float64) for a in (o, d, z))
    dz = d[:, None, :] * z[:, :, None]
    pts = o[:, None, :] + dz
    return pts, U * (np.abs(dz) + np.abs(pts))


def points32(o, d, z, mutant=None):
    d = _next_ray(d, mutant)
    return o[:, None, :] + d[:, None, :] * z[:, :, None]


def points_backward64(dpts, d):
    """(dz [R, N], bound)."""
    terms = np.asarray(dpts, dtype=np.float64) * np.asarray(d, dtype=np.float64)[:, None, :]
    return terms.sum(-1), 3 * U * np.abs(terms).sum(-1)


def points_backward32(dpts, d, mutant=None):
    t = dpts * _next_ray(d, mutant)[:, None, :]
    return (t[..., 0] + t[..., 1]) + t[..., 2]


def compare_points(got, o, d, z):
    return compare_bound(got, *points64(o, d, z))


def compare_points_backward(got, dpts, d):
    return compare_bound(got, *points_backward64(dpts, d))


# ---- Adam -------------------------------------------------------------------------------------------------------------------
def hyper32(lr=ADAM_HYPER["lr"], b1=ADAM_HYPER["b1"], b2=ADAM_HYPER["b2"], eps=ADAM_HYPER["eps"]):
    """The hyper-parameters as the kernel receives them (c_float), widened."""
    return tuple(float(F32(h)) for h in (lr, b1, b2, eps))


def gen_adam(n, seed):
    """dict(p, g, m, v) of [n] fp32.  See the module docstring for the planted blocks."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    p = rng.standard_normal(n).astype(F32)
    p[idx % 2 == 1] *= F32(1e-3)
    g = (np.sign(rng.standard_normal(n)) * 10.0 ** rng.uniform(-6, 4, n)).astype(F32)
    m = (0.1 * rng.standard_normal(n)).astype(F32)
    v = (0.01 * rng.random(n)).astype(F32)
    g[idx % 8 >= 6] = 0.0
    v[idx % 8 == 7] = 0.0
    return dict(p=p, g=g, m=m, v=v)


def _ulp(x):
    """The spacing of fp32 at |x| (float64 in, float64 out)."""
    return float(np.spacing(F32(abs(x))))


def bc_rel_error(b, t):
    """r(b, t): the relative error of bc = 1 - powf(b, t) for the fp32 value b."""
    pw = b ** t
    return POW_ULPS * _ulp(pw) / (1.0 - pw) + U


def adam_rel(b1, b2, t):
    return 9 * U + bc_rel_error(b1, t) + 0.5 * bc_rel_error(b2, t)


def adam64(s, t, lr, b1, b2, eps):
    """Reference step t on the state s (fp32 arrays), hyper-parameters from hyper32.  Returns dict(m, v, delta, p) in float64 with
    their bounds bm, bv, bd."""
    p, g, m, v = (np.asarray(s[k], dtype=np.float64) for k in "pgmv")
    a1, a2 = b1 * m, (1.0 - b1) * g
    m1 = a1 + a2
    bm = 3 * U * (np.abs(a1) + np.abs(a2))
    c1, c2 = b2 * v, (1.0 - b2) * g * g
    v1 = c1 + c2
    bv = 3 * U * (np.abs(c1) + np.abs(c2))
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    S = (lr / bc1) / (np.sqrt(v1) / np.sqrt(bc2) + eps)
    delta = -S * m1
    p1 = p + delta
    rel = adam_rel(b1, b2, t)
    bd = S * bm * (1 + rel) + rel * S * np.abs(m1) + U * np.abs(p1)
    return dict(m=m1, v=v1, delta=delta, p=p1, bm=bm, bv=bv, bd=bd)


def adam32(s, t, lr, b1, b2, eps, mutant=None):
    """The kernel's statements in numpy float32: dict(p, m, v)."""
    lr, b1, b2, eps, one = F32(lr), F32(b1), F32(b2), F32(eps), F32(1)
    if mutant == "betas_swapped":
        b1, b2 = b2, b1
    p, g, m, v = (np.asarray(s[k], dtype=F32) for k in "pgmv")
    step = F32(t + 1 if mutant == "step_plus_one" else t)
    bc1, bc2 = one - np.power(b1, step), one - np.power(b2, step)
    mi = b1 * m + (one - b1) * g
    vi = b2 * v + (one - b2) * g * g
    if mutant == "eps_inside_sqrt":
        denom = np.sqrt(vi / bc2 + eps)
    elif mutant == "bc2_without_sqrt":
        denom = np.sqrt(vi) / bc2 + eps
    else:
        denom = np.sqrt(vi) / np.sqrt(bc2) + eps
    pn = p - (lr / bc1) * (mi / denom)
    if mutant == "stride_tail_unchanged":
        pn[STRIDE_THRESHOLD:], mi[STRIDE_THRESHOLD:], vi[STRIDE_THRESHOLD:] = p[STRIDE_THRESHOLD:], m[STRIDE_THRESHOLD:], v[STRIDE_THRESHOLD:]
    return dict(p=pn.astype(F32), m=mi.astype(F32), v=vi.astype(F32))


def compare_adam(got, s, t, lr, b1, b2, eps):
    """got: dict(p, m, v) after the step on state s.  Rejected entries of m', v' and of the update p' - p."""
    r = adam64(s, t, lr, b1, b2, eps)
    delta = np.asarray(got["p"], dtype=np.float64) - np.asarray(s["p"], dtype=np.float64)
    return merge(compare_bound(got["m"], r["m"], r["bm"]), compare_bound(got["v"], r["v"], r["bv"]),
                 compare_bound(delta, r["delta"], r["bd"]))


def gen_adam_table(seed):
    """The sizes of the multi-tensor launch: ADAM_TABLE_ROWS draws from ADAM_TABLE_SIZES with every size present, the largest
    neither first nor last, and a last row that is not empty."""
    rng = np.random.default_rng(seed)
    sizes = list(ADAM_TABLE_SIZES) + [int(n) for n in rng.choice(ADAM_TABLE_SIZES,ADAM_TABLE_ROWS - len(ADAM_TABLE_SIZES))]
    sizes = [int(sizes[i]) for i in rng.permutation(len(sizes))]
    big = max(ADAM_TABLE_SIZES)
    for edge in (0, -1):                                   # the largest away from both ends, the last row not empty
        if sizes[edge] in (big, 0):
            k = next(i for i in range(1, len(sizes) - 1) if sizes[i] not in (big, 0))
            sizes[edge], sizes[k] = sizes[k], sizes[edge]
    return sizes
