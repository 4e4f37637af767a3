"""The ray front end's small fp32 kernels (csrc/ns_rays.hip: ns_get_rays, ns_sphere_intersect, ns_solve_quadratic,
ns_place_samples, ns_coarse_z; csrc/ns_composite_bwd.hip: ns_place_samples_backward; csrc/ns_composite.hip: ns_argmax_gather)
entry by entry, twice: bit for bit against a numpy float32 transcription of the kernel's statements (the `*32` models), and
against float64 on the fp32 inputs (the `*64` references) inside an error bound derived from the count of roundings.  Seeded
inputs, case tables, comparators and fp32 mutants of the models.

Shared by tests/test_gpu_ray_front.py (the HIP kernels) and tests/test_ray_front_host.py (on the CPU: the generators meet their
conditions, the float64 references agree with oracle.nerf_oracle in double, every model is accepted by its float64 comparator,
the uniform model equals a literal transcription of nsplace::uniform_z and uniform_z_pair, and every mutant is rejected by the
comparator named below).  Nothing here calls the library.

Why bits.  The library is built with -ffp-contract=off and without fast-math; apart from expf in max_rgb every statement of these
kernels is a correctly rounded IEEE operation (+ - * /, sqrtf, fmaf, int -> float, comparisons, selections), and numpy float32
performs the same operations.  fmaf is the one numpy lacks (and Python 3.10 has no math.fma): fma32 below forms the product of the
fp32 operands exactly in float64 (48 bits), adds c in float64 and rounds to fp32.  That can round twice, but only where the
float64 sum lies exactly on the midpoint of two fp32 neighbours while the true sum does not: the TwoSum error term of the float64
addition (exact) says on which side the true sum lies, and the result is moved to that neighbour.  (TwoSum, not
fractions.Fraction; the host test checks fma32 against Fraction on random operands and on constructed ties.)

A comparator returns Verdict(rejected, worst) as tests/train_kernels_reference.py does: the flat indices of the rejected entries,
and the worst |err| / bound over the others.  NaN must sit in the same entries as in the reference, an infinite reference value
must be met exactly, and no entry is forgiven -- but for the UNDECIDABLE rows of the sphere and the quadratic, defined below.

U = 2^-24;  g(k) = k U / (1 - k U) bounds the relative error of k roundings in a row (Higham's gamma_k), so no spare counts are
needed for second-order terms.

Camera rays (pixel column i, row j; c2w = [r | t]):  dx = (i - cx) / fx,  dy = -((j - cy) / fy),
d_c = (dx r_c0 + dy r_c1) + (-1) r_c2,  n = sqrtf(fma(d_2, d_2, fma(d_1, d_1, d_0 d_0))),  viewdirs = d / n.
    rays_o, near, far: copies, bit for bit.
    rays_d:  |err| <= g(5) A_c,  A_c = |dx r_c0| + |dy r_c1| + |r_c2|: the subtraction, the division and the product round once
      each on the path of a product (i, j convert exactly, -1 r is exact), then the two additions.
    viewdirs:  |err| <= (e_c + |v_c| E) / n + g(4) |v_c|,  e_c the bound on d_c, E = sqrt(e_0^2 + e_1^2 + e_2^2) >= |n(d + e) - n(d)|:
      the three roundings of the sum of squares (all terms positive: 3 U relative) halve under the square root, sqrtf rounds
      once (2.5 U on n), the division once more: 3.5 U, taken as g(4).
    On the exactly representable camera (fx = fy a power of two, half-integer cx and cy, a signed permutation for r) every d_c is
    exact: float64 and fp32 agree on rays_d to the bit, which the host test asserts.

Sphere and quadratic.  b = 2 ((dx ox + dy oy) + dz oz),  c = n(o)^2 - radius^2 with n(o) = sqrtf(fma chain) squared again (the
reference's torch.norm(o) ** 2),  a = (dx dx + dy dy) + dz dz,  disc = b b - 4 a c,  t = (-b -+ sqrtf(disc)) / (2 a), minus first;
pts = o + t d.  ns_solve_quadratic receives a, b, c as they are (their errors are 0).
    e_b = 2 g(3) sum |d_i o_i|;  e_a = g(3) a;  e_c = (g(6) |o|^2 + U radius^2)(1 + U) + U |c|  (three roundings in the sum of
      squares, halved by the root, one for sqrtf, doubled by the square, one for the product: 6).
    e_disc = (1 + U) [ (1 + U)(2 |b| e_b + e_b^2) + U b^2  +  (1 + U) 4 (|a| e_c + |c| e_a + e_a e_c) + U |4 a c| ] + U |disc|.
    Where |disc64| > e_disc the sign of the discriminant is decided: negative gives NaN roots, positive gives
      e_sq = (1 + U) e_disc / sqrt(disc) + U sqrt(disc)     (sqrt(x) - sqrt(x - e) <= e / sqrt(x); it grows toward tangency),
      e_num = (1 + U)(e_b + e_sq) + U |num|,   e_t = (1 + U)(e_num + |t| 2 e_a) / (|2 a| - 2 e_a) + U |t|   (infinite once 2 e_a
      reaches |2 a|),   e_pts = (1 + U)(|d_c| e_t + U |t d_c|) + U |pts_c|.
    UNDECIDABLE rows: |disc64| <= e_disc.  Whether the fp32 discriminant is negative cannot be told, so a NaN is accepted in
      either root; a real root must lie within the bound above taken with sqrt(disc) := 0 and e_sq := (1 + 2 U) sqrt(2 e_disc)
      (the fp32 discriminant is below |disc64| + e_disc <= 2 e_disc) around -b / (2 a).
    The rounding model holds inside fp32's normal range only.  Where an intermediate of the float64 evaluation (a product, a sum
      of squares, b^2, 4 a c) exceeds FLT_MAX or is nonzero below 2^-126, e_disc is infinite: the row is undecidable by the same
      rule and anything is accepted there by the float64 comparator (the bit comparison still holds it: |o| = 1e20 gives NaN
      roots, a denormal d gives a = 0).  Only planted rows are of this kind.
    Undecidable rows may be at most 1 % of a case's random rows (UNDECIDABLE_CAP): the generators are built to meet that, and the
      host test asserts it.  The planted exact tangents (o = (-0.75 r, r, 0), d = (1, 0, 0), r a power of two: |o| = 1.25 r,
      c = 0.5625 r^2, b = -1.5 r, disc = 0 with every operation exact) are asserted on their own: both roots are 0.75 r.  The
      reference's tangent o = (-3, 1, 0), r = 1 is planted too; its n(o)^2 = fl(sqrt(10))^2 is not exact, and the model decides.

Placement (ns_place.h).  linspace(start, end, steps)[i] is start + step i below steps / 2 and end - step (steps - 1 - i) from
there, step = (end - start) / float(steps - 1).
    uniform: the MODEL is not the kernel's merge but the reference's own formulation: the fp32 grid values m + g_i, the mean
      appended, a real sort, the clip to [2, 6], NaN everywhere for a NaN mean.  The kernel's shortcut (merging the mean at its
      rank, nsplace::uniform_z) is what the bit check tests; uniform_z_literal32 and uniform_z_pair32 transcribe the shortcut and
      the host test holds them to the model.
      float64:  |err| <= g(3) std + U (|m| + std) per row: the division, the product and the add of a grid value (|step k| <= std
      on either side), then the add to the mean; the sort and the clip are 1-Lipschitz in the maximum norm, so the row's largest
      error bounds every sorted entry.  0 for an infinite mean (inf + g is exact) and at std = 0 (every g_i is 0, m + 0 is m).
    gaussian: sort(cat[m + std noise, m]), NaN last:  |err| <= max over the row's finite entries of (1 + U) U |std noise| + U |v|.
    depth_only: z = m, bit for bit.
    pts = o + d z: train_kernels_reference.points32 / compare_points (ns_points_along_rays has its own checks there).
    backward d_mean = sum_j mask_j d_z[j], sequentially in fp32 from 0; uniform: mask_j = 2 <= v_j <= 6 on the value BEFORE the
      clip (inclusive; false for NaN), the other modes: every sample.
      float64:  |err| <= g(N) sum_j mask_j |d_z[j]| + sum over the undecided j of |d_z[j]|, a sample being undecided where
      v64_j lies within the (nonzero) placement bound of 2 or of 6: its mask may go either way, so the reference leaves it out
      and the bound takes it in.  A row whose undecided samples hold a NaN or an infinity is accepted as it comes.

Coarse depths.  t_k = linspace(0, 1, N)[k]: e_t = g(3) (division, product, and the subtraction on the upper side), and 1 - t
rounds once more.
    linear  z = nr (1 - t) + fr t:   e_z = |nr| (e_t + U) + |fr| e_t + g(2) (|nr (1 - t)| + |fr t|).
    lindisp z = 1 / (1 / nr (1 - t) + 1 / fr t), s the denominator:  e_s = |1 / nr| (e_t + U) + |1 / fr| e_t +
      g(3) (|(1 - t) / nr| + |t / fr|),   e_z = e_s / (|s| (|s| - e_s)) (1 + U) + U |z|   (infinite once e_s reaches |s|).
    jitter  v = lower + (upper - lower) t_rand with mids 0.5 (z_{k+1} + z_k):  e_mid = (e_k + e_{k+1}) / 2 + U |mid|,
      e_v = e_lower + (e_upper + e_lower + U |upper - lower|) t_rand (1 + U) + U |(upper - lower) t_rand| + U |v|.
    Where an infinity enters (near = 0 under lindisp) fp32 and float64 follow the same IEEE rules: the bound is 0 there.

Argmax (nscomp::beats, transcribed as beats(); argmax_wave() walks a row in the kernel's lane and butterfly order, and the host
test holds the vectorised model to it): NaN counts as the largest value and the first NaN wins; otherwise the largest value, the first index
among equals (-0 equals +0); the start value 0 of the kernel's running best never wins, so a row of negatives returns its
largest negative.  max_w and max_z are selections: bit for bit, also in the float64 comparator (bound 0).  max_rgb =
1 / (1 + expf(-raw)) is held to train_kernels_reference.sigmoid_bound, which is imported, not restated.

Mutants of the models (one change each).  (64): the float64 comparator must reject it wherever it is not the identity;
(bits): only the bit comparison can -- the change stays inside the float64 bound.
    rays:       dy_no_negation (64), ij_swapped (64), row0_ignored (64; identity at row0 = 0), norm_plain_sum (bits).
    sphere:     roots_swapped (64), b_no_factor_2 (64), c_from_dot (bits), radius_not_squared (64; identity at radius 1).
    quadratic:  roots_swapped (64).
    uniform:    appended_no_merge (64), clip_before_merge (64), nan_mean_clipped (64), one_sided_linspace (bits; identity for
                N <= 3, at std = 0 and wherever both evaluations round alike), step_over_n_minus_1 (64; identity for N <= 3 and at std = 0).
    gaussian:   no_mean (64), no_sort (64); both need N >= 2.
    coarse:     lindisp_interpolates_depth (64; lindisp only, N >= 3 -- at N <= 2 only t = 0 and 1 occur), jitter_upper_only (64;
                needs t_rand and N >= 2).
    argmax:     last_index_on_ties (64), nan_ignored (64), start_value_wins (64).
    backward:   exclusive_bounds (64 at std = 0, where a mean of 2 or 6 sits on the clip bound exactly and the placement bound is 0;
                bits elsewhere: a sample on 2 or 6 is then within its own bound of it), mask_from_clipped (64).

Worst |err| / bound over the cases below: the fp32 model on the CPU / the HIP kernels on the MI355X.  Every bit comparison of
the kernels against the models held with no entry rejected.
    ns_get_rays (rays_d, viewdirs)          0.380 / 0.380   (0.239 on the row shard; the exact camera's rays_d: 0, float64 = fp32)
    ns_sphere_intersect (t and pts)         0.940 / 0.940
    ns_solve_quadratic                      0.713 / 0.713
    ns_place_samples uniform z              0.989 / 0.989   (pts 0.982 / 0.982)
    ns_place_samples gaussian z             1.000 / 1.000   (0.9997 at the mean 4096, N = 129: just above a power of two half
                                                             an ulp is U |v| itself; pts 0.968)
    ns_place_samples_backward               1.000 / 1.000   (0.9999995 on a row with an undecided sample, m = 6.1 and std = 0.1: the
                                                             kernel's mask takes the sample the reference leaves out, and the
                                                             sample's own |d_z| is nearly all of that row's bound; 0.518 over the
                                                             rows without an undecided sample)
    ns_coarse_z                             0.403 / 0.403
    ns_argmax_gather max_rgb                0.561 / 0.358   (numpy's expf / the device's; max_w and max_z exact)
  The kernels match the models bit for bit, so the two columns agree wherever expf is not involved.
  Undecidable share of the random rows (cap 1 %): sphere 0 of 1, 255, 256 and 257 rows at every radius, 7.6e-6 (8 rows) at
  R = 1048653, radius 2; quadratic 0 at every size.  81 % of the random sphere rows have real roots.
  Mutants that are the identity (the host test prints the list): ij_swapped on the 1 x 1 frame; row0_ignored everywhere but the row
  shard; norm_plain_sum on 1 x 1 frames and on the exact camera (its squares are exact); c_from_dot at R = 1; radius_not_squared at
  radius 1; appended_no_merge at N = 2 and at std = 0; one_sided_linspace at N <= 6, at std = 0 and at 20 more (N, std) pairs where
  both evaluations round alike (it differs at 32 of the 90); step_over_n_minus_1 at N <= 3 and at std = 0; exclusive_bounds is
  decided by float64 at std = 0 only (elsewhere a sample on 2 or 6 is within its own bound of it: bits only); the two coarse
  mutants where their branch is not taken (lindisp off or N <= 2; no t_rand or N = 1); last_index_on_ties and nan_ignored at
  N = 1 and at R = 1 (the one row there is the all-negative one).  No mutant is the identity everywhere.
  No kernel needed a rejected entry forgiven, and no derived constant was enlarged.
"""

import numpy as np

from train_kernels_reference import EW_GRID, U, compare_bits, compare_bound, merge, sigmoid64, sigmoid_bound

F32 = np.float32
F64 = np.float64
FLT_MAX = float(np.finfo(F32).max)
FLT_MIN = 2.0 ** -126
UNDECIDABLE_CAP = 0.01
CLIP_LO, CLIP_HI = F32(2.0), F32(6.0)
MODE_DEPTH_ONLY, MODE_UNIFORM, MODE_GAUSSIAN = 0, 1, 2      # NS_MODE_* of include/nerf_sampling_hip.h

# ---- the cases of the GPU tests (the host test runs the same) ---------------------------------------------------------------
SIZES = (1, 255, 256, 257, EW_GRID + 77)                    # per-element kernels; the last makes the grid-stride loop pass twice
FRAMES = ((1, 1), (5, 7), (3, 257), (1027, 1025))           # 1027 x 1025 = 1052675 rays > EW_GRID
POSES = ("look_at", "exact", "skewed")
SHARD_FRAME, SHARD_ROWS = (5, 7), (2, 5)
SPHERE_RADII = (0.5, 1.0, 2.0)
UNIFORM_N = (2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 31, 32, 33, 63, 64, 65, 128, 129)
UNIFORM_STD = (0.0, 0.01, 0.1, 0.5, 3.0)
PLACE_R = 257
UNIFORM_STRIDE4 = (1048581, 4)                              # R N / 4 > EW_GRID: the float4 kernel's second pass
UNIFORM_STRIDE = (16133, 65)                                # R N = 1048645 > EW_GRID: the generic kernel's
GAUSSIAN_N = (1, 2, 33, 64, 65, 129)
BACKWARD_STRIDE = (EW_GRID + 77, 2)
COARSE_N = (1, 2, 3, 64, 65, 128)
COARSE_R = 257
COARSE_STRIDE = (16133, 65)
ARGMAX_N = (1, 2, 63, 64, 65, 128, 192, 513)
ARGMAX_WAVES = 256 * 16 * 4                                 # ns_argmax_gather: at most 256 * 16 workgroups of four waves, a ray per wave
ARGMAX_R = (1, 257, ARGMAX_WAVES + 1)


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- comparators ------------------------------------------------------------------------------------------------------------
def compare_either(got, ref, bound, either):
    """compare_bound, but an entry of `either` (the undecidable rows) may also be NaN, and anything where its bound is infinite."""
    ref = np.asarray(ref, dtype=F64)
    got = np.asarray(got, dtype=F64).reshape(ref.shape)
    bound = np.broadcast_to(np.asarray(bound, dtype=F64), ref.shape)
    either = np.broadcast_to(np.asarray(either, dtype=bool), ref.shape)
    forgiven = either & (np.isnan(got) | np.isposinf(bound))
    return compare_bound(np.where(forgiven, ref, got), ref, np.where(forgiven | np.isnan(bound), 0.0, bound))


# ---- fmaf -------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 operands, correctly rounded (see the module docstring)."""
    a, b, c = (np.asarray(v, dtype=F32).astype(F64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b                                            # exact: 48 bits
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)                          # TwoSum: p + c = s + e exactly
        r = s.astype(F32)
        r64 = r.astype(F64)
        up, dn = np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf))
        fin = np.isfinite(s) & np.isfinite(r64)
        tie_up = fin & (s == 0.5 * (r64 + up.astype(F64))) & (e > 0)
        tie_dn = fin & (s == 0.5 * (r64 + dn.astype(F64))) & (e < 0)
    return np.where(tie_up, up, np.where(tie_dn, dn, r)).astype(F32)


def norm_sq32(x, y, z, plain=False):
    """The sum of squares under torch.norm: an fma chain (plain: the mutant's (x x + y y) + z z)."""
    with np.errstate(over="ignore", invalid="ignore"):
        if plain:
            return (x * x + y * y) + z * z
        return fma32(z, z, fma32(y, y, x * x))


# ---- camera rays ------------------------------------------------------------------------------------------------------------
def _look_at(eye, target, up=(0.0, 0.0, 1.0)):
    eye, target, up = (np.asarray(v, dtype=F64) for v in (eye, target, up))
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    return np.concatenate([np.stack([right, np.cross(back, right), back], 1), eye[:, None]], 1).astype(F32)


def gen_camera(H, W, pose, row0=0, row1=None):
    """dict(H, W, fx, fy, cx, cy, c2w [3, 4] fp32, row0, row1, near, far)."""
    cam = dict(H=H, W=W, row0=row0, row1=H if row1 is None else row1, near=2.0, far=6.0)
    if pose == "look_at":
        cam.update(fx=1111.111 * W / 800 + 3, fy=1093.7 * W / 800 + 3, cx=0.5 * W, cy=0.5 * H, c2w=_look_at((2.7, -2.1, 1.9), (0.1, 0.2, -0.1)))
    elif pose == "exact":        # a power-of-two focal length, half-integer centre, a signed permutation, small dyadic translation
        cam.update(fx=512.0, fy=512.0, cx=W // 2 + 0.5, cy=H // 2 + 0.5,
                   c2w=np.array([[0, -1, 0, 1.0], [0, 0, 1, -2.0], [-1, 0, 0, 0.5]], dtype=F32))
    elif pose == "skewed":       # not orthonormal, a large translation
        rng = np.random.default_rng(H * 10007 + W)
        c2w = np.concatenate([1.7 * rng.standard_normal((3, 3)), np.array([[1e4], [-3e5], [7e3]])], 1).astype(F32)
        cam.update(fx=0.9 * W + 1, fy=1.3 * W + 2, cx=0.37 * W, cy=0.61 * H, c2w=c2w)
    else:
        raise ValueError(pose)
    for k in ("fx", "fy", "cx", "cy", "near", "far"):
        cam[k] = float(F32(cam[k]))
    return cam


def _pixels(cam, mutant):
    j, i = np.meshgrid(np.arange(cam["row0"], cam["row1"]), np.arange(cam["W"]), indexing="ij")
    i, j = i.ravel(), j.ravel()
    if mutant == "row0_ignored":
        j = j - cam["row0"]
    if mutant == "ij_swapped":
        i, j = j, i
    return i, j


def rays32(cam, mutant=None):
    """dict(rays_o, rays_d, viewdirs [R, 3], ray_batch [R, 11]) as get_rays_kernel writes them."""
    i, j = _pixels(cam, mutant)
    fx, fy, cx, cy = (F32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    r, t = cam["c2w"][:, :3], cam["c2w"][:, 3]
    dx = (i.astype(F32) - cx) / fx
    dy = (j.astype(F32) - cy) / fy
    if mutant != "dy_no_negation":
        dy = -dy
    d = np.stack([(dx * r[c, 0] + dy * r[c, 1]) + F32(-1.0) * r[c, 2] for c in range(3)], 1)
    n = np.sqrt(norm_sq32(d[:, 0], d[:, 1], d[:, 2], plain=mutant == "norm_plain_sum"))
    v = d / n[:, None]
    R = d.shape[0]
    o = np.broadcast_to(t, (R, 3)).astype(F32)
    nf = np.broadcast_to(np.array([cam["near"], cam["far"]], dtype=F32), (R, 2))
    return dict(rays_o=o, rays_d=d, viewdirs=v, ray_batch=np.concatenate([o, d, nf, v], 1))


def rays64(cam):
    """dict(rays_d, viewdirs, bound_d, bound_v) in float64."""
    i, j = _pixels(cam, None)
    r, t = cam["c2w"][:, :3].astype(F64), cam["c2w"][:, 3].astype(F64)
    dx = (i - cam["cx"]) / cam["fx"]
    dy = -((j - cam["cy"]) / cam["fy"])
    d = np.stack([dx * r[c, 0] + dy * r[c, 1] - r[c, 2] for c in range(3)], 1)
    e = gamma(5) * np.stack([np.abs(dx * r[c, 0]) + np.abs(dy * r[c, 1]) + np.abs(r[c, 2]) for c in range(3)], 1)
    n = np.sqrt((d * d).sum(1))[:, None]
    v = d / n
    E = np.sqrt((e * e).sum(1))[:, None]
    return dict(rays_d=d, viewdirs=v, bound_d=e, bound_v=(e + np.abs(v) * E) / n + gamma(4) * np.abs(v))


def compare_rays(got, cam):
    """got: dict with any of rays_o, rays_d, viewdirs, ray_batch."""
    ref = rays64(cam)
    R = ref["rays_d"].shape[0]
    o = np.broadcast_to(cam["c2w"][:, 3], (R, 3))
    nf = np.broadcast_to(np.array([cam["near"], cam["far"]], dtype=F32), (R, 2))
    out = []
    if "rays_o" in got:
        out.append(compare_bits(got["rays_o"], o))
    if "rays_d" in got:
        out.append(compare_bound(np.reshape(got["rays_d"], (R, 3)), ref["rays_d"], ref["bound_d"]))
    if "viewdirs" in got:
        out.append(compare_bound(np.reshape(got["viewdirs"], (R, 3)), ref["viewdirs"], ref["bound_v"]))
    if "ray_batch" in got:
        b = np.reshape(got["ray_batch"], (R, 11))
        out += [compare_bits(b[:, 0:3], o), compare_bound(b[:, 3:6], ref["rays_d"], ref["bound_d"]), compare_bits(b[:, 6:8], nf),
                compare_bound(b[:, 8:11], ref["viewdirs"], ref["bound_v"])]
    return merge(*out)


# ---- sphere and quadratic ---------------------------------------------------------------------------------------------------
TANGENT_K = (1, 2, 8, 64)                                   # impact parameters radius (1 +- k 2^-20)


def sphere_planted(radius):
    """[(name, o, d)]: the planted rows of a sphere case."""
    r = radius
    rows = [("toward", (-3, 0, 0), (1, 0, 0)), ("parallel_miss", (-3, 0, 0), (0, 2, 0)), ("away", (-3, 0, 0), (-1, 0, 0)),
            ("reference_tangent", (-3, 1, 0), (1, 0, 0)), ("on_sphere", (1, 0, 0), (0, 1, 0)), ("inside", (0, 0, 0), (-1, 0, 0)),
            ("on_sphere_inward", (1, 0, 0), (-1, 0, 0)),
            ("exact_tangent", (-0.75 * r, r, 0), (1, 0, 0)), ("exact_tangent_z", (0, -0.75 * r, -r), (0, 2, 0))]
    for k in TANGENT_K:
        for s in (1, -1):
            rows.append((f"impact_{'+' if s > 0 else '-'}{k}", (-3 * r, float(F32(r * (1 + s * k * 2.0 ** -20))), 0), (1, 0, 0)))
    rows += [("o_zero", (0, 0, 0), (0.3, -1.1, 0.7)), ("d_zero", (1, 2, 3), (0, 0, 0)), ("d_denormal", (-3, 0, 0), (1e-40, 0, 0)),
             ("o_huge", (1e20, 0, 0), (-1, 0, 0)), ("o_nan", (np.nan, 0, 1), (1, 0, 0)), ("d_nan", (-3, 0, 0), (1, np.nan, 0)),
             ("o_inf", (-np.inf, 0, 0), (1, 0, 0)), ("d_inf", (-3, 0, 0), (np.inf, 0, 0))]
    return rows


def _plant(n, planted):
    """Row indices for `planted` rows in an array of n: the front (as many as fit) and, from 2 x as many rows on, the back too."""
    k = min(n, planted)
    front = np.arange(k)
    back = np.arange(n - planted, n) if n >= 2 * planted else np.zeros(0, dtype=np.int64)
    return front, back


def gen_sphere(R, radius, seed):
    """(o, d [R, 3] fp32, random [R] bool, rows {name: index}): rays from the shell of radius 2 radius toward a ball of
    1.25 radius (about a fifth miss), direction lengths over two decades; sphere_planted at the front and again at the back."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((R, 3))
    o = 2.0 * radius * u / np.linalg.norm(u, axis=1, keepdims=True)
    w = rng.standard_normal((R, 3))
    target = 1.25 * radius * w / np.linalg.norm(w, axis=1, keepdims=True) * rng.random((R, 1)) ** (1 / 3)
    d = (target - o) * 10.0 ** rng.uniform(-1, 1, (R, 1))
    o, d = o.astype(F32), d.astype(F32)
    planted = sphere_planted(radius)
    front, back = _plant(R, len(planted))
    random = np.ones(R, dtype=bool)
    rows = {}
    for idx in (front, back):
        for k, at in enumerate(idx):
            name, po, pd = planted[k]
            o[at], d[at] = po, pd
            random[at] = False
            rows.setdefault(name, int(at))
    return o, d, random, rows


def sphere32(o, d, radius, mutant=None):
    """(t [R, 2], pts [R, 2, 3]) as sphere_kernel writes them."""
    o, d, radius = np.asarray(o, dtype=F32), np.asarray(d, dtype=F32), F32(radius)
    ox, oy, oz, dx, dy, dz = o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]
    two, four = F32(2), F32(4)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        b = (dx * ox + dy * oy) + dz * oz
        if mutant != "b_no_factor_2":
            b = two * b
        rr = radius if mutant == "radius_not_squared" else radius * radius
        if mutant == "c_from_dot":
            c = ((ox * ox + oy * oy) + oz * oz) - rr
        else:
            on = np.sqrt(norm_sq32(ox, oy, oz))
            c = on * on - rr
        a = (dx * dx + dy * dy) + dz * dz
        return _sphere_points32(o, d, _roots32(a, b, c, mutant))


def _roots32(a, b, c, mutant=None):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        sq = np.sqrt(b * b - F32(4) * a * c)
        t0, t1 = (-b - sq) / (F32(2) * a), (-b + sq) / (F32(2) * a)
    return (t1, t0) if mutant == "roots_swapped" else (t0, t1)


def _sphere_points32(o, d, roots):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = np.stack(roots, 1)
        return t, o[:, None, :] + t[:, :, None] * d[:, None, :]


def quadratic32(a, b, c, mutant=None):
    """out [2, n]: the minus-sqrt root first."""
    return np.stack(_roots32(np.asarray(a, dtype=F32), np.asarray(b, dtype=F32), np.asarray(c, dtype=F32), mutant), 0)


def _out_of_range(*values):
    """Rows where a float64 intermediate leaves fp32's normal range (above FLT_MAX, or nonzero below 2^-126)."""
    bad = np.zeros(np.shape(values[0]), dtype=bool)
    for v in values:
        m = np.abs(v)
        bad |= (m > FLT_MAX) | ((m > 0) & (m < FLT_MIN))
    return bad


def roots64(a, b, c, ea, eb, ec, oor):
    """dict(t [n, 2], bound [n, 2], undecidable [n], e_disc [n]) of a x^2 + b x + c in float64, the coefficients known within
    ea, eb, ec; `oor` marks the rows whose error model does not hold (e_disc infinite)."""
    with np.errstate(all="ignore"):
        bb, ac4 = b * b, 4 * a * c
        disc = bb - ac4
        e_bb = (1 + U) * (2 * np.abs(b) * eb + eb * eb) + U * bb
        e_ac = (1 + U) * 4 * (np.abs(a) * ec + np.abs(c) * ea + ea * ec) + U * np.abs(ac4)
        e_disc = (1 + U) * (e_bb + e_ac) + U * np.abs(disc)
        oor = oor | _out_of_range(bb, ac4, a)
        e_disc = np.where(oor | (~np.isfinite(e_disc) & ~np.isnan(disc)), np.inf, e_disc)
        und = np.abs(disc) <= e_disc                         # (a NaN discriminant inside the range is decided: NaN roots)
        sq = np.where(und, 0.0, np.sqrt(disc))
        e_sq = np.where(und, (1 + 2 * U) * np.sqrt(2 * e_disc), (1 + U) * e_disc / sq + U * sq)
        den, e_den = 2 * a, 2 * ea
        t, bound = [], []
        for sign in (-1.0, 1.0):
            num = -b + sign * sq
            e_num = (1 + U) * (eb + e_sq) + U * np.abs(num)
            tk = num / den
            room = np.abs(den) - e_den
            bk = np.where(room > 0, (1 + U) * (e_num + np.abs(tk) * e_den) / room + U * np.abs(tk), np.inf)
            t.append(tk)
            bound.append(np.where(oor, np.inf, bk))
    return dict(t=np.stack(t, 1), bound=np.stack(bound, 1), undecidable=und, e_disc=e_disc)


def sphere64(o, d, radius):
    """roots64's dict plus pts [R, 2, 3] and bound_pts."""
    o, d, radius = np.asarray(o, dtype=F32).astype(F64), np.asarray(d, dtype=F32).astype(F64), float(F32(radius))
    with np.errstate(all="ignore"):
        prod = d * o
        b = 2 * prod.sum(1)
        eb = 2 * gamma(3) * np.abs(prod).sum(1)
        oo = (o * o).sum(1)
        c = oo - radius * radius
        ec = (gamma(6) * oo + U * radius * radius) * (1 + U) + U * np.abs(c)
        a = (d * d).sum(1)
        ea = gamma(3) * a
        oor = _out_of_range(prod[:, 0], prod[:, 1], prod[:, 2], *(o * o).T, *(d * d).T, oo, a, b)
        r = roots64(a, b, c, ea, eb, ec, oor)
        t, et = r["t"], r["bound"]
        td = t[:, :, None] * d[:, None, :]
        pts = o[:, None, :] + td
        r["pts"] = pts
        r["bound_pts"] = (1 + U) * (np.abs(d)[:, None, :] * et[:, :, None] + U * np.abs(td)) + U * np.abs(pts)
    return r


def compare_sphere(got_t, got_pts, o, d, radius):
    """Either output may be None (not requested)."""
    r = sphere64(o, d, radius)
    und = r["undecidable"]
    out = []
    if got_t is not None:
        out.append(compare_either(np.reshape(got_t, (-1, 2)), r["t"], r["bound"], und[:, None]))
    if got_pts is not None:
        out.append(compare_either(np.reshape(got_pts, (-1, 2, 3)), r["pts"], r["bound_pts"], und[:, None, None]))
    return merge(*out)


QUAD_PLANTED = ((0.0, 3.0, 1.0), (1.0, 1.0, 1.0), (1.0, 2.0, 1.0), (np.nan, 1.0, 1.0), (4.0, 4.0, 1.0), (5.0, 6.0, 1.0))
QUAD_NAMES = ("a_zero", "disc_negative", "disc_zero", "nan", "reference_double_root", "reference_two_roots")


def gen_quadratic(n, seed):
    """(a, b, c [n] fp32, random [n] bool, rows): normal draws, about half with real roots; QUAD_PLANTED at the front and back."""
    rng = np.random.default_rng(seed)
    a, b, c = (rng.standard_normal(n).astype(F32) for _ in range(3))
    b = (b * F32(2)).astype(F32)
    front, back = _plant(n, len(QUAD_PLANTED))
    random = np.ones(n, dtype=bool)
    rows = {}
    for idx in (front, back):
        for k, at in enumerate(idx):
            a[at], b[at], c[at] = QUAD_PLANTED[k]
            random[at] = False
            rows.setdefault(QUAD_NAMES[k], int(at))
    return a, b, c, random, rows


def quadratic64(a, b, c):
    a, b, c = (np.asarray(v, dtype=F32).astype(F64) for v in (a, b, c))
    zero = np.zeros_like(a)
    return roots64(a, b, c, zero, zero, zero, np.zeros(a.shape, dtype=bool))


def compare_quadratic(got, a, b, c):
    """got [2, n]."""
    r = quadratic64(a, b, c)
    return compare_either(np.reshape(got, (2, -1)).T, r["t"], r["bound"], r["undecidable"][:, None])


# ---- placement --------------------------------------------------------------------------------------------------------------
def linspace_step32(start, end, step, steps, i):
    """nsplace::linspace_step at the integer array i."""
    i = np.asarray(i)
    if steps <= 1:
        return np.full(i.shape, start, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = start + step * i.astype(F32)
        hi = end - step * (steps - i - 1).astype(F32)
    return np.where(i < steps // 2, lo, hi).astype(F32)


def linspace_at32(start, end, steps, i, one_sided=False):
    """nsplace::linspace_at (torch.linspace's two-sided evaluation)."""
    start, end = F32(start), F32(end)
    i = np.asarray(i)
    if steps <= 1:
        return np.full(i.shape, start, dtype=F32)
    step = (end - start) / F32(steps - 1)
    if one_sided:
        return (start + step * i.astype(F32)).astype(F32)
    return linspace_step32(start, end, step, steps, i)


def _clip32(v):
    return np.minimum(np.maximum(v, CLIP_LO), CLIP_HI)       # (NaN stays NaN, as torch.clip keeps it)


def _uniform_grid32(N, std, mutant=None):
    steps, std = N - 1, F32(std)
    denom = F32(N - 1 if mutant == "step_over_n_minus_1" else N - 2)
    step = (std - (-std)) / denom if N > 2 else F32(0)
    i = np.arange(steps)
    if mutant == "one_sided_linspace":
        return (-std + step * i.astype(F32)).astype(F32) if steps > 1 else np.full(1, -std, dtype=F32)
    return linspace_step32(-std, std, step, steps, i)


def uniform_unclipped32(mean, N, std, mutant=None):
    """sort(cat[m + linspace(-std, std, N - 1), m]) in fp32, [R, N]."""
    M = np.asarray(mean, dtype=F32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        a = M + _uniform_grid32(N, std, mutant)[None, :]
    if mutant == "clip_before_merge":
        a = _clip32(a)
    z = np.concatenate([a, M], 1)
    return z if mutant == "appended_no_merge" else np.sort(z, 1)


def place_uniform32(mean, N, std, mutant=None):
    z = uniform_unclipped32(mean, N, std, mutant)
    if mutant != "clip_before_merge":
        z = _clip32(z)
    if mutant == "nan_mean_clipped":
        z = np.where(np.isnan(z), CLIP_LO, z)
    return z.astype(F32)


def uniform_z_literal32(mean, N, std, clip=True):
    """nsplace::uniform_z (clip=False: uniform_z_unclipped) statement by statement, [R, N]."""
    steps, std = N - 1, F32(std)
    step = (std - (-std)) / F32(N - 2) if N > 2 else F32(0)
    M = np.asarray(mean, dtype=F32)[:, None]
    j = np.arange(N)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        b = M + linspace_step32(-std, std, step, steps, np.minimum(j, steps - 1))
        v = np.where((j < steps) & (b < M), b, np.broadcast_to(M, b.shape))
        a = M + linspace_step32(-std, std, step, steps, np.maximum(j - 1, 0))
        v = np.where((v == M) & (j >= 1) & ~(a < M), a, v)
        if clip:
            v = np.where(np.isnan(M), M, np.fmin(np.fmax(v, CLIP_LO), CLIP_HI))        # fmaxf / fminf drop a NaN operand
    return v.astype(F32)


def uniform_z_pair32(mean, N, std):
    """nsplace::uniform_z_pair for j = 0 .. N - 2: (z [R, N - 1], z_next [R, N - 1]), i.e. samples j and j + 1."""
    steps, std = N - 1, F32(std)
    step = (std - (-std)) / F32(N - 2) if N > 2 else F32(0)
    half, one, fs1 = steps // 2, steps <= 1, F32(steps - 1)
    M = np.asarray(mean, dtype=F32)[:, None]
    j = np.arange(N - 1)[None, :]
    fj = j.astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        def grid(k, fk):
            lo, hi = -std + step * fk, std - step * (fs1 - fk)
            return M + np.where((k < half) | one, lo, hi)

        def pick(jj, below, here):
            v = np.where((jj < steps) & (here < M), here, np.broadcast_to(M, here.shape))
            v = np.where((v == M) & (jj >= 1) & ~(below < M), below, v)
            return np.where(np.isnan(M), M, np.fmin(np.fmax(v, CLIP_LO), CLIP_HI)).astype(F32)

        am, a0, ap = grid(j - 1, fj - F32(1)), grid(j, fj), grid(j + 1, fj + F32(1))
        return pick(j, am, a0), pick(j + 1, a0, ap)


def _uniform_unclipped64(mean, N, std):
    """(v [R, N], bound [R, 1]) before the clip."""
    m = np.asarray(mean, dtype=F32).astype(F64)[:, None]
    std = float(F32(std))
    steps = N - 1
    g = -std + (2 * std / (steps - 1)) * np.arange(steps) if steps > 1 else np.array([-std])
    if steps > 1:
        g[steps // 2:] = std - (2 * std / (steps - 1)) * (steps - 1 - np.arange(steps // 2, steps))
    with np.errstate(invalid="ignore"):
        v = np.sort(np.concatenate([m + g[None, :], m], 1), 1)
        bound = gamma(3) * std + U * (np.abs(m) + std)
    return v, np.where(np.isfinite(m) & (std > 0), bound, 0.0)


def place_uniform64(mean, N, std):
    """(z [R, N], bound [R, 1])."""
    v, bound = _uniform_unclipped64(mean, N, std)
    return np.minimum(np.maximum(v, 2.0), 6.0), bound


def compare_uniform(got, mean, N, std):
    z, bound = place_uniform64(mean, N, std)
    return compare_bound(np.reshape(got, z.shape), z, np.broadcast_to(bound, z.shape))


MEAN_PLANTED_COUNT = 21


def gen_means(R, std, seed):
    """[R] fp32: uniform draws in [2, 6] with the planted means at the front and again at the back (R >= 2 x 21)."""
    rng = np.random.default_rng(seed)
    std = F32(std)
    planted = np.array([2, 6, F32(2) + std, F32(6) - std, 1.9, 6.1, np.nextafter(F32(2), F32(0)), np.nextafter(F32(2), F32(9)),
                        np.nextafter(F32(6), F32(0)), np.nextafter(F32(6), F32(9)), 0, -3, np.inf, -np.inf, np.nan, 1e-30, 4096,
                        2.0 ** 24, 4, 3.5, 2.5], dtype=F32)
    assert planted.size == MEAN_PLANTED_COUNT and R >= 2 * planted.size
    m = rng.uniform(2, 6, R).astype(F32)
    m[:planted.size] = planted
    m[-planted.size:] = planted
    return m


def gen_rays_od(R, seed):
    """(o, d [R, 3]) for the pts output."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((R, 3)).astype(F32), rng.standard_normal((R, 3)).astype(F32)


NOISE_PLANTED = np.array([0.0, 0.75, 0.75, np.inf, -np.inf, np.nan, -0.75], dtype=F32)


def gen_noise(R, N, seed):
    """[R, N - 1] standard normal draws; rows 30 .. 36 carry 0, equal draws, +-inf and NaN (cycled along the row), row 37 is
    all zeros (every sample equals the mean) and row 38 all equal."""
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((R, max(N - 1, 0))).astype(F32)
    if N > 1:
        for k in range(len(NOISE_PLANTED)):
            noise[30 + k, :min(N - 1, 3)] = np.roll(NOISE_PLANTED, k)[:min(N - 1, 3)]
        noise[37], noise[38] = 0.0, 1.25
    return noise


def place_gaussian32(mean, noise, N, std, mutant=None):
    M = np.asarray(mean, dtype=F32)[:, None]
    if N == 1:
        return M.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        v = M + F32(std) * np.asarray(noise, dtype=F32)
    z = np.concatenate([v, v[:, :1] if mutant == "no_mean" else M], 1)
    return z if mutant == "no_sort" else np.sort(z, 1)


def place_gaussian64(mean, noise, N, std):
    """(z [R, N], bound [R, 1])."""
    m = np.asarray(mean, dtype=F32).astype(F64)[:, None]
    if N == 1:
        return m.copy(), np.zeros_like(m)
    with np.errstate(invalid="ignore", over="ignore"):
        sn = float(F32(std)) * np.asarray(noise, dtype=F32).astype(F64)
        v = m + sn
        e = (1 + U) * U * np.abs(sn) + U * np.abs(v)
        bound = np.where(np.isfinite(e), e, 0.0).max(1, keepdims=True)
    return np.sort(np.concatenate([v, m], 1), 1), bound


def compare_gaussian(got, mean, noise, N, std):
    z, bound = place_gaussian64(mean, noise, N, std)
    return compare_bound(np.reshape(got, z.shape), z, np.broadcast_to(bound, z.shape))


# ---- placement backward -----------------------------------------------------------------------------------------------------
def gen_dz(R, N, seed):
    """[R, N] normal upstream gradients; 0, NaN and +inf planted in rows 21 .. 29 (random means), first, middle and last column."""
    rng = np.random.default_rng(seed)
    dz = rng.standard_normal((R, N)).astype(F32)
    if R >= 30:
        for k, val in enumerate((0.0, np.nan, np.inf)):
            for c, col in enumerate((0, N // 2, N - 1)):
                dz[21 + 3 * k + c, col] = val
    return dz


def _sequential_sum32(terms, mask):
    s = np.zeros(terms.shape[0], dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(terms.shape[1]):
            s = np.where(mask[:, j], s + terms[:, j], s)
    return s


def place_backward32(mode, mean, dz, N, std, mutant=None):
    dz = np.asarray(dz, dtype=F32)
    if mode == MODE_DEPTH_ONLY:
        N = 1
    dz = dz.reshape(-1, N)
    mask = np.ones(dz.shape, dtype=bool)
    if mode == MODE_UNIFORM:
        v = uniform_unclipped32(mean, N, std)
        if mutant == "mask_from_clipped":
            v = _clip32(v)
        with np.errstate(invalid="ignore"):
            mask = (v > CLIP_LO) & (v < CLIP_HI) if mutant == "exclusive_bounds" else (v >= CLIP_LO) & (v <= CLIP_HI)
    return _sequential_sum32(dz, mask)


def place_backward64(mode, mean, dz, N, std):
    """(d_mean [R], bound [R], either [R])."""
    if mode == MODE_DEPTH_ONLY:
        N = 1
    g = np.asarray(dz, dtype=F32).astype(F64).reshape(-1, N)
    mask = np.ones(g.shape, dtype=bool)
    open_ = np.zeros(g.shape, dtype=bool)
    if mode == MODE_UNIFORM:
        v, bz = _uniform_unclipped64(mean, N, std)
        with np.errstate(invalid="ignore"):
            mask = (v >= 2.0) & (v <= 6.0)
            open_ = (np.abs(v - 2.0) <= bz) & (bz > 0) | (np.abs(v - 6.0) <= bz) & (bz > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = np.where(mask & ~open_, g, 0.0).sum(1)
        mag = np.where(mask | open_, np.abs(g), 0.0)
        bound = gamma(N) * mag.sum(1) + np.where(open_, np.abs(g), 0.0).sum(1)
    either = (open_ & ~np.isfinite(g)).any(1)
    return ref, np.where(either, np.inf, bound), either


def compare_place_backward(got, mode, mean, dz, N, std):
    ref, bound, either = place_backward64(mode, mean, dz, N, std)
    return compare_either(got, ref, bound, either)


# ---- coarse depths ----------------------------------------------------------------------------------------------------------
NEAR_FAR_PLANTED = ((2.0, 6.0), (0.05, 1e3), (3.0, 3.0), (6.0, 2.0), (0.0, 6.0), (np.nan, 6.0), (2.0, np.nan))
T_RAND_PLANTED = np.array([0.0, 0.5, 1.0 - 2.0 ** -24], dtype=F32)


def gen_coarse(R, N, seed):
    """(near, far [R], t_rand [R, N]): near in [0.05, 3], far = near + [0.5, 10]; NEAR_FAR_PLANTED at the front and the back;
    t_rand in [0, 1) with 0, 0.5 and 1 - 2^-24 planted along rows 0 and 8."""
    rng = np.random.default_rng(seed)
    near = rng.uniform(0.05, 3, R).astype(F32)
    far = (near + rng.uniform(0.5, 10, R)).astype(F32)
    front, back = _plant(R, len(NEAR_FAR_PLANTED))
    for idx in (front, back):
        for k, at in enumerate(idx):
            near[at], far[at] = NEAR_FAR_PLANTED[k]
    t_rand = rng.random((R, N)).astype(F32)
    for row in (0, 8):
        if row < R:
            t_rand[row, :] = np.resize(T_RAND_PLANTED, N)
    return near, far, t_rand


def _jitter(z, t_rand, half, upper_only=False):
    upper = np.concatenate([half * (z[:, 1:] + z[:, :-1]), z[:, -1:]], 1)
    lower = z if upper_only else np.concatenate([z[:, :1], half * (z[:, 1:] + z[:, :-1])], 1)
    return lower, upper, lower + (upper - lower) * t_rand


def coarse32(near, far, N, lindisp, t_rand=None, mutant=None):
    nr, fr = np.asarray(near, dtype=F32)[:, None], np.asarray(far, dtype=F32)[:, None]
    t = linspace_at32(0.0, 1.0, N, np.arange(N))[None, :]
    one = F32(1)
    with np.errstate(all="ignore"):
        if lindisp and mutant != "lindisp_interpolates_depth":
            z = one / (one / nr * (one - t) + one / fr * t)
        else:
            z = nr * (one - t) + fr * t
        if t_rand is not None:
            # upper = 0.5 (z[i + 1] + v), lower = 0.5 (v + z[i - 1]): the same two operands, and fp32 addition commutes
            z = _jitter(z, np.asarray(t_rand, dtype=F32), F32(0.5), mutant == "jitter_upper_only")[2]
    return z.astype(F32)


def coarse64(near, far, N, lindisp, t_rand=None):
    """(z [R, N], bound [R, N])."""
    nr, fr = np.asarray(near, dtype=F32).astype(F64)[:, None], np.asarray(far, dtype=F32).astype(F64)[:, None]
    k = np.arange(N)
    t = (k / (N - 1) if N > 1 else np.zeros(1))[None, :]
    et = gamma(3) if N > 1 else 0.0
    with np.errstate(all="ignore"):
        if lindisp:
            a, b = 1.0 / nr * (1.0 - t), 1.0 / fr * t
            s = a + b
            es = np.abs(1.0 / nr) * (et + U) + np.abs(1.0 / fr) * et + gamma(3) * (np.abs(a) + np.abs(b))
            z = 1.0 / s
            room = np.abs(s) - es
            e = np.where(room > 0, es / (np.abs(s) * room) * (1 + U) + U * np.abs(z), np.inf)
        else:
            a, b = nr * (1.0 - t), fr * t
            z = a + b
            e = np.abs(nr) * (et + U) + np.abs(fr) * et + gamma(2) * (np.abs(a) + np.abs(b))
        e = np.where(np.isnan(e) | ~np.isfinite(z), 0.0, e)
        if t_rand is not None:
            tr = np.asarray(t_rand, dtype=F32).astype(F64)
            lower, upper, v = _jitter(z, tr, 0.5)
            em = 0.5 * (e[:, 1:] + e[:, :-1])
            eu = np.concatenate([em, e[:, -1:]], 1) + U * np.abs(upper) * (k < N - 1)
            el = np.concatenate([e[:, :1], em], 1) + U * np.abs(lower) * (k > 0)
            e = el + (eu + el + U * np.abs(upper - lower)) * tr * (1 + U) + U * np.abs((upper - lower) * tr) + U * np.abs(v)
            z = v
            e = np.where(np.isnan(e) | ~np.isfinite(z), 0.0, e)
    return z, e


def compare_coarse(got, near, far, N, lindisp, t_rand=None):
    z, e = coarse64(near, far, N, lindisp, t_rand)
    return compare_bound(np.reshape(got, z.shape), z, e)


# ---- argmax -----------------------------------------------------------------------------------------------------------------
ARGMAX_PLANTED = ("all_zero", "all_negative", "minus_zero_first", "two_nans", "plus_inf", "duplicate_max", "max_last")


def gen_argmax(R, N, seed):
    """(w [R, N], z [R, N], raw [R, N, 4], rows {name: index}): weights in [0, 1), raw colours over +-15; the planted rows come
    first, `all_negative` leading (it is the one row of R = 1), and again at the back."""
    rng = np.random.default_rng(seed)
    w = rng.random((R, N)).astype(F32)
    z = rng.uniform(2, 6, (R, N)).astype(F32)
    raw = (5 * rng.standard_normal((R, N, 4))).astype(F32)
    order = ("all_negative",) + tuple(n for n in ARGMAX_PLANTED if n != "all_negative")
    front, back = _plant(R, len(order))
    rows = {}
    for idx in (front, back):
        for k, at in enumerate(idx):
            name = order[k]
            rows.setdefault(name, int(at))
            if name == "all_zero":
                w[at] = 0.0
            elif name == "all_negative":
                w[at] = -1.0 - w[at]
            elif name == "minus_zero_first":
                w[at] = 0.0
                w[at, 0] = -0.0
            elif name == "two_nans":
                w[at, N // 3] = w[at, (2 * N) // 3] = np.nan
                w[at, N - 1] = 2.0
            elif name == "plus_inf":
                w[at, N // 2] = np.inf
            elif name == "duplicate_max":           # lanes i and i + 64 of the same wave where the row is long enough
                i = min(5, N - 1)
                w[at, i] = w[at, i + 64 if i + 64 < N else N - 1] = 1.5
            elif name == "max_last":
                w[at, N - 1] = 1.5
    return w, z, raw, rows


NO_SAMPLE = 0x7FFFFFFF


def beats(v, i, bv, bi):
    """nscomp::beats statement by statement: does sample (v, i) come before the running best (bv, bi)?"""
    if i == NO_SAMPLE:
        return False
    if bi == NO_SAMPLE:
        return True
    vn, bn = v != v, bv != bv
    if vn != bn:
        return vn
    if vn:
        return i < bi
    if v != bv:
        return v > bv
    return i < bi


def argmax_wave(row):
    """The index argmax_gather_kernel finds in one row, in the kernel's own order: lane l runs over samples l, l + 64, .. from
    the start value (0, NO_SAMPLE), then the 64 lanes meet in a butterfly (lane ^ 1, ^ 2, .. ^ 32)."""
    row = [float(x) for x in row]
    best = []
    for lane in range(64):
        bv, bi = 0.0, NO_SAMPLE
        for i in range(lane, len(row), 64):
            if beats(row[i], i, bv, bi):
                bv, bi = row[i], i
        best.append((bv, bi))
    m = 1
    while m < 64:
        best = [best[l ^ m] if beats(*best[l ^ m], *best[l]) else best[l] for l in range(64)]
        m <<= 1
    assert all(b[1] == best[0][1] for b in best), "beats is a total order: every lane ends with the same sample"
    return best[0][1]


def argmax_index32(w, mutant=None):
    """(index [R], start_wins [R]) in the order of nscomp::beats."""
    w = np.asarray(w, dtype=F32)
    nan = np.isnan(w)
    R, N = w.shape
    clean = np.where(nan, F32(-np.inf), w)

    def first_max(x):
        return (N - 1 - np.argmax(x[:, ::-1], 1)) if mutant == "last_index_on_ties" else np.argmax(x, 1)

    idx = first_max(clean)
    if mutant != "nan_ignored":
        idx = np.where(nan.any(1), first_max(nan), idx)
    start_wins = np.zeros(R, dtype=bool)
    if mutant == "start_value_wins":
        start_wins = ~nan.any(1) & (clean.max(1) < 0)
    return idx, start_wins


def argmax32(w, z, raw, mutant=None):
    """dict(max_w [R], max_z [R], max_rgb [R, 3]); max_rgb in fp32 with numpy's expf (it is compared inside the sigmoid bound)."""
    idx, start_wins = argmax_index32(w, mutant)
    rows = np.arange(w.shape[0])
    idx = np.where(start_wins, 0, idx)
    with np.errstate(over="ignore"):
        rgb = (F32(1) / (F32(1) + np.exp(-raw[rows, idx, :3]))).astype(F32)
    return dict(max_w=np.where(start_wins, F32(0), w[rows, idx]), max_z=z[rows, idx], max_rgb=rgb)


def compare_argmax(got, w, z, raw):
    """got: dict with any of max_w, max_z, max_rgb.  The selections are exact in float64 too (bound 0)."""
    idx, _ = argmax_index32(w)
    rows = np.arange(w.shape[0])
    out = []
    if "max_w" in got:
        out.append(compare_bound(got["max_w"], w[rows, idx].astype(F64), 0.0))
    if "max_z" in got:
        out.append(compare_bound(got["max_z"], z[rows, idx].astype(F64), 0.0))
    if "max_rgb" in got:
        x = raw[rows, idx, :3]
        out.append(compare_bound(np.reshape(got["max_rgb"], x.shape), sigmoid64(x), sigmoid_bound(x)))
    return merge(*out)
