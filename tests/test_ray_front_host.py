"""tests/ray_front_reference.py on the CPU, at every case tests/test_gpu_ray_front.py runs: the generators meet their stated
conditions (planted rows present, undecidable share at most 1 %), every fp32 model is accepted by its float64 comparator (the
worst |err| / bound is printed), the uniform model equals the literal transcriptions of nsplace::uniform_z and uniform_z_pair
bit for bit, the float64 references agree with oracle.nerf_oracle in double, and every mutant is rejected by the comparator the
reference module names for it (a mutant that is the identity at a case is listed in the output; none is the identity everywhere)."""

import contextlib
from fractions import Fraction

import numpy as np
import torch

import ray_front_reference as K
from oracle import nerf_oracle as O

F32 = np.float32


@contextlib.contextmanager
def _double():
    """The oracle's torch.linspace follows the default dtype: double inside this block."""
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(before)


def _accepted(verdict, what):
    assert verdict.rejected.size == 0, (what, verdict.rejected[:8], verdict.worst)
    assert verdict.worst <= 1.0, (what, verdict.worst)
    return verdict.worst


class Mutants:
    """Tally of one family's mutants over its cases: kind "64" must be rejected by the float64 comparator wherever its bits
    differ from the model's, kind "bits" only has to differ somewhere."""

    def __init__(self, kinds):
        self.kinds = kinds
        self.differed = {name: 0 for name in kinds}
        self.identity = {name: [] for name in kinds}

    def see(self, name, case, differs, verdict, applies=True):
        """applies=False: at this case the change is the identity in exact arithmetic (it can move the last bit only)."""
        if not differs or not applies:
            self.identity[name].append(case)
            return
        self.differed[name] += 1
        if self.kinds[name] == "64":
            assert verdict.rejected.size > 0, f"mutant {name} not rejected at {case}"

    def finish(self, family):
        for name, n in self.differed.items():
            assert n > 0, f"{family}: mutant {name} is the identity at every case"
            if self.identity[name]:
                cases = self.identity[name]
                print(f"{family}: mutant {name} is the identity at {len(cases)} cases: {cases[:6]}{' ...' if len(cases) > 6 else ''}")


def _differs(a, b):
    return K.compare_bits(a, b).rejected.size > 0


# ---- fmaf -------------------------------------------------------------------------------------------------------------------
def _fma_exact(a, b, c):
    """fmaf by exact rational arithmetic: round(a b + c) to fp32, ties to even."""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        return F32(0)
    lo = F32(float(x))                                      # double rounding may be off by one neighbour: pick among three
    cands = [np.nextafter(lo, F32(-np.inf)), lo, np.nextafter(lo, F32(np.inf))]
    best = min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(v.view(np.uint32)) & 1))
    return best


def test_fma32_rounds_once():
    rng = np.random.default_rng(5)
    a = rng.standard_normal(3000).astype(F32)
    b = rng.standard_normal(3000).astype(F32)
    c = (rng.standard_normal(3000) * 10.0 ** rng.uniform(-8, 2, 3000)).astype(F32)
    # constructed ties: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 lies on a midpoint of fp32; c far below decides the side
    x = F32(1 + 2.0 ** -12)
    a[:4], b[:4] = x, x
    c[:4] = [2.0 ** -80, -(2.0 ** -80), 0.0, 2.0 ** -60]
    got = K.fma32(a, b, c)
    want = np.array([_fma_exact(*v) for v in zip(a, b, c)], dtype=F32)
    assert K.compare_bits(got, want).rejected.size == 0
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert _differs(naive[:4], want[:4]), "the constructed ties do round twice without the correction"


# ---- camera rays ------------------------------------------------------------------------------------------------------------
def _camera_cases():
    for H, W in K.FRAMES:
        for pose in K.POSES:
            if (H, W) == K.FRAMES[-1] and pose == "skewed":
                continue
            yield f"{H}x{W} {pose}", K.gen_camera(H, W, pose)
    for pose in K.POSES:
        yield f"shard {pose}", K.gen_camera(*K.SHARD_FRAME, pose, *K.SHARD_ROWS)


def test_rays():
    kinds = {"dy_no_negation": "64", "ij_swapped": "64", "row0_ignored": "64", "norm_plain_sum": "bits"}
    tally, worst = Mutants(kinds), 0.0
    for case, cam in _camera_cases():
        model = K.rays32(cam)
        R = (cam["row1"] - cam["row0"]) * cam["W"]
        assert model["ray_batch"].shape == (R, 11) and model["rays_d"].dtype == F32
        worst = max(worst, _accepted(K.compare_rays(model, cam), case))
        if "exact" in case:
            assert np.array_equal(model["rays_d"].astype(np.float64), K.rays64(cam)["rays_d"]), "exact camera: fp32 = float64"
        for name in kinds:
            if R > 10 ** 6 and name != "norm_plain_sum":
                continue                                    # the large frame adds nothing for the others
            mut = K.rays32(cam, name)
            diff = any(_differs(mut[k], model[k]) for k in model)
            tally.see(name, case, diff, K.compare_rays(mut, cam) if kinds[name] == "64" else None)
    tally.finish("rays")
    print(f"rays: fp32 model worst |err| / bound = {worst:.3f}")
    # the shard is the same rows of the full frame
    full, shard = K.rays32(K.gen_camera(*K.SHARD_FRAME, "look_at")), K.rays32(K.gen_camera(*K.SHARD_FRAME, "look_at", *K.SHARD_ROWS))
    W, (r0, r1) = K.SHARD_FRAME[1], K.SHARD_ROWS
    assert np.array_equal(full["ray_batch"][r0 * W:r1 * W], shard["ray_batch"])
    # the oracle's get_rays in double on the look-at camera
    cam = K.gen_camera(5, 7, "look_at")
    c2w = torch.from_numpy(cam["c2w"]).double()
    i, j = torch.meshgrid(torch.arange(7, dtype=torch.float64), torch.arange(5, dtype=torch.float64), indexing="xy")
    dirs = torch.stack([(i - cam["cx"]) / cam["fx"], -(j - cam["cy"]) / cam["fy"], -torch.ones_like(i)], -1)
    d = (dirs[..., None, :] * c2w[:3, :3]).sum(-1).reshape(-1, 3).numpy()
    assert np.allclose(K.rays64(cam)["rays_d"], d, rtol=1e-13, atol=1e-15)


# ---- sphere and quadratic ---------------------------------------------------------------------------------------------------
def _sphere_cases():
    for n in K.SIZES:
        for radius in K.SPHERE_RADII:
            if n > 10 ** 6 and radius != 2.0:
                continue
            yield n, radius


def test_sphere():
    kinds = {"roots_swapped": "64", "b_no_factor_2": "64", "c_from_dot": "bits", "radius_not_squared": "64"}
    tally, worst = Mutants(kinds), 0.0
    for n, radius in _sphere_cases():
        case = f"R={n} radius={radius}"
        o, d, random, rows = K.gen_sphere(n, radius, n + int(8 * radius))
        planted = K.sphere_planted(radius)
        assert len(rows) == min(n, len(planted)) and (n < 2 * len(planted) or (~random).sum() == 2 * len(planted))
        r = K.sphere64(o, d, radius)
        share = float((r["undecidable"] & random).sum()) / max(int(random.sum()), 1)
        assert share <= K.UNDECIDABLE_CAP, (case, share)
        t, pts = K.sphere32(o, d, radius)
        worst = max(worst, _accepted(K.compare_sphere(t, pts, o, d, radius), case))
        print(f"sphere {case}: undecidable share of the random rows {share:.2e}, real roots on {int(np.isfinite(t[random, 0]).sum())} of them")
        if n >= len(planted):
            for name in ("exact_tangent", "exact_tangent_z"):
                assert r["e_disc"][rows[name]] > 0 and r["undecidable"][rows[name]]
            assert np.array_equal(t[rows["exact_tangent"]], F32([0.75 * radius] * 2)), "the exact tangent's double root"
            assert np.array_equal(t[rows["exact_tangent_z"]], F32([0.375 * radius] * 2))
            assert np.array_equal(pts[rows["exact_tangent"]], F32([[0, radius, 0]] * 2))
            for k in K.TANGENT_K:                           # just inside hits, just outside misses (decided from k 2^-20 up to 64)
                inside, outside = t[rows[f"impact_-{k}"]], t[rows[f"impact_+{k}"]]
                if not r["undecidable"][rows[f"impact_-{k}"]]:
                    assert np.isfinite(inside).all() and inside[0] < inside[1]
                if not r["undecidable"][rows[f"impact_+{k}"]]:
                    assert np.isnan(outside).all()
            assert not r["undecidable"][rows["impact_-64"]] and not r["undecidable"][rows["impact_+64"]]
            assert np.isnan(t[rows["d_zero"]]).all() and np.isnan(t[rows["o_huge"]]).all() and np.isnan(t[rows["o_nan"]]).all()
            assert np.isnan(t[rows["parallel_miss"]]).all()
            ro = float(F32(radius)) / np.linalg.norm(d[rows["o_zero"]].astype(np.float64))
            assert np.allclose(t[rows["o_zero"]], [-ro, ro], rtol=1e-6)
            if radius == 1.0:                               # the reference's known answers
                assert np.array_equal(pts[rows["toward"]], F32([[-1, 0, 0], [1, 0, 0]]))
                assert np.array_equal(pts[rows["away"]], F32([[1, 0, 0], [-1, 0, 0]]))
                assert np.array_equal(pts[rows["inside"]], F32([[1, 0, 0], [-1, 0, 0]]))
                assert np.array_equal(pts[rows["on_sphere"]], F32([[1, 0, 0], [1, 0, 0]]))
                assert np.array_equal(pts[rows["on_sphere_inward"]], F32([[1, 0, 0], [-1, 0, 0]]))
        # the oracle in double, on the rows the oracle's own arithmetic decides
        fin = np.isfinite(o).all(1) & np.isfinite(d).all(1) & ~r["undecidable"]
        to, po = O.sphere_intersections(torch.from_numpy(o[fin]).double(), torch.from_numpy(d[fin]).double(),
                                        torch.tensor([float(F32(radius))], dtype=torch.float64))
        assert np.allclose(r["t"][fin], to.numpy(), rtol=1e-9, atol=1e-12, equal_nan=True)
        assert np.allclose(r["pts"][fin], po.numpy(), rtol=1e-9, atol=1e-9, equal_nan=True)
        for name in kinds:
            if n > 10 ** 6 and kinds[name] == "64":
                continue                                    # the large case adds nothing for these
            mt, mp = K.sphere32(o, d, radius, name)
            tally.see(name, case, _differs(mt, t) or _differs(mp, pts),
                      K.compare_sphere(mt, mp, o, d, radius) if kinds[name] == "64" else None)
    tally.finish("sphere")
    print(f"sphere: fp32 model worst |err| / bound = {worst:.3f}")


def test_quadratic():
    tally, worst = Mutants({"roots_swapped": "64"}), 0.0
    for n in K.SIZES:
        a, b, c, random, rows = K.gen_quadratic(n, n + 3)
        assert len(rows) == min(n, len(K.QUAD_PLANTED))
        r = K.quadratic64(a, b, c)
        share = float((r["undecidable"] & random).sum()) / max(int(random.sum()), 1)
        assert share <= K.UNDECIDABLE_CAP, (n, share)
        out = K.quadratic32(a, b, c)
        assert out.shape == (2, n)
        worst = max(worst, _accepted(K.compare_quadratic(out, a, b, c), f"n={n}"))
        print(f"quadratic n={n}: undecidable share of the random rows {share:.2e}")
        if n >= len(K.QUAD_PLANTED):
            assert out[0, rows["a_zero"]] == -np.inf and np.isnan(out[1, rows["a_zero"]])
            assert np.isnan(out[:, rows["disc_negative"]]).all() and np.isnan(out[:, rows["nan"]]).all()
            assert np.array_equal(out[:, rows["disc_zero"]], F32([-1, -1])) and r["undecidable"][rows["disc_zero"]]
            assert np.array_equal(out[:, rows["reference_double_root"]], F32([-0.5, -0.5]))
            assert np.array_equal(out[:, rows["reference_two_roots"]], F32([-1, -0.2]))
        fin = ~np.isnan(a) & ~r["undecidable"]
        ref = O.solve_quadratic(*(torch.from_numpy(v[fin]).double() for v in (a, b, c))).numpy()
        assert np.allclose(r["t"][fin].T, ref, rtol=1e-9, atol=0, equal_nan=True)
        mut = K.quadratic32(a, b, c, "roots_swapped")
        tally.see("roots_swapped", f"n={n}", _differs(mut, out), K.compare_quadratic(mut, a, b, c))
    tally.finish("quadratic")
    print(f"quadratic: fp32 model worst |err| / bound = {worst:.3f}")


# ---- placement --------------------------------------------------------------------------------------------------------------
def _oracle_place(mean, N, mode, std, noise=None):
    R = mean.shape[0]
    zero = torch.zeros(R, 3, dtype=torch.float64)
    nz = None if noise is None else torch.from_numpy(noise).double()
    with _double():
        return O.place_samples(zero, zero, torch.from_numpy(mean).double()[:, None], N, mode, float(F32(std)), nz)[1].numpy()


def test_uniform_placement():
    kinds = {"appended_no_merge": "64", "clip_before_merge": "64", "nan_mean_clipped": "64", "one_sided_linspace": "bits",
             "step_over_n_minus_1": "64"}
    tally, worst = Mutants(kinds), 0.0
    shapes = [(K.PLACE_R, N) for N in K.UNIFORM_N] + [K.UNIFORM_STRIDE4, K.UNIFORM_STRIDE]
    for R, N in shapes:
        for std in K.UNIFORM_STD if R == K.PLACE_R else (0.1,):
            case = f"R={R} N={N} std={std}"
            mean = K.gen_means(R, std, N)
            assert np.isnan(mean).sum() == 2 and np.isinf(mean).sum() == 4 and (mean == 2).any() and (mean == 6).any()
            z = K.place_uniform32(mean, N, std)
            assert z.shape == (R, N) and z.dtype == F32
            assert np.array_equal(np.isnan(z), np.broadcast_to(np.isnan(mean)[:, None], z.shape)), "a NaN mean gives NaN everywhere"
            ok = ~np.isnan(mean)
            assert (np.diff(z[ok], axis=1) >= 0).all() and z[ok].min() >= 2 and z[ok].max() <= 6
            worst = max(worst, _accepted(K.compare_uniform(z, mean, N, std), case))
            assert K.compare_bits(K.uniform_z_literal32(mean, N, std), z).rejected.size == 0, (case, "uniform_z against the sort")
            assert K.compare_bits(K.uniform_z_literal32(mean, N, std, clip=False), K.uniform_unclipped32(mean, N, std)).rejected.size == 0
            zj, zn = K.uniform_z_pair32(mean, N, std)
            assert K.compare_bits(zj, z[:, :-1]).rejected.size == 0 and K.compare_bits(zn, z[:, 1:]).rejected.size == 0, (case, "uniform_z_pair")
            if R == K.PLACE_R:
                fin = np.isfinite(mean)
                ref = _oracle_place(mean[fin], N, "uniform", std)
                z64 = K.place_uniform64(mean, N, std)[0]
                assert np.allclose(z64[fin], ref, rtol=1e-13, atol=1e-9 if mean[fin].max() > 1e6 else 1e-13), case
                for name in kinds:
                    mut = K.place_uniform32(mean, N, std, name)
                    tally.see(name, case, _differs(mut, z), K.compare_uniform(mut, mean, N, std))
    tally.finish("uniform")
    print(f"uniform placement: fp32 model worst |err| / bound = {worst:.3f}")


def test_gaussian_and_depth_only_placement():
    kinds = {"no_mean": "64", "no_sort": "64"}
    tally, worst = Mutants(kinds), 0.0
    for N in K.GAUSSIAN_N:
        for std in (0.1, 3.0):
            case = f"N={N} std={std}"
            mean, noise = K.gen_means(K.PLACE_R, std, 100 + N), K.gen_noise(K.PLACE_R, N, 200 + N)
            if N >= 4:
                assert np.isnan(noise[30:37]).any() and np.isinf(noise[30:37]).any() and (noise[37] == 0).all()
            z = K.place_gaussian32(mean, noise, N, std)
            assert z.shape == (K.PLACE_R, N)
            worst = max(worst, _accepted(K.compare_gaussian(z, mean, noise, N, std), case))
            nan = np.isnan(z)
            assert (nan[:, :-1] <= nan[:, 1:]).all(), "NaN sorts last"
            if N > 1:
                fin = np.isfinite(mean) & np.isfinite(noise).all(1)
                ref = _oracle_place(mean[fin], N, "gaussian", std, noise[fin])
                assert np.allclose(K.place_gaussian64(mean, noise, N, std)[0][fin], ref, rtol=1e-14, atol=0)
                for name in kinds:
                    mut = K.place_gaussian32(mean, noise, N, std, name)
                    tally.see(name, case, _differs(mut, z), K.compare_gaussian(mut, mean, noise, N, std))
    tally.finish("gaussian")
    print(f"gaussian placement: fp32 model worst |err| / bound = {worst:.3f}")


def test_placement_backward():
    kinds = {"exclusive_bounds": "64", "mask_from_clipped": "64"}
    tally, worst = Mutants(kinds), 0.0
    shapes = [(K.PLACE_R, N) for N in K.UNIFORM_N] + [K.BACKWARD_STRIDE]
    for R, N in shapes:
        for std in K.UNIFORM_STD if R == K.PLACE_R else (0.1,):
            case = f"R={R} N={N} std={std}"
            mean, dz = K.gen_means(R, std, N), K.gen_dz(R, N, 300 + N)
            assert np.isnan(dz).sum() == 3 and np.isinf(dz).sum() == 3 and (dz == 0).sum() >= 3
            got = K.place_backward32(K.MODE_UNIFORM, mean, dz, N, std)
            worst = max(worst, _accepted(K.compare_place_backward(got, K.MODE_UNIFORM, mean, dz, N, std), case))
            assert (got[np.isnan(mean)] == 0).all(), "a NaN mean passes nothing"
            if R == K.PLACE_R:
                # torch float64 autograd through the oracle on rows whose masks are decided and whose gradients are finite
                _, _, either = K.place_backward64(K.MODE_UNIFORM, mean, dz, N, std)
                ref, bound, _ = K.place_backward64(K.MODE_UNIFORM, mean, dz, N, std)
                fin = np.isfinite(mean) & np.isfinite(dz).all(1) & (bound < 1e-4) & ~either
                m = torch.from_numpy(mean[fin]).double()[:, None].requires_grad_(True)
                zero = torch.zeros(int(fin.sum()), 3, dtype=torch.float64)
                with _double():
                    O.place_samples(zero, zero, m, N, "uniform", float(F32(std)))[1].backward(torch.from_numpy(dz[fin]).double())
                assert np.allclose(m.grad.numpy()[:, 0], ref[fin], rtol=1e-12, atol=1e-12), case
                for name in kinds:
                    mut = K.place_backward32(K.MODE_UNIFORM, mean, dz, N, std, name)
                    # exclusive bounds differ only where a sample sits on 2 or 6 exactly: float64 decides that at std = 0 alone
                    tally.see(name, case, _differs(mut, got), K.compare_place_backward(mut, K.MODE_UNIFORM, mean, dz, N, std),
                              applies=name != "exclusive_bounds" or std == 0.0)
    for mode, N in ((K.MODE_GAUSSIAN, 33), (K.MODE_GAUSSIAN, 1), (K.MODE_DEPTH_ONLY, 7)):
        mean = K.gen_means(K.PLACE_R, 0.1, N)
        dz = K.gen_dz(K.PLACE_R, 1 if mode == K.MODE_DEPTH_ONLY else N, 400 + N)
        got = K.place_backward32(mode, mean, dz, N, 0.1)
        worst = max(worst, _accepted(K.compare_place_backward(got, mode, mean, dz, N, 0.1), f"mode {mode} N={N}"))
    tally.finish("placement backward")
    print(f"placement backward: fp32 model worst |err| / bound = {worst:.3f}")


# ---- coarse depths ----------------------------------------------------------------------------------------------------------
def test_coarse_depths():
    kinds = {"lindisp_interpolates_depth": "64", "jitter_upper_only": "64"}
    tally, worst = Mutants(kinds), 0.0
    shapes = [(K.COARSE_R, N) for N in K.COARSE_N] + [K.COARSE_STRIDE]
    for R, N in shapes:
        near, far, t_rand = K.gen_coarse(R, N, 500 + N)
        assert np.isnan(near).any() and (near == 0).any() and (near == far).any() and (near > far).any()
        assert (t_rand[0, :min(N, 3)] == K.T_RAND_PLANTED[:min(N, 3)]).all() and t_rand.max() < 1
        for lindisp in (0, 1):
            for tr in (None, t_rand):
                case = f"R={R} N={N} lindisp={lindisp} jitter={tr is not None}"
                z = K.coarse32(near, far, N, lindisp, tr)
                worst = max(worst, _accepted(K.compare_coarse(z, near, far, N, lindisp, tr), case))
                if R != K.COARSE_R:
                    continue
                z64 = K.coarse64(near, far, N, lindisp, tr)[0]
                fin = np.isfinite(near) & np.isfinite(far) & ((near > 0) | (lindisp == 0))
                with _double():
                    ref = O.coarse_z_vals(torch.from_numpy(near[fin]).double()[:, None], torch.from_numpy(far[fin]).double()[:, None],
                                          int(fin.sum()), N, bool(lindisp), perturb=0.0 if tr is None else 1.0,
                                          t_rand=None if tr is None else torch.from_numpy(tr[fin]).double()).numpy()
                assert np.allclose(z64[fin], ref, rtol=1e-12, atol=1e-13), case
                for name in kinds:
                    mut = K.coarse32(near, far, N, lindisp, tr, name)
                    # at N <= 2 only t = 0 and t = 1 occur: 1 / (1 / near) is near but for its last bit
                    tally.see(name, case, _differs(mut, z), K.compare_coarse(mut, near, far, N, lindisp, tr),
                              applies=name != "lindisp_interpolates_depth" or N >= 3)
    tally.finish("coarse depths")
    print(f"coarse depths: fp32 model worst |err| / bound = {worst:.3f}")


# ---- argmax -----------------------------------------------------------------------------------------------------------------
def test_argmax():
    kinds = {"last_index_on_ties": "64", "nan_ignored": "64", "start_value_wins": "64"}
    tally, worst = Mutants(kinds), 0.0
    for N in K.ARGMAX_N:
        for R in K.ARGMAX_R:
            if R > 257 and N not in (2, 65):
                continue
            case = f"R={R} N={N}"
            w, z, raw, rows = K.gen_argmax(R, N, 600 + N)
            assert len(rows) == min(R, len(K.ARGMAX_PLANTED)) and "all_negative" in rows
            got = K.argmax32(w, z, raw)
            worst = max(worst, _accepted(K.compare_argmax(got, w, z, raw), case))
            idx, _ = K.argmax_index32(w)
            assert got["max_w"][rows["all_negative"]] < 0, "a row of negatives does not return the start value 0"
            if R >= len(K.ARGMAX_PLANTED):
                assert idx[rows["all_zero"]] == 0 and idx[rows["minus_zero_first"]] == 0 and np.signbit(got["max_w"][rows["minus_zero_first"]])
                assert idx[rows["max_last"]] == N - 1 and (N < 2 or idx[rows["plus_inf"]] == N // 2)
                if N >= 3:
                    assert idx[rows["two_nans"]] == N // 3 and np.isnan(got["max_w"][rows["two_nans"]])
                if N >= 2:
                    assert idx[rows["duplicate_max"]] == min(5, N - 1) or N <= 6
            if R <= 257:                                    # the kernel's own order (lanes, then the butterfly) on the planted rows
                for r in sorted(set(rows.values()) | set(range(R - min(R, 12), R))):
                    assert K.argmax_wave(w[r]) == idx[r], (case, r)
            # torch.argmax on rows without NaN (torch leaves the choice among equals open on some builds: compare values)
            clean = ~np.isnan(w).any(1)
            ti = torch.from_numpy(w[clean]).argmax(1).numpy()
            assert np.array_equal(w[clean][np.arange(ti.size), ti], got["max_w"][clean])
            for name in kinds:
                mut = K.argmax32(w, z, raw, name)
                diff = any(_differs(mut[k], got[k]) for k in got)
                tally.see(name, case, diff, K.compare_argmax(mut, w, z, raw))
    tally.finish("argmax")
    print(f"argmax: fp32 model worst |err| / bound = {worst:.3f} (max_rgb against numpy's expf)")
