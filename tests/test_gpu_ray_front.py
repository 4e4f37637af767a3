"""The ray front end's small kernels on the GPU, entry by entry (tests/ray_front_reference.py holds the inputs, the fp32 models,
the float64 references, the error bounds and the comparators; tests/test_ray_front_host.py shows on the CPU that they reject every
mutant).  Called through the C ABI: ns_get_rays (every output NULL in turn, a row shard), ns_sphere_intersect and
ns_solve_quadratic, ns_place_samples (uniform through the float4 kernel and, with z offset by one float, through the generic one;
gaussian; depth_only; pts requested and not), ns_place_samples_backward, ns_coarse_z and ns_argmax_gather.

Every output is held twice: to the BITS of the fp32 model (max_rgb, which goes through expf, to the sigmoid bound instead), and
to the float64 reference inside the derived bound, so that a wrong model cannot hide a wrong kernel.  Every buffer a kernel writes
has a band of sentinels behind it (and, where the pointer is offset, in front of it) that must survive."""

import ctypes as C

import numpy as np
import pytest
import torch

import ray_front_reference as K
from nerf_sampling_amd import _lib
from train_kernels_reference import compare_bits, compare_points, points32

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = 7777.25
GUARD = 512                      # floats behind every buffer a kernel writes


def _ptr(t, offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + 4 * offset)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(n, front=0):
    """A device buffer of `front` + n + GUARD sentinels; the kernel is given the address of element `front`."""
    return torch.full((front + n + GUARD,), SENTINEL, device="cuda")


def _result(buf, n, front=0):
    host = buf.cpu().numpy()
    assert bool((host[:front] == F32(SENTINEL)).all()) and bool((host[front + n:] == F32(SENTINEL)).all()), "written outside the buffer"
    return host[front:front + n]


def _call(name, *args):
    lib = _lib.load()
    assert getattr(lib, name)(*args, _stream()) == 0, (name, lib.ns_last_error())


def _bits(got, want, what):
    v = compare_bits(got, want)
    assert v.rejected.size == 0, (what, "bits differ from the fp32 model", int(v.rejected.size), v.rejected[:8],
                                  np.ravel(got)[v.rejected[:4]], np.ravel(want)[v.rejected[:4]])


def _accept(verdict, what):
    print(f"{what}: worst |err| / bound = {verdict.worst:.3f}")
    assert verdict.rejected.size == 0, (what, int(verdict.rejected.size), verdict.rejected[:8], verdict.worst)


# ---- camera rays ------------------------------------------------------------------------------------------------------------
RAY_OUTPUTS = (("rays_o", 3), ("rays_d", 3), ("viewdirs", 3), ("ray_batch", 11))


def _get_rays(cam, want=("rays_o", "rays_d", "viewdirs", "ray_batch")):
    R = (cam["row1"] - cam["row0"]) * cam["W"]
    bufs = {k: _out(R * w) if k in want else None for k, w in RAY_OUTPUTS}
    c2w = np.ascontiguousarray(cam["c2w"], dtype=F32)
    _call("ns_get_rays", cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], C.c_void_p(c2w.ctypes.data), cam["row0"],
          cam["row1"], cam["near"], cam["far"], *(_ptr(bufs[k]) for k, _ in RAY_OUTPUTS))
    return {k: _result(bufs[k], R * w).reshape(R, w) for k, w in RAY_OUTPUTS if k in want}


def _camera_cases():
    cases = [(H, W, pose) for H, W in K.FRAMES for pose in K.POSES if not ((H, W) == K.FRAMES[-1] and pose == "skewed")]
    return cases


@pytest.mark.parametrize("H,W,pose", _camera_cases())
def test_get_rays(H, W, pose):
    cam = K.gen_camera(H, W, pose)
    got, model = _get_rays(cam), K.rays32(cam)
    for k in model:
        _bits(got[k], model[k], f"ns_get_rays {H}x{W} {pose} {k}")
    _accept(K.compare_rays(got, cam), f"ns_get_rays {H}x{W} {pose}")


@pytest.mark.parametrize("pose", K.POSES)
def test_get_rays_row_shard(pose):
    (H, W), (r0, r1) = K.SHARD_FRAME, K.SHARD_ROWS
    cam = K.gen_camera(H, W, pose, r0, r1)
    got, model, full = _get_rays(cam), K.rays32(cam), _get_rays(K.gen_camera(H, W, pose))
    for k in model:
        _bits(got[k], model[k], f"ns_get_rays shard {pose} {k}")
        _bits(got[k], full[k][r0 * W:r1 * W], f"ns_get_rays shard {pose} {k} against the full frame's rows")
    _accept(K.compare_rays(got, cam), f"ns_get_rays shard {pose}")


@pytest.mark.parametrize("H,W", [(5, 7), (3, 257)])
def test_get_rays_null_outputs(H, W):
    cam = K.gen_camera(H, W, "look_at")
    model = K.rays32(cam)
    for missing, _ in RAY_OUTPUTS:
        got = _get_rays(cam, tuple(k for k, _ in RAY_OUTPUTS if k != missing))
        assert missing not in got
        for k in got:
            _bits(got[k], model[k], f"ns_get_rays {H}x{W} without {missing}: {k}")
    for only, _ in RAY_OUTPUTS:
        _bits(_get_rays(cam, (only,))[only], model[only], f"ns_get_rays {H}x{W} {only} alone")


# ---- sphere and quadratic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,radius", [(n, r) for n in K.SIZES for r in K.SPHERE_RADII if n < 10 ** 6 or r == 2.0])
def test_sphere_intersect(n, radius):
    o, d, _, _ = K.gen_sphere(n, radius, n + int(8 * radius))
    od, dd = _dev(o), _dev(d)
    mt, mp = K.sphere32(o, d, radius)
    variants = ((True, True),) if n > 10 ** 6 else ((True, True), (True, False), (False, True))
    for want_t, want_p in variants:
        tb, pb = (_out(2 * n) if want_t else None), (_out(6 * n) if want_p else None)
        _call("ns_sphere_intersect", _ptr(od), _ptr(dd), n, radius, _ptr(tb), _ptr(pb))
        t = _result(tb, 2 * n) if want_t else None
        p = _result(pb, 6 * n) if want_p else None
        what = f"ns_sphere_intersect R={n} radius={radius} t={want_t} pts={want_p}"
        if want_t:
            _bits(t, mt, what + " t")
        if want_p:
            _bits(p, mp, what + " pts")
        _accept(K.compare_sphere(t, p, o, d, radius), what)
    assert compare_bits(od.cpu().numpy(), o).rejected.size == 0 and compare_bits(dd.cpu().numpy(), d).rejected.size == 0


@pytest.mark.parametrize("n", K.SIZES)
def test_solve_quadratic(n):
    a, b, c, _, _ = K.gen_quadratic(n, n + 3)
    ad, bd, cd, out = _dev(a), _dev(b), _dev(c), _out(2 * n)
    _call("ns_solve_quadratic", _ptr(ad), _ptr(bd), _ptr(cd), n, _ptr(out))
    got = _result(out, 2 * n).reshape(2, n)
    for dev, host in ((ad, a), (bd, b), (cd, c)):
        assert compare_bits(dev.cpu().numpy(), host).rejected.size == 0, "the coefficients are read-only"
    _bits(got, K.quadratic32(a, b, c), f"ns_solve_quadratic n={n}")
    _accept(K.compare_quadratic(got, a, b, c), f"ns_solve_quadratic n={n}")


# ---- placement --------------------------------------------------------------------------------------------------------------
def _place(mode, mean, noise, N, std, od=None, dd=None, offset=0):
    """(z [R, n], pts [R, n, 3] or None); offset: floats by which z is moved off its 16-byte alignment."""
    R = mean.shape[0]
    n = 1 if mode == K.MODE_DEPTH_ONLY else N
    zb = _out(R * n, front=offset)
    pb = _out(R * n * 3) if od is not None else None
    md, nd = _dev(mean), (None if noise is None else _dev(noise))
    assert zb.data_ptr() % 16 == 0
    _call("ns_place_samples", mode, _ptr(od), _ptr(dd), _ptr(md), _ptr(nd), R, N, std, _ptr(pb), _ptr(zb, offset))
    assert compare_bits(md.cpu().numpy(), mean).rejected.size == 0, "the means are read-only"
    assert nd is None or compare_bits(nd.cpu().numpy(), noise).rejected.size == 0, "the noise is read-only"
    z = _result(zb, R * n, front=offset).reshape(R, n)
    return z, (None if pb is None else _result(pb, R * n * 3).reshape(R, n, 3))


def _check_pts(pts, o, d, z, what):
    _bits(pts, points32(o, d, z), what + " pts")
    _accept(compare_points(pts, o, d, z), what + " pts")


def _uniform_case(R, N, std, with_pts, seed):
    what = f"ns_place_samples uniform R={R} N={N} std={std}"
    mean = K.gen_means(R, std, seed)
    model = K.place_uniform32(mean, N, std)
    o, d = K.gen_rays_od(R, seed + 1)
    od, dd = (_dev(o), _dev(d)) if with_pts else (None, None)
    z, pts = _place(K.MODE_UNIFORM, mean, None, N, std, od, dd)              # aligned: the float4 kernel where N % 4 == 0
    _bits(z, model, what)
    verdict = K.compare_uniform(z, mean, N, std)
    if with_pts:
        _check_pts(pts, o, d, z, what)
    if N % 4 == 0:
        z1, _ = _place(K.MODE_UNIFORM, mean, None, N, std, offset=1)         # one float off: the generic kernel
        _bits(z1, z, what + ": the generic kernel against the float4 kernel")
        _bits(z1, model, what + " (generic kernel)")
    return verdict


@pytest.mark.parametrize("N", K.UNIFORM_N)
def test_place_uniform(N):
    worst = 0.0
    for std in K.UNIFORM_STD:
        v = _uniform_case(K.PLACE_R, N, std, with_pts=std == 0.1, seed=N)
        assert v.rejected.size == 0, (N, std, v.rejected[:8], v.worst)
        worst = max(worst, v.worst)
    print(f"ns_place_samples uniform N={N}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("R,N", [K.UNIFORM_STRIDE4, K.UNIFORM_STRIDE])
def test_place_uniform_grid_stride(R, N):
    _accept(_uniform_case(R, N, 0.1, with_pts=False, seed=N), f"ns_place_samples uniform R={R} N={N}")


@pytest.mark.parametrize("N", K.GAUSSIAN_N)
def test_place_gaussian(N):
    R = K.PLACE_R
    for std in (0.1, 3.0):
        what = f"ns_place_samples gaussian N={N} std={std}"
        mean, noise = K.gen_means(R, std, 100 + N), K.gen_noise(R, N, 200 + N)
        o, d = K.gen_rays_od(R, N)
        with_pts = std == 0.1
        z, pts = _place(K.MODE_GAUSSIAN, mean, noise if N > 1 else None, N, std, *((_dev(o), _dev(d)) if with_pts else (None, None)))
        _bits(z, K.place_gaussian32(mean, noise, N, std), what)
        _accept(K.compare_gaussian(z, mean, noise, N, std), what)
        if with_pts:
            _check_pts(pts, o, d, z, what)


@pytest.mark.parametrize("with_pts", [False, True])
def test_place_depth_only(with_pts):
    R = K.PLACE_R
    mean = K.gen_means(R, 0.1, 7)
    o, d = K.gen_rays_od(R, 7)
    z, pts = _place(K.MODE_DEPTH_ONLY, mean, None, 7, 0.1, *((_dev(o), _dev(d)) if with_pts else (None, None)))    # N is ignored
    _bits(z, mean[:, None], "ns_place_samples depth_only")
    if with_pts:
        _check_pts(pts, o, d, z, "ns_place_samples depth_only")


def _backward(mode, mean, dz, N, std):
    R = mean.shape[0]
    md, gd, out = _dev(mean), _dev(dz), _out(R)
    _call("ns_place_samples_backward", mode, _ptr(md), R, N, std, _ptr(gd), _ptr(out))
    assert compare_bits(gd.cpu().numpy(), dz).rejected.size == 0, "the upstream gradient is read-only"
    return _result(out, R)


@pytest.mark.parametrize("N", K.UNIFORM_N)
def test_place_backward_uniform(N):
    worst = 0.0
    for std in K.UNIFORM_STD:
        mean, dz = K.gen_means(K.PLACE_R, std, N), K.gen_dz(K.PLACE_R, N, 300 + N)
        got = _backward(K.MODE_UNIFORM, mean, dz, N, std)
        _bits(got, K.place_backward32(K.MODE_UNIFORM, mean, dz, N, std), f"ns_place_samples_backward uniform N={N} std={std}")
        v = K.compare_place_backward(got, K.MODE_UNIFORM, mean, dz, N, std)
        assert v.rejected.size == 0, (N, std, v.rejected[:8], v.worst)
        worst = max(worst, v.worst)
    print(f"ns_place_samples_backward uniform N={N}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("mode,R,N", [(K.MODE_UNIFORM,) + K.BACKWARD_STRIDE, (K.MODE_GAUSSIAN, K.PLACE_R, 33), (K.MODE_GAUSSIAN, K.PLACE_R, 1),
                                      (K.MODE_DEPTH_ONLY, K.PLACE_R, 7)])
def test_place_backward_other(mode, R, N):
    mean = K.gen_means(R, 0.1, N)
    dz = K.gen_dz(R, 1 if mode == K.MODE_DEPTH_ONLY else N, (300 if mode == K.MODE_UNIFORM else 400) + N)
    got = _backward(mode, mean, dz, N, 0.1)
    what = f"ns_place_samples_backward mode={mode} R={R} N={N}"
    _bits(got, K.place_backward32(mode, mean, dz, N, 0.1), what)
    _accept(K.compare_place_backward(got, mode, mean, dz, N, 0.1), what)


# ---- coarse depths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N", [(K.COARSE_R, N) for N in K.COARSE_N] + [K.COARSE_STRIDE])
def test_coarse_z(R, N):
    near, far, t_rand = K.gen_coarse(R, N, 500 + N)
    nd, fd, td = _dev(near), _dev(far), _dev(t_rand)
    for lindisp in (0, 1):
        for tr, trd in ((None, None), (t_rand, td)):
            what = f"ns_coarse_z R={R} N={N} lindisp={lindisp} jitter={tr is not None}"
            out = _out(R * N)
            _call("ns_coarse_z", _ptr(nd), _ptr(fd), R, N, lindisp, _ptr(trd), _ptr(out))
            got = _result(out, R * N).reshape(R, N)
            _bits(got, K.coarse32(near, far, N, lindisp, tr), what)
            _accept(K.compare_coarse(got, near, far, N, lindisp, tr), what)


# ---- argmax -----------------------------------------------------------------------------------------------------------------
ARGMAX_OUTPUTS = (("max_z", 1), ("max_w", 1), ("max_rgb", 3))


def _argmax(wd, zd, rawd, R, N, want):
    bufs = {k: _out(R * n) if k in want else None for k, n in ARGMAX_OUTPUTS}
    _call("ns_argmax_gather", _ptr(wd), _ptr(zd), _ptr(rawd), R, N, *(_ptr(bufs[k]) for k, _ in ARGMAX_OUTPUTS))
    return {k: _result(bufs[k], R * n).reshape((R, 3) if n == 3 else (R,)) for k, n in ARGMAX_OUTPUTS if k in want}


@pytest.mark.parametrize("R,N", [(R, N) for N in K.ARGMAX_N for R in K.ARGMAX_R if R <= 257 or N in (2, 65)])
def test_argmax_gather(R, N):
    w, z, raw, _ = K.gen_argmax(R, N, 600 + N)
    wd, zd, rawd = _dev(w), _dev(z), _dev(raw)
    model = K.argmax32(w, z, raw)
    what = f"ns_argmax_gather R={R} N={N}"
    variants = [("max_z", "max_w", "max_rgb"), ("max_w", "max_rgb"), ("max_z", "max_rgb"), ("max_z", "max_w"), ("max_w",)]
    for want in variants if R <= 257 else variants[:1]:
        no_raw = "max_rgb" not in want
        got = _argmax(wd, zd if "max_z" in want else None, None if no_raw else rawd, R, N, want)
        for k in ("max_z", "max_w"):
            if k in got:
                _bits(got[k], model[k], f"{what} {want}: {k}")
        _accept(K.compare_argmax(got, w, z, raw), f"{what} {want}")
    for dev, host in ((wd, w), (zd, z), (rawd, raw)):
        assert compare_bits(dev.cpu().numpy(), host).rejected.size == 0, "inputs are read-only"
