"""GPU parity tests, kernel level: every C-ABI entry point against the golden vectors captured from
the reference and against the CPU oracle on the same seeded inputs (run with -m gpu on an MI355X).

Tolerances are stated per check.  fp32 paths are held to ~1e-6..1e-5 (different summation order /
libm only); the bf16/fp16 MFMA paths are held to operand-rounding-sized errors.

The DepthNet forward's exact checks -- every kernel instantiation against the float64 chain on exactly representable
networks and rays, 8 * 2^-24 * max(|near|, |far|) on every ray -- live in tests/test_gpu_exact_depthnet.py; the gates on
the DepthNet below are the looser ones for ordinary weights.

The ray front end's exact checks -- ns_get_rays, ns_sphere_intersect, ns_solve_quadratic, ns_place_samples, ns_coarse_z,
ns_place_samples_backward and ns_argmax_gather bit for bit against fp32 models of their statements and inside derived bounds
against float64, at grid-stride sizes, on both placement kernels and on adversarial means, tangent rays and NaN / inf rows -- live
in tests/test_gpu_ray_front.py; sections a1, a2, a5, a11 and test_argmax_gather below are the golden-file checks at 1e-6..2e-5.
"""

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

T = torch.from_numpy


def dev(x):
    return (T(x) if isinstance(x, np.ndarray) else x).float().cuda()


def close(a, b, rtol=1e-5, atol=1e-6, msg=""):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, equal_nan=True, err_msg=msg)


@pytest.fixture(scope="module")
def ops():
    from nerf_sampling_amd import ops as _ops

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


# ---- a1 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["64", "5x7"])
def test_get_rays(ops, golden, tag):
    g = golden(f"rays_{tag}")
    H, W = int(g["H"]), int(g["W"])
    o, d, v, b = ops.get_rays(H, W, g["K"], g["c2w"], near=2.0, far=6.0, want_batch=True)
    close(b, g["ray_batch"], 2e-6, 1e-7)       # fp32 mul/add in the reference's order; norm differs by <= 1 ulp
    close(o, g["ray_batch"][:, 0:3], 0, 0)
    close(d, g["ray_batch"][:, 3:6], 2e-6, 1e-7)
    # row sharding: rows [r0, r1) equal the same rows of the full frame (bit exact)
    r0, r1 = 1, min(H, 4)
    o2, d2, v2 = ops.get_rays(H, W, g["K"], g["c2w"], row0=r0, row1=r1)
    assert torch.equal(d2, d[r0 * W : r1 * W]) and torch.equal(v2, v[r0 * W : r1 * W])


def test_prepare_rays_staticcam(ops, golden):
    """prepare_rays(c2w, c2w_staticcam) against the reference (nerf_utils.py:172-176): columns 8..10 are the view directions
    of c2w, columns 0..5 the rays of the static camera; origins bit-exact, directions to 2e-6 as test_get_rays."""
    from nerf_sampling_amd import nerf_utils

    g = golden("staticcam")
    H, W = int(g["H"]), int(g["W"])
    batch, o, d, sh = nerf_utils.prepare_rays(c2w=T(g["c2w"]), c2w_staticcam=T(g["c2w_staticcam"]), use_viewdirs=True,
                                              ndc=False, H=H, W=W, K=g["K"], near=2.0, far=6.0, rays=None)
    assert tuple(sh) == (H, W, 3) and batch.shape == (H * W, 11)
    close(batch[:, 0:3], g["ray_batch"][:, 0:3], 0, 0)
    close(batch[:, 3:6], g["ray_batch"][:, 3:6], 0, 2e-6)
    close(batch[:, 6:8], g["ray_batch"][:, 6:8], 0, 0)
    close(batch[:, 8:11], g["ray_batch"][:, 8:11], 0, 2e-6)
    assert not np.allclose(g["ray_batch"][:, 8:11], g["ray_batch"][:, 3:6] / np.linalg.norm(g["ray_batch"][:, 3:6], axis=-1, keepdims=True), atol=1e-3)
    close(o, g["rays_o"].reshape(-1, 3), 0, 0)


def test_get_rays_empty(ops, golden):
    g = golden("rays_5x7")
    o, d, v = ops.get_rays(5, 7, g["K"], g["c2w"], row0=2, row1=2)
    assert o.shape == (0, 3)


# ---- a2 -------------------------------------------------------------------------------------------
def test_sphere(ops, golden):
    g = golden("sphere")
    t, p = ops.sphere_intersect(dev(g["known_o"]), dev(g["known_d"]), 1.0)
    close(t, g["known_t"], 1e-6, 1e-6)
    close(p, g["known_p"], 1e-6, 1e-6)
    t, p = ops.sphere_intersect(dev(g["o"]), dev(g["d"]), 2.0)
    assert np.isnan(g["t"]).sum() == np.isnan(t.cpu().numpy()).sum()
    close(t, g["t"], 2e-5, 2e-6)   # the discriminant cancels: b^2 - 4ac with fused vs unfused products
    close(p, g["p"], 2e-5, 2e-5)
    q = ops.solve_quadratic(dev(g["qa"]), dev(g["qb"]), dev(g["qc"]))
    close(q, g["qs"], 1e-6, 1e-7)


@pytest.mark.parametrize(
    "o,d,expected",
    [  # the reference's own known answers, tests.py:250-331, sphere radius 1
        ([-3.0, 0, 0], [1.0, 0, 0], [[-1.0, 0, 0], [1.0, 0, 0]]),
        ([-3.0, 0, 0], [0.0, 2, 0], [[float("nan")] * 3] * 2),
        ([-3.0, 0, 0], [-1.0, 0, 0], [[1.0, 0, 0], [-1.0, 0, 0]]),
        ([-3.0, 1, 0], [1.0, 0, 0], [[0.0, 1, 0], [0.0, 1, 0]]),
        ([1.0, 0, 0], [0.0, 1, 0], [[1.0, 0, 0], [1.0, 0, 0]]),
        ([0.0, 0, 0], [-1.0, 0, 0], [[1.0, 0, 0], [-1.0, 0, 0]]),
        ([1.0, 0, 0], [-1.0, 0, 0], [[1.0, 0, 0], [-1.0, 0, 0]]),
    ],
)
def test_sphere_known_answers(ops, o, d, expected):
    from nerf_sampling_amd.utils import find_intersection_points_with_sphere

    t, p = find_intersection_points_with_sphere(torch.tensor([o]).cuda(), torch.tensor([d]).cuda(),
                                                torch.tensor([1.0]))
    assert p.shape == (1, 2, 3)
    close(p[0], np.array(expected), 1e-6, 1e-6)


def test_quadratic_known_answers(ops):
    from nerf_sampling_amd.utils import solve_quadratic_equation

    nan = float("nan")
    a = torch.tensor([[1.0, 4, 5], [1, 4, 5]]).cuda(); b = torch.tensor([[1.0, 4, 6], [1, 4, 6]]).cuda()
    out = solve_quadratic_equation(a, b, torch.ones(2, 3).cuda())
    close(out, np.array([[[nan, -0.5, -1], [nan, -0.5, -1]], [[nan, -0.5, -0.2], [nan, -0.5, -0.2]]]))


# ---- a3 -------------------------------------------------------------------------------------------
def test_posenc(ops, golden):
    g = golden("posenc")
    close(ops.posenc(dev(g["x3"]), 10), g["e63"], 0, 2e-6)     # |arg| up to 3072 rad; libm vs sleef <= 2 ulp
    close(ops.posenc(dev(g["x3"]) / 6.0, 4), g["e27"], 0, 1e-6)
    close(ops.posenc(dev(g["x6"]), 10), g["e126"], 0, 2e-6)


# ---- a5 -------------------------------------------------------------------------------------------
def test_place_samples(ops, golden):
    g = golden("place_samples")
    o, d, mean = dev(g["o"]), dev(g["d"]), dev(g["mean"]).reshape(-1)
    for n_s in (2, 3, 32, 64):
        for std in (0.01, 0.1):
            pts, z = ops.place_samples(o, d, mean, n_s, "uniform", std)
            close(z, g[f"uniform_n{n_s}_s{std}_z"], 1e-6, 1e-6)
            if n_s <= 3:
                close(pts, g[f"uniform_n{n_s}_s{std}_pts"], 1e-6, 2e-6)
    pts, z = ops.place_samples(o, d, mean, 32, "depth_only", 0.1)
    assert z.shape == (256, 1)
    close(z, g["depth_only_z"], 0, 0)
    close(pts, g["depth_only_pts"], 1e-6, 1e-6)
    pts, z = ops.place_samples(o, d, mean, 32, "gaussian", 0.1, noise=dev(g["gaussian_noise"]))
    close(z, g["gaussian_n32_z"], 1e-6, 1e-6)
    close(pts[:8], g["gaussian_n32_pts_first8"], 1e-6, 2e-6)
    assert (z[:, 1:] >= z[:, :-1]).all()
    # NaN mean (ray missed the sphere) stays NaN in every mode
    nan_mean = torch.full((4,), float("nan")).cuda()
    for mode in ("uniform", "gaussian", "depth_only"):
        _, zz = ops.place_samples(o[:4], d[:4], nan_mean, 8, mode, 0.1)
        assert torch.isnan(zz).all()


# ---- a8 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 32, 64, 192])
@pytest.mark.parametrize("wb", [True, False])
def test_raw2outputs(ops, golden, N, wb):
    g = golden("raw2outputs")
    rgb, disp, acc, depth, alphas, weights = ops.raw2outputs(dev(g[f"N{N}_raw"]), dev(g[f"N{N}_z"]),
                                                             dev(g[f"N{N}_rays_d"]), None, wb)
    p = f"N{N}_wb{int(wb)}_"
    close(alphas, g[p + "alphas"], 2e-6, 1e-7)
    close(weights, g[p + "weights"], 3e-5, 1e-7)   # scan vs sequential cumprod: <= N ulp
    close(acc, g[p + "acc"], 1e-5, 1e-6)
    close(rgb, g[p + "rgb"], 1e-5, 2e-6)
    close(depth, g[p + "depth"], 1e-5, 2e-6)
    close(disp, g[p + "disp"], 2e-5, 1e-6)


def test_compositing_on_the_transcendental_unit_keeps_its_absolute_error_bound(ops):
    """ns_composite_ray.h evaluates exp on v_exp_f32 (the argument times log2 e, rounded once) and 1 / x on v_rcp_f32.  What
    compositing uses are 1 - exp(-s) and 1 / (1 + exp(-x)): their ABSOLUTE error stays at the rounding of the fp32 result for
    every argument -- checked here against float64 over the whole range the kernels can see, far beyond what
    the golden fixtures contain: sigma * dist from 1e-6 to 1e4, colour logits from -60 to 60."""
    R = 4096
    gen = torch.Generator().manual_seed(5)
    # two samples per ray: sample 0 opaque (alpha = 1 exactly), so rgb = sigmoid(raw[0, :3]); sample 0's alpha probes 1 - exp(-s)
    x = (torch.rand(R, 3, generator=gen) * 2 - 1) * 60.0
    s = 10.0 ** (torch.rand(R, generator=gen) * 10 - 6)                       # sigma * dist (dist = 1: z = [2, 3], unit d)
    raw = torch.zeros(R, 2, 4)
    raw[:, 0, :3] = x
    raw[:, 0, 3] = 1e6
    z = torch.tensor([[2.0, 3.0]]).expand(R, 2).contiguous()
    d = torch.tensor([[0.0, 0.0, 1.0]]).expand(R, 3).contiguous()
    rgb = ops.raw2outputs(raw.cuda(), z.cuda(), d.cuda(), None, False)[0].cpu().double()
    err_c = (rgb - torch.sigmoid(x.double())).abs().max().item()
    raw2 = torch.zeros(R, 2, 4)
    raw2[:, 0, 3] = s
    alphas = ops.raw2outputs(raw2.cuda(), z.cuda(), d.cuda(), None, False)[4].cpu().double()
    err_a = (alphas[:, 0] - (1.0 - torch.exp(-s.double()))).abs().max().item()
    print(f"compositing on the transcendental unit: max |sigmoid err| {err_c:.2e}, max |alpha err| {err_a:.2e}")
    assert err_c < 1.5e-7 and err_a < 1.5e-7, (err_c, err_a)


def test_raw2outputs_noise_and_trainer_signature(ops, golden):
    from nerf_sampling_amd.trainers import DepthNetTrainer

    g = golden("raw2outputs")
    noise = dev(g["N32_noise"]) * 0.5
    rgb, _, _, _, _, w = ops.raw2outputs(dev(g["N32_raw"]), dev(g["N32_z"]), dev(g["N32_rays_d"]), noise, True)
    close(rgb, g["N32_noisy_rgb"], 1e-5, 2e-6)
    close(w, g["N32_noisy_weights"], 3e-5, 1e-7)
    tr = DepthNetTrainer(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="",
                         half_res=True, white_bkgd=True)
    res = tr.raw2outputs(dev(g["N32_raw"]), dev(g["N32_z"]), dev(g["N32_rays_d"]), raw_noise=0.7, white_bkdg=False)
    assert len(res) == 7                                  # misspelled kwargs are swallowed (reference quirk)
    close(res[0], g["N32_wb1_rgb"], 1e-5, 2e-6)
    close(res[4], g["N32_raw"][..., 3], 0, 0)


# ---- a11 pieces -----------------------------------------------------------------------------------
def test_sample_pdf(ops, golden):
    g = golden("sample_pdf")
    det = ops.sample_pdf(dev(g["bins"]), dev(g["weights"]), 128, None)
    rnd = ops.sample_pdf(dev(g["bins"]), dev(g["weights"]), 128, dev(g["u"]))
    # the inverse CDF is continuous in u except where a bin's mass is below the reference's 1e-5
    # threshold; allow a handful of such samples to land in the neighbouring bin
    for mine, exp in ((det, g["det"]), (rnd, g["rnd"])):
        err = np.abs(mine.cpu().numpy() - exp)
        assert np.mean(err > 2e-5) < 2e-3, float(np.mean(err > 2e-5))
        assert np.median(err) < 1e-6


def test_sort_rows(ops):
    gen = torch.Generator().manual_seed(3)
    for n in (1, 2, 63, 64, 65, 192, 500):
        x = torch.randn(37, n, generator=gen)
        close(ops.sort_rows(x.cuda()), torch.sort(x, -1).values, 0, 0)
    x = torch.tensor([[3.0, float("nan"), 1.0, 2.0]])
    out = ops.sort_rows(x.cuda()).cpu()
    assert out[0, :3].tolist() == [1.0, 2.0, 3.0] and torch.isnan(out[0, 3])


def test_importance_z_and_coarse_z(ops, golden):
    g = golden("hierarchical")
    rb = T(g["ray_batch"])
    for lindisp in (True, False):
        z = ops.coarse_z(rb[:, 6].cuda(), rb[:, 7].cuda(), 64, lindisp)
        exp = O.coarse_z_vals(rb[:, 6:7], rb[:, 7:8], rb.shape[0], 64, lindisp)
        close(z, exp, 2e-6, 1e-6)
    z = ops.coarse_z(rb[:, 6].cuda(), rb[:, 7].cuda(), 64, True, dev(g["perturb_t_rand"]))
    exp = O.coarse_z_vals(rb[:, 6:7], rb[:, 7:8], rb.shape[0], 64, True, 1.0, T(g["perturb_t_rand"]))
    close(z, exp, 2e-6, 1e-6)
    # importance_z == sort(cat[z, sample_pdf(z_mid, w[1:-1])]) of the oracle
    zc = exp
    w = torch.rand(rb.shape[0], 64, generator=torch.Generator().manual_seed(5)) ** 3
    z_mid = 0.5 * (zc[..., 1:] + zc[..., :-1])
    ref = torch.sort(torch.cat([zc, O.sample_pdf(z_mid, w[..., 1:-1], 128, det=True)], -1), -1).values
    mine = ops.importance_z(zc.cuda(), w.cuda(), 128, None)
    err = (mine.cpu() - ref).abs().numpy()
    assert np.mean(err > 2e-5) < 2e-3 and np.median(err) < 1e-6
    assert (mine[:, 1:] >= mine[:, :-1]).all()


@pytest.mark.parametrize("Nc,Nf,random_u", [(64, 128, True), (8, 16, False), (8, 16, True), (32, 64, True),
                                             (33, 95, False), (64, 192, True), (96, 200, True), (3, 5, False)])
def test_importance_z_shapes(ops, Nc, Nf, random_u):
    """Both kernels behind ns_importance_z (one wave per ray in registers for Nc <= 64 and Nc + Nf <= 256, the LDS
    version beyond) against the oracle, with sorted (deterministic) and unsorted (random u) samples."""
    gen = torch.Generator().manual_seed(100 * Nc + Nf)
    R = 257
    zc = torch.sort(2.0 + 4.0 * torch.rand(R, Nc, generator=gen), -1).values
    w = torch.rand(R, Nc, generator=gen) ** 3
    w[5] = 0.0                                      # all mass from the 1e-5 floor
    u = torch.rand(R, Nf, generator=gen) if random_u else None
    z_mid = 0.5 * (zc[..., 1:] + zc[..., :-1])
    ref = torch.sort(torch.cat([zc, O.sample_pdf(z_mid, w[..., 1:-1], Nf, det=True, u=u)], -1), -1).values
    mine = ops.importance_z(zc.cuda(), w.cuda(), Nf, None if u is None else u.cuda()).cpu()
    assert mine.shape == (R, Nc + Nf) and torch.isfinite(mine).all()
    assert (mine[:, 1:] >= mine[:, :-1]).all()
    err = (mine - ref).abs().numpy()
    assert np.mean(err > 2e-5) < 5e-3 and np.median(err) < 1e-6
    if not random_u:
        # the wave kernel sorts deterministic draws with ONE merge stage when the coarse depths ascend and the new samples do too;
        # rows that do not (here: descending coarse depths) must take the full network and still come out as torch.sort gives them
        zd = zc.flip(-1).contiguous()
        z_mid = 0.5 * (zd[..., 1:] + zd[..., :-1])
        ref = torch.sort(torch.cat([zd, O.sample_pdf(z_mid, w[..., 1:-1], Nf, det=True)], -1), -1).values
        mine = ops.importance_z(zd.cuda(), w.cuda(), Nf, None).cpu()
        assert (mine[:, 1:] >= mine[:, :-1]).all()
        err = (mine - ref).abs().numpy()
        assert np.mean(err > 2e-5) < 5e-3 and np.median(err) < 1e-6


def test_argmax_gather(ops):
    gen = torch.Generator().manual_seed(8)
    w = torch.rand(50, 192, generator=gen); z = torch.rand(50, 192, generator=gen); raw = torch.randn(50, 192, 4, generator=gen)
    w[3] = 0.0                       # ties -> first index
    w[4, 7] = w[4, 100] = 2.0        # duplicated maximum -> first
    mz, mw, mrgb = ops.argmax_gather(w.cuda(), z.cuda(), raw.cuda())
    idx = w.argmax(dim=1, keepdim=True)
    close(mz, torch.gather(z, 1, idx), 0, 0)
    close(mw, torch.gather(w, 1, idx), 0, 0)
    close(mrgb, torch.sigmoid(torch.gather(raw[..., :3], 1, idx.unsqueeze(-1).expand(-1, 1, 3)).squeeze(1)), 1e-6, 1e-7)


# ---- a6/a7 NeRF MLP --------------------------------------------------------------------------------
def _mlp_err(ops, gpu_modules, golden, scene, dtype):
    g = golden("nerf_mlp")
    m = gpu_modules(scene)
    out = {}
    for which in ("coarse", "fine"):
        raw = ops.nerf_forward(m[which].packed(dtype), dev(g["pts"]), dev(g["viewdirs"]))
        out[which] = (raw.cpu().numpy(), g[f"raw_{scene}_{which}"])
    return out


@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth"])
@pytest.mark.parametrize("dtype", ["f32", "f16x3"])
def test_nerf_mlp_f32(ops, gpu_modules, golden, scene, dtype):
    """fp32 MFMA path: exact-fp32 products, k-ordered fma chain; only summation order differs from the CPU GEMM.
    f16x3 (split fp16 operands, three MFMAs per product term on the 16x16x32 engine) is held to the SAME gate."""
    for which, (mine, exp) in _mlp_err(ops, gpu_modules, golden, scene, dtype).items():
        scale = np.abs(exp).max(axis=(0, 1))             # per output channel (rgb ~ O(1), sigma ~ O(100))
        err = np.abs(mine - exp).max(axis=(0, 1)) / scale
        print(f"nerf_mlp {dtype} {scene} {which}: max err/scale {err}")
        assert (err < 2e-5).all(), (which, err)


@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth"])
@pytest.mark.parametrize("dtype,tol", [("bf16", 2.2e-2), ("f16", 2.7e-3)])   # measured rms/scale <= 7.1e-3 / 8.7e-4 (round 2)
def test_nerf_mlp_16bit(ops, gpu_modules, golden, scene, dtype, tol):
    """16-bit operands, fp32 accumulation: error is operand rounding (2^-9 bf16, 2^-12 fp16) through ~10 layers."""
    for which, (mine, exp) in _mlp_err(ops, gpu_modules, golden, scene, dtype).items():
        scale = np.abs(exp).max(axis=(0, 1))
        rms = np.sqrt(((mine - exp) ** 2).mean(axis=(0, 1))) / scale
        print(f"nerf_mlp_16bit {scene} {which} {dtype}: rms/scale {rms}")
        assert (rms < tol).all(), (which, dtype, rms)


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f16x3"])
def test_hand_scheduled_layers_are_bit_identical_to_the_compiled_ones(ops, gpu_modules, dtype):
    """The production network (8 x 256, skips = [4]) takes the kernel whose hidden layers are the generated asm streams
    (csrc/ns_ob16_asm.inc, tools/gen_ob16_asm.py); the diagnostic switch generic_kernels (ns_debug_set) sends the same call
    through the compiler-scheduled kernel.  Both issue the same MFMAs in the same order per accumulator, so raw must agree BIT FOR BIT -- a hazard or a
    wrong register in the hand-written stream shows here.  Ragged counts, several groups per workgroup, both input forms."""
    m = gpu_modules("lego_synth")
    net = m["fine"]
    assert (net.D, net.W, list(net.skips)) == (8, 256, [4])
    packed = net.packed(dtype)
    gen = torch.Generator().manual_seed(5)
    for R, N in ((1, 1), (5, 7), (300, 64), (4100, 64), (2500, 192)):
        pts = ((torch.rand(R, N, 3, generator=gen) * 2 - 1) * 2.5).cuda()
        view = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1).cuda()
        with ops.debug_switch(generic_kernels=1):
            ref = ops.nerf_forward(packed, pts, view)
            torch.cuda.synchronize()
        # the 16-bit production kernel exists with four and with five tiles per wave (chosen per launch; the switch
        # prod_tiles forces one): a sample's arithmetic does not depend on the tile it rides in, so both must give the same bits
        for tiles in ((4, 5, 0) if dtype != "f16x3" else (0,)):
            with ops.debug_switch(prod_tiles=tiles):
                for _ in range(2):      # twice: the ring phase at the start of a launch does not depend on the previous one
                    got = ops.nerf_forward(packed, pts, view)
                    torch.cuda.synchronize()
                    assert torch.isfinite(got).all()
                    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (dtype, tiles, R, N, (got - ref).abs().max().item())


@pytest.mark.parametrize("dtype", ["f16", "f16x3"])
def test_depthnet_generated_layers_are_bit_identical_to_the_compiled_ones(ops, gpu_modules, dtype):
    """The production DepthNet (10 x 256 trunk) on fp16 operands -- what the bf16 compute dtype pairs the field with -- and on
    split fp16 operands (the PSNR guard's DepthNet) runs its ten LeakyReLU layers as generated streams (tools/gen_ob16_asm.py,
    act = "leaky"); the switch generic_kernels sends the same call through the compiled layers (fp16: the same packed
    v_pk_mul_f16 / v_pk_max_f16 LeakyReLU; f16x3: the same fp32 max and the same hi / lo split, whose remainder the streams
    form with one mixed-precision fma): depths must agree bit for bit.  Ragged ray counts, several groups per workgroup; rays
    that miss the sphere (NaN) included."""
    m = gpu_modules("lego_synth")
    dn = m["depth"]
    assert list(dn.cat_hidden_sizes) == [256] * 10
    packed = dn.packed(dtype)
    gen = torch.Generator().manual_seed(17)
    for R in (1, 77, 4096, 70001):
        o = (torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1) * 4.0).cuda()
        d = (-o / 4.0 + 0.25 * torch.randn(R, 3, generator=gen).cuda()).contiguous()
        with ops.debug_switch(generic_kernels=1):
            ref = ops.depthnet_forward(packed, o, d)
            torch.cuda.synchronize()
        for _ in range(2):
            got = ops.depthnet_forward(packed, o, d)
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (R, (got - ref).abs().nan_to_num().max().item())
        hit = torch.isfinite(ref)
        assert hit.float().mean() > 0.3 and bool(((ref[hit] >= 2.0) & (ref[hit] <= 6.0)).all())


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f16x3"])
def test_hand_scheduled_layers_other_input_forms(ops, gpu_modules, dtype):
    """The same bit-for-bit comparison for the other two input forms of the production kernels: rays (o, d, z) with the
    points formed in-kernel -- what the frame renderer launches -- and the pre-embedded [M, 90] rows of NeRF.forward
    (their own kernel instantiations, four and five tiles)."""
    m = gpu_modules("lego_synth")
    packed = m["fine"].packed(dtype)
    gen = torch.Generator().manual_seed(9)
    R, N = 1300, 64
    o = (torch.randn(R, 3, generator=gen) * 0.5).cuda()
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1).cuda()
    z = (torch.rand(R, N, generator=gen) * 4 + 2).sort(dim=-1).values.cuda()
    view = d.clone()
    pts = (o[:, None] + d[:, None] * z[..., None]).cpu()
    x90 = torch.cat([O.posenc(pts.reshape(-1, 3), 10), O.posenc(view.cpu()[:, None].expand(pts.shape).reshape(-1, 3), 4)], -1).cuda()

    def both():
        return ops.nerf_forward_rays(packed, o, d, z, view), ops.nerf_forward_embedded(packed, x90)

    with ops.debug_switch(generic_kernels=1):
        ref = both()
        torch.cuda.synchronize()
    for tiles in ((4, 5) if dtype != "f16x3" else (0,)):
        with ops.debug_switch(prod_tiles=tiles):
            got = both()
            torch.cuda.synchronize()
        for a, b in zip(got, ref):
            assert torch.isfinite(a).all()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (dtype, tiles, (a - b).abs().max().item())


@pytest.mark.parametrize("D,W,skip", [(2, 128, -1), (3, 256, 0), (5, 128, 3), (6, 256, 4), (7, 128, 1), (8, 256, -1), (9, 256, 4)])
def test_nerf_mlp_shapes_16bit_vs_fp32(ops, D, W, skip):
    """Program logic of the 16x16x32 kernel (two layers per trip + odd tail, skip at any depth or none, both widths,
    ragged / tiny sample counts) against the k-major fp32 kernel, a different engine with a different stream layout:
    agreement within 16-bit operand rounding."""
    from nerf_sampling_amd.run_nerf_helpers import NeRF
    from nerf_sampling_amd import synthetic

    skips = () if skip < 0 else (skip,)
    params = synthetic.make_nerf_params(seed=100 * D + skip + 7, D=D, W=W, skips=skips, hidden_gain=6 ** 0.5,
                                        sigma_gain=30.0, spectral_decay=True)
    net = NeRF(D=D, W=W, input_ch=63, input_ch_views=27, output_ch=5, skips=list(skips), use_viewdirs=True)
    net.load_state_dict(params)
    net = net.cuda()
    gen = torch.Generator().manual_seed(D * 31 + W)
    for R, N in ((1, 1), (3, 5), (37, 64), (130, 33)):
        pts = (torch.rand(R, N, 3, generator=gen) * 4 - 2).cuda()
        view = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1).cuda()
        ref = ops.nerf_forward(net.packed("f32"), pts, view).cpu().numpy()
        scale = np.abs(ref).reshape(-1, 4).max(0) + 1e-6
        # max error over all samples (measured 0.092 / 0.0127 / 1.9e-5, the largest at R = N = 1 where the scale is one
        # sample's own value); a wrong program gives O(1)
        for dtype, tol in (("bf16", 0.15), ("f16", 0.03), ("f16x3", 6e-5)):
            got = ops.nerf_forward(net.packed(dtype), pts, view).cpu().numpy()
            assert got.shape == (R, N, 4) and np.isfinite(got).all()
            err = np.abs(got - ref).reshape(-1, 4).max(0) / scale
            print(f"shapes D{D} W{W} skip{skip} R{R} N{N} {dtype}: max err/scale {err.max():.3e}")
            assert (err < tol).all(), (D, W, skip, R, N, dtype, err)


@pytest.mark.parametrize("tag", ["two_skips", "skip_first_and_late", "no_viewdirs_5ch", "no_viewdirs_4ch"])
@pytest.mark.parametrize("dtype,tol", [("f32", 7e-6), ("f16x3", 7e-6), ("f16", 6.5e-3), ("bf16", 5.2e-2)])   # <= 3x measured: 2.1e-6, 2.1e-6, 2.1e-3, 1.7e-2
def test_nerf_constructor_variants(ops, golden, tag, dtype, tol):
    """The reference's whole NeRF signature (run_nerf_helpers.py:67-134) on every kernel: a `skips` list (several skips,
    a skip right after layer 0), and use_viewdirs=False -- the output_linear head with 5 or 4 channels, no view
    directions (run_network gets viewdirs=None, Trainer.py:792-800).  Expected raw comes from the reference's own
    module.  fp32-grade paths at the golden gate (2e-5 of channel scale), 16-bit paths at operand-rounding size; the
    mirrored module API (forward on the embedded input, Trainer.run_network) must agree with the direct call."""
    from nerf_sampling_amd import synthetic
    from nerf_sampling_amd.run_nerf_helpers import NeRF, get_embedder
    from test_gpu_render import make_trainer

    g = golden("nerf_variants")
    kw = synthetic.NERF_VARIANTS[tag]
    net = NeRF(D=kw["D"], W=kw["W"], input_ch=63, input_ch_views=kw.get("input_ch_views", 27), output_ch=kw.get("output_ch", 4),
               skips=list(kw["skips"]), use_viewdirs=kw["use_viewdirs"])
    net.load_state_dict(synthetic.make_nerf_params(**kw))
    net = net.cuda()
    exp = g[f"raw_{tag}"]
    view = dev(g["viewdirs"]) if kw["use_viewdirs"] else None
    raw = ops.nerf_forward(net.packed(dtype), dev(g["pts"]), view)
    assert tuple(raw.shape) == exp.shape
    scale = np.abs(exp).reshape(-1, exp.shape[-1]).max(0)
    err = np.abs(raw.cpu().numpy() - exp) / scale
    print(f"nerf variant {tag} [{dtype}]: max err / channel scale {err.max():.2e}")
    assert err.max() < tol, (tag, dtype, float(err.max()))
    if dtype == "f32":
        ops.set_compute_dtype("f32")
        e1, _ = get_embedder(10, 0, 3)
        e2, _ = get_embedder(4, 0, 3)
        tr = make_trainer()
        via = tr.run_network(dev(g["pts"]), view, net, embed_fn=e1, embeddirs_fn=e2 if kw["use_viewdirs"] else None)
        assert torch.equal(via, raw)
        x = e1(dev(g["pts"]).reshape(-1, 3))
        if kw["use_viewdirs"]:
            x = torch.cat([x, e2(view[:, None].expand(48, 5, 3).reshape(-1, 3))], -1)
        fwd = net(x)                                    # NeRF.forward on the embedded input, as the reference's module
        assert fwd.shape == (240, exp.shape[-1])
        assert np.abs(fwd.cpu().numpy().reshape(exp.shape) - exp).max() / scale.max() < 2e-5


@pytest.mark.parametrize("tag", ["w64", "w200", "w97_odd", "w40_no_viewdirs"])
@pytest.mark.parametrize("dtype,tol", [("f32", 7e-6), ("f16x3", 7e-6), ("f16", 6.5e-3), ("bf16", 5.2e-2)])   # the gates of the constructor variants
def test_nerf_widths_other_than_the_kernel_widths(ops, golden, tag, dtype, tol):
    """netwidth / netwidth_fine other than 128 / 256 (nerf_utils.py:409-423; run_nerf_helpers.py:87-105 builds W // 2 view
    channels, so an odd width is legal): ns_pack_nerf_ex zero-pads every tensor to the next kernel width -- a padded unit is
    relu(0) = 0 feeding zero columns, the real units sum the same products plus exact zeros.  Expected raw from the reference's
    own module; the packed handle reports the kernel width it runs on."""
    from nerf_sampling_amd import synthetic
    from nerf_sampling_amd.run_nerf_helpers import NeRF

    g = golden("nerf_widths")
    kw = synthetic.NERF_WIDTHS[tag]
    net = NeRF(D=kw["D"], W=kw["W"], input_ch=63, input_ch_views=kw.get("input_ch_views", 27), output_ch=kw.get("output_ch", 4),
               skips=list(kw["skips"]), use_viewdirs=kw["use_viewdirs"])
    net.load_state_dict(synthetic.make_nerf_params(**kw))
    net = net.cuda()
    exp = g[f"raw_{tag}"]
    view = dev(g["viewdirs"]) if kw["use_viewdirs"] else None
    raw = ops.nerf_forward(net.packed(dtype), dev(g["pts"]), view)
    assert tuple(raw.shape) == exp.shape
    scale = np.abs(exp).reshape(-1, exp.shape[-1]).max(0)
    err = np.abs(raw.cpu().numpy() - exp) / scale
    print(f"nerf width {tag} [{dtype}]: max err / channel scale {err.max():.2e}")
    assert err.max() < tol, (tag, dtype, float(err.max()))


def test_nerf_width_beyond_the_kernels_is_refused(ops):
    from nerf_sampling_amd import synthetic
    from nerf_sampling_amd.run_nerf_helpers import NeRF

    net = NeRF(D=2, W=320, input_ch=63, input_ch_views=27, output_ch=4, skips=[], use_viewdirs=True).cuda()
    with pytest.raises(NotImplementedError):
        net.packed("f32")


@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth"])
def test_nerf_forward_embedded_and_rays(ops, gpu_modules, golden, scene):
    g = golden("nerf_mlp")
    m = gpu_modules(scene)
    pts, view = T(g["pts"]), T(g["viewdirs"])
    x90 = torch.cat([O.posenc(pts.reshape(-1, 3), 10), O.posenc(view[:, None].expand(pts.shape).reshape(-1, 3), 4)], -1)
    mine = m["fine"](x90.cuda())                          # NeRF.forward on [M,90]
    exp = g[f"fwd_{scene}_fine"]
    scale = np.abs(exp).max(axis=0)
    assert (np.abs(mine.cpu().numpy() - exp).max(axis=0) / scale < 2e-5).all()
    # points formed in-kernel from (o, d, z) == explicit points
    o = torch.randn(64, 3); d = torch.randn(64, 3); z = torch.rand(64, 4) * 4 + 2
    p = o[:, None] + d[:, None] * z[..., None]
    a = ops.nerf_forward(m["fine"].packed("f32"), p.cuda(), view.cuda())
    b = ops.nerf_forward_rays(m["fine"].packed("f32"), o.cuda(), d.cuda(), z.cuda(), view.cuda())
    close(a, b, 1e-4, 1e-4)


def test_nerf_mlp_ragged_sizes(ops, gpu_modules):
    """Tile tails: sample counts that are not multiples of 32 / of a workgroup, and a single sample."""
    m = gpu_modules("tiny_synth")
    gen = torch.Generator().manual_seed(11)
    p = m["params"]["fine"]
    for R, N in ((1, 1), (3, 5), (33, 31), (257, 9), (700, 64)):
        pts = (torch.rand(R, N, 3, generator=gen) * 2 - 1) * 3
        view = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
        exp = O.run_network(p, pts, view).numpy()
        mine = ops.nerf_forward(m["fine"].packed("f32"), pts.cuda(), view.cuda()).cpu().numpy()
        scale = np.abs(exp).reshape(-1, 4).max(axis=0) + 1e-6
        assert (np.abs(mine - exp).reshape(-1, 4).max(axis=0) / scale < 3e-5).all(), (R, N)


# ---- a4 DepthNet ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth"])
def test_depthnet_f32(ops, gpu_modules, golden, scene):
    g = golden("depthnet")
    z = gpu_modules(scene)["depth"](dev(g["o"]), dev(g["d"]))   # DepthNet.forward -> [R,1]
    exp = g[f"z_{scene}"]
    assert z.shape == exp.shape
    assert torch.isnan(z[256:258]).all()                        # rays that miss the sphere: NaN, as the reference
    close(z, exp, 0, 2e-4)                                      # z in [2,6]: 2e-4 abs = 5e-5 of the range


@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth"])
@pytest.mark.parametrize("dtype,tol", [("bf16", 1.0e-2), ("f16", 1.3e-3)])   # measured rms 2.5-3.3e-3 / 3.2-4.2e-4 (z in [2,6])
def test_depthnet_16bit(ops, gpu_modules, golden, scene, dtype, tol):
    g = golden("depthnet")
    z = ops.depthnet_forward(gpu_modules(scene)["depth"].packed(dtype), dev(g["o"]), dev(g["d"]))
    exp = g[f"z_{scene}"]
    ok = ~np.isnan(exp[:, 0])
    err = np.abs(z.cpu().numpy() - exp)[ok]
    assert np.sqrt((err ** 2).mean()) < tol, float(np.sqrt((err ** 2).mean()))


@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth"])
def test_depthnet_f16x3(ops, gpu_modules, golden, scene):
    """split fp16 operands: the fp32 gate (2e-4 abs on z in [2,6]), NaN rows kept"""
    g = golden("depthnet")
    z = ops.depthnet_forward(gpu_modules(scene)["depth"].packed("f16x3"), dev(g["o"]), dev(g["d"]))
    exp = g[f"z_{scene}"]
    assert torch.isnan(z[256:258]).all()
    ok = ~np.isnan(exp[:, 0])
    print(f"depthnet f16x3 {scene}: max |z err| {np.abs(z.cpu().numpy() - exp)[ok].max():.3e}")
    close(z, exp, 0, 2e-4)


def test_depthnet_f16m_mixed_operands(ops, gpu_modules, golden):
    """NS_DTYPE_F16M: the production trunk with its first three layers on split fp16 operands and the other seven on plain fp16
    (depthnet_mix_kernel: a wave takes its four tiles through the split layers two at a time).  Against the reference's golden
    depths: between the fp16 kernel (rms 3-4e-4 here) and the f16x3 one; NaN rows kept; ragged ray counts against the exact-fp32
    kernel; another trunk shape is refused by the packer and the guard's pairing falls back to f16x3."""
    g = golden("depthnet")
    m = gpu_modules("lego_synth")
    w = m["depth"].packed("f16m")
    z = ops.depthnet_forward(w, dev(g["o"]), dev(g["d"]))
    exp = g["z_lego_synth"]
    assert torch.isnan(z[256:258]).all()
    ok = ~np.isnan(exp[:, 0])
    err = np.abs(z.cpu().numpy() - exp)[ok]
    rms = float(np.sqrt((err ** 2).mean()))
    z16 = ops.depthnet_forward(m["depth"].packed("f16"), dev(g["o"]), dev(g["d"])).cpu().numpy()
    rms16 = float(np.sqrt((np.abs(z16 - exp)[ok] ** 2).mean()))
    print(f"depthnet f16m lego_synth: rms {rms:.3e} (f16: {rms16:.3e}), max {err.max():.3e}")
    # seeded random weights spread the rounding error evenly over the ten layers: three exact ones are worth sqrt(7 / 10) (measured
    # 3.4e-4 against 4.4e-4) ...
    assert rms < 0.9 * rms16 and rms < 5e-4, (rms, rms16)
    # ... a TRAINED DepthNet loses its depth in the first layers (their inputs are its widest-ranged activations): on the fitted
    # scene the mixed kernel is 7 x closer than the fp16 one (measured rms 1.2e-4 against 8.9e-4, z in [2, 6])
    fit = gpu_modules("shapes_fit")["depth"]
    _, K = O.blender_intrinsics(200, 200)
    o_f, d_f = ops.get_rays(200, 200, K, O.pose_spherical(-50.0, -30.0, 4.0)[:3, :4])[:2]
    ref = ops.depthnet_forward(fit.packed("f32"), o_f, d_f)
    fin = torch.isfinite(ref)
    e_mix = float((ops.depthnet_forward(fit.packed("f16m"), o_f, d_f) - ref)[fin].pow(2).mean().sqrt())
    e_16 = float((ops.depthnet_forward(fit.packed("f16"), o_f, d_f) - ref)[fin].pow(2).mean().sqrt())
    print(f"depthnet f16m fitted scene: rms {e_mix:.3e} (f16: {e_16:.3e})")
    assert e_mix < 0.3 * e_16 and e_mix < 4e-4, (e_mix, e_16)
    gen = torch.Generator().manual_seed(13)
    for R in (1, 31, 33, 63, 65, 300, 1000):
        o = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1) * 4.0
        d = -o / 4.0 + 0.1 * torch.randn(R, 3, generator=gen)
        ref = ops.depthnet_forward(m["depth"].packed("f32"), o.cuda(), d.cuda())
        got = ops.depthnet_forward(w, o.cuda(), d.cuda())
        assert got.shape == ref.shape and torch.equal(torch.isnan(got), torch.isnan(ref)), R
        fin = torch.isfinite(ref)
        assert float((got - ref)[fin].abs().max()) < 5e-3, (R, float((got - ref)[fin].abs().max()))
    tiny = gpu_modules("tiny_synth")["depth"]
    with pytest.raises(NotImplementedError):
        tiny.packed("f16m")
    ops.set_compute_dtype("bf16"); ops.set_psnr_guard(True, depthnet="f16m")
    try:
        assert m["depth"].packed().dtype == "f16m" and tiny.packed().dtype == "f16x3"
    finally:
        ops.set_psnr_guard(False, depthnet="f16x3"); ops.set_compute_dtype("f32")


def test_depthnet_ragged_sizes(ops, gpu_modules):
    m = gpu_modules("tiny_synth")
    gen = torch.Generator().manual_seed(12)
    for R in (1, 31, 33, 300):
        o = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1) * 4.0
        d = -o / 4.0 + 0.1 * torch.randn(R, 3, generator=gen)
        exp = O.depthnet_forward(m["params"]["depth"], o, d)
        close(m["depth"](o.cuda(), d.cuda()), exp, 0, 2e-4)


@pytest.mark.parametrize("hidden,cat", [([128] * 6, [128, 128, 128, 128, 256]),      # the reference's class defaults
                                        ([48, 80], [64, 16, 200, 256]), ([32], [96]), ([256] * 3, [256] * 4)])
def test_depthnet_shapes_vs_oracle(ops, hidden, cat):
    """DepthNet shapes other than one uniform width -- the reference's class defaults (depth_net.py:13-16, pinned by its
    own structure tests, tests.py:115-194), ragged widths, one layer -- through the folded kernels, all three operand
    types, against the oracle's literal chain on the module's own (torch-default-init, seeded) weights."""
    from nerf_sampling_amd.depth_net import DepthNet

    torch.manual_seed(31 + len(hidden) + sum(cat))
    dn = DepthNet(hidden_sizes=hidden, cat_hidden_sizes=cat)
    # default init shrinks the signal layer by layer (z would be a constant); the synthetic scenes' gains keep it alive
    p = {k: v.detach().clone() * (2.4 if "cat_layers" in k and k.endswith("weight") else 1.7 if k.endswith("weight") else 1.0)
         for k, v in dn.state_dict().items()}
    dn.load_state_dict(p)
    dn = dn.cuda()
    for q in dn.parameters():
        q.requires_grad_(False)
    gen = torch.Generator().manual_seed(5)
    for R in (1, 70, 300):
        o = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1) * 4.0
        d = -o / 4.0 + 0.1 * torch.randn(R, 3, generator=gen)
        exp = O.depthnet_forward(p, o, d)
        assert exp.shape == (R, 1)
        if R == 300:
            assert float(exp.std()) > 0.05                  # the depth really varies across rays
        close(ops.depthnet_forward(dn.packed("f32"), o.cuda(), d.cuda()), exp, 0, 2e-4)
        for dtype, tol in (("bf16", 3e-2), ("f16", 4e-3), ("f16x3", 2e-4)):
            z = ops.depthnet_forward(dn.packed(dtype), o.cuda(), d.cuda())
            assert float((z.cpu() - exp).abs().max()) < tol, (dtype, R, float((z.cpu() - exp).abs().max()))


@pytest.mark.parametrize("dtype", ["f32", "f16x3", "bf16", "f16"])
def test_nerf_mlp_nan_points_stay_nan(ops, gpu_modules, dtype):
    """A NaN sample point (a ray that misses the DepthNet's sphere gives NaN depths, utils.py:159-217) comes out as NaN
    raw values, as torch.relu / nn.Linear propagate it in the reference -- and only for that sample."""
    m = gpu_modules("tiny_synth")
    pts = torch.rand(3, 5, 3) * 2 - 1
    pts[1, 2, 0] = float("nan")
    view = torch.nn.functional.normalize(torch.randn(3, 3), dim=-1)
    raw = ops.nerf_forward(m["fine"].packed(dtype), pts.cuda(), view.cuda()).cpu()
    assert torch.isnan(raw[1, 2]).all(), raw[1, 2]
    ok = torch.ones(3, 5, dtype=torch.bool); ok[1, 2] = False
    assert torch.isfinite(raw[ok]).all()


@pytest.mark.parametrize("tag", ["default", "ragged", "one"])
def test_depthnet_shapes_golden(ops, golden, tag):
    """The same non-uniform DepthNet shapes through the folded HIP kernels against outputs captured from the REFERENCE
    (tests/golden/depthnet_shapes.npz): fp32 and f16x3 at the fp32 gate, bf16 / f16 at 3x their measured error."""
    from nerf_sampling_amd import synthetic
    from nerf_sampling_amd.depth_net import DepthNet

    g = golden("depthnet_shapes")
    hs, cs, seed = synthetic.DEPTHNET_SHAPES[tag]
    dn = DepthNet(hidden_sizes=list(hs), cat_hidden_sizes=list(cs))
    dn.load_state_dict(synthetic.make_depthnet_params_shaped(seed, hs, cs, branch_gain=synthetic.SQRT3,
                                                             trunk_gain=synthetic.SQRT6))
    dn = dn.cuda()
    for q in dn.parameters():
        q.requires_grad_(False)
    exp = g[f"z_{tag}"]
    ok = ~np.isnan(exp[:, 0])
    # measured max |z err| (round 2): f32 1.7e-6, f16x3 1.2e-6, f16 1.3e-3, bf16 8.8e-3
    for dtype, tol in (("f32", 2e-4), ("f16x3", 2e-4), ("f16", 4e-3), ("bf16", 2.6e-2)):
        z = ops.depthnet_forward(dn.packed(dtype), dev(g["o"]), dev(g["d"])).cpu().numpy()
        assert z.shape == exp.shape
        assert np.isnan(z[~ok]).all(), dtype                                   # rays that miss the sphere stay NaN
        err = np.abs(z - exp)[ok]
        print(f"depthnet_shapes {tag} {dtype}: max |z err| {err.max():.3e}")
        assert err.max() < tol, (tag, dtype, float(err.max()))


# ---- the reference's pytest=True determinism hook, through the mirrored API -----------------------------------------
def test_pytest_hook_against_the_reference(ops, golden, gpu_modules):
    """pytest=True (Trainer.py:621-624, run_nerf_helpers.py:265-273, sampling_trainer.py:188-193): numpy draws under
    np.random.seed(0).  Expected values are the reference's own outputs (tests/golden/pytest_hook.npz).  Recorded
    difference: the reference's numpy draws are float64 and promote everything downstream to float64 (which is also why
    its sample_as_in_NeRF(pytest=True) raises at the MLP); this build casts the draws to fp32 and stays fp32, so the
    comparison is at fp32 rounding."""
    from test_gpu_render import make_trainer, render_kwargs

    from nerf_sampling_amd.run_nerf_helpers import sample_pdf

    g = golden("pytest_hook")
    # sample_pdf(det=True / False, pytest=True)
    for det, key in ((True, "pdf_det"), (False, "pdf_rnd")):
        mine = sample_pdf(dev(g["pdf_bins"]), dev(g["pdf_weights"]), 128, det=det, pytest=True)
        assert mine.dtype == torch.float32
        err = np.abs(mine.cpu().numpy() - g[key])
        assert np.mean(err > 2e-5) < 2e-3 and np.median(err) < 1e-6, (key, float(np.mean(err > 2e-5)))
    # raw2outputs(raw_noise_std > 0, pytest=True): uniform numpy noise
    tr = make_trainer()
    res = tr.raw2outputs(dev(g["r2o_raw"]), dev(g["r2o_z"]), dev(g["r2o_rays_d"]), float(g["r2o_std"]), True, pytest=True)
    close(res[5], g["r2o_alphas"], 2e-6, 1e-7)
    close(res[6], g["r2o_weights"], 3e-5, 1e-7)
    close(res[0], g["r2o_rgb"], 1e-5, 2e-6)
    close(res[1], g["r2o_disp"], 2e-5, 1e-6)
    close(res[2], g["r2o_acc"], 1e-5, 1e-6)
    close(res[3], g["r2o_depth"], 1e-5, 2e-6)
    close(res[4], g["r2o_density"], 0, 0)
    # sample_coarse_points(perturb=1, pytest=True): stratified jitter, then the coarse MLP + compositing
    m = gpu_modules("tiny_synth")
    kw = render_kwargs(tr, m)
    rb = dev(g["coarse_ray_batch"])
    for lindisp in (True, False):
        out = tr.sample_coarse_points(near=rb[:, 6].contiguous(), far=rb[:, 7].contiguous(), perturb=1.0,
                                      N_rays=rb.shape[0], N_samples=64, viewdirs=rb[:, -3:].contiguous(),
                                      network_fn=m["coarse"], network_query_fn=kw["network_query_fn"],
                                      rays_o=rb[:, 0:3].contiguous(), rays_d=rb[:, 3:6].contiguous(), raw_noise_std=0.0,
                                      white_bkgd=True, pytest=True, lindisp=lindisp)
        close(out[5], g[f"coarse_lin{int(lindisp)}_z"], 2e-6, 1e-6)
        bad, _ = (np.mean(np.abs(out[0].cpu().numpy() - g[f"coarse_lin{int(lindisp)}_rgb_map"]).max(-1) > 1e-4), None)
        assert bad <= 0.02, bad                          # fp32 MLP at golden-level tolerance, as test_sample_as_in_nerf
        assert np.median(np.abs(out[3].cpu().numpy() - g[f"coarse_lin{int(lindisp)}_weights"])) < 1e-5
