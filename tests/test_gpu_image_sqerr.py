"""ns_image_sqerr / DeviceRayDataset.image_sqerr: the squared error of a rendered frame against a dataset image, summed in
double on the device.  Yardstick: sum (double)(fl32(rgb - target))^2 with the ray-batch kernels' target -- exact where every
term is exact, within the bound of ANY summation order of non-negative terms on random floats."""

import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = [(5, 7), (33, 20), (67, 129)]      # the last: more than one workgroup's share (2048 pixels), no side a multiple of 64
N_IMAGES = 3
SENTINEL = -12345.0


def _bands(H):
    return [None, (0, 1), (H - 1, H), (H // 3, H // 3 + max(1, H // 2))]


def _dataset(images, white_bkgd):
    from nerf_sampling_amd.ray_batches import DeviceRayDataset

    n, H, W, _ = images.shape
    poses = np.tile(np.eye(4, dtype=np.float32)[None], (n, 1, 1))
    return DeviceRayDataset(images, poses, [H, W, 1.5 * W], [0], white_bkgd=white_bkgd)


def _target(images, white_bkgd):
    """numpy's fp32 restatement of the kernels' target: rgb, or rgb * a + (1 - a) in separate roundings"""
    if images.shape[-1] == 4 and white_bkgd:
        a = images[..., 3:]
        return (images[..., :3] * a).astype(np.float32) + (np.float32(1.0) - a)
    return images[..., :3]


def _grid_case(H, W, Cc, seed):
    """rgb and image rgb multiples of 1/64 in [0,1], alpha in {0, 1/2, 1}: every blend, difference, square and sum is exact"""
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 65, size=(N_IMAGES, H, W, Cc)).astype(np.float32) / np.float32(64.0)
    if Cc == 4:
        images[..., 3] = rng.integers(0, 3, size=(N_IMAGES, H, W)).astype(np.float32) / np.float32(2.0)
    k = rng.integers(0, 65, size=(N_IMAGES, H * W, 3))
    return images, k


def _grid_reference(images, k, white_bkgd, img, r0, r1):
    """the sum in int64, in units of 1/128^2"""
    _, H, W, Cc = images.shape
    m = np.rint(images[img, ..., :3] * 64).astype(np.int64).reshape(H * W, 3)
    if Cc == 4 and white_bkgd:
        a2 = np.rint(images[img, ..., 3] * 2).astype(np.int64).reshape(H * W, 1)          # 0, 1, 2
        t = m * a2 + (2 - a2) * 64                                                          # target * 128
    else:
        t = 2 * m
    d = (2 * k[img] - t)[r0 * W:r1 * W]
    return float(np.sum(d * d, dtype=np.int64)) / 16384.0


def _device_rgb(rgb_host, stride):
    """[R,3] on the device: packed, or the [:, :3] view of a [R,4] shard whose fourth column is poisoned"""
    import torch

    if stride == 3:
        return torch.from_numpy(np.ascontiguousarray(rgb_host)).cuda()
    shard = torch.full((rgb_host.shape[0], 4), float("nan"), dtype=torch.float32, device="cuda")
    shard[:, :3] = torch.from_numpy(np.ascontiguousarray(rgb_host)).cuda()
    return shard[:, :3]


def _guarded_workspace(ds, n_pixels):
    import torch

    need = ds.sqerr_workspace_bytes(n_pixels)
    assert need >= 8 * ((n_pixels + 2047) // 2048) and need % 256 == 0
    buf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[256:256 + need]


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("Cc,white", [(3, False), (3, True), (4, False), (4, True)])
def test_exact_on_a_dyadic_grid(H, W, Cc, white):
    """Full frames and row bands, both strides, several images each into its own slot of one array: the result EQUALS the int64
    reference, and the guard bands around ``out`` and around the workspace stay untouched."""
    import torch

    images, k = _grid_case(H, W, Cc, seed=H * 1000 + W * 10 + Cc)
    ds = _dataset(images, white)
    for rows in _bands(H):
        r0, r1 = (0, H) if rows is None else rows
        for stride in (3, 4):
            out = torch.full((N_IMAGES + 2,), SENTINEL, dtype=torch.float64, device="cuda")
            buf, ws = _guarded_workspace(ds, (r1 - r0) * W)
            for img in range(N_IMAGES):
                rgb = _device_rgb((k[img][r0 * W:r1 * W] / 64.0).astype(np.float32), stride)
                assert ds.image_sqerr(img, rgb, rows=rows, out=out, slot=img + 1, workspace=ws) is out
            got = out.cpu().numpy()
            assert got[0] == SENTINEL and got[-1] == SENTINEL
            for img in range(N_IMAGES):
                ref = _grid_reference(images, k, white, img, r0, r1)
                print(f"{H}x{W} C={Cc} white={white} rows={rows} stride={stride} img={img}: got {got[img + 1]!r} ref {ref!r}")
                assert got[img + 1] == ref
            b = buf.cpu().numpy()
            assert (b[:256] == 0xA5).all() and (b[-256:] == 0xA5).all()


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("Cc,white", [(3, False), (4, False), (4, True)])
def test_random_floats_within_the_summation_bound(H, W, Cc, white):
    """|got - ref| <= (n - 1) 2^-53 ref, ref the float64 sum of squares of the fp32 differences (exactly rounded: math.fsum).
    The terms are non-negative, so the bound holds for any order of summation, and only for the single fp32 rounding of the
    difference; the same bits on a second call and on a second stream; the returned tensor form."""
    import torch

    rng = np.random.default_rng(H * 77 + W + Cc)
    images = rng.random((N_IMAGES, H, W, Cc), dtype=np.float32)
    target = _target(images, white)
    ds = _dataset(images, white)
    side = torch.cuda.Stream()
    for rows in _bands(H):
        r0, r1 = (0, H) if rows is None else rows
        for img, stride in ((0, 3), (N_IMAGES - 1, 4)):
            rgb_h = rng.random(((r1 - r0) * W, 3), dtype=np.float32) * np.float32(1.25) - np.float32(0.125)
            rgb = _device_rgb(rgb_h, stride)
            d = rgb_h - target[img].reshape(H * W, 3)[r0 * W:r1 * W]
            assert d.dtype == np.float32
            d = d.astype(np.float64).reshape(-1)
            ref = math.fsum(d * d)
            one = ds.image_sqerr(img, rgb, rows=rows)
            assert one.shape == (1,) and one.dtype == torch.float64 and one.is_cuda
            again = ds.image_sqerr(img, rgb, rows=rows)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                other = ds.image_sqerr(img, rgb, rows=rows)
            side.synchronize()
            got = float(one.cpu()[0])
            bound = (d.size - 1) * 2.0 ** -53 * ref
            print(f"{H}x{W} C={Cc} white={white} rows={rows} stride={stride}: got {got!r} ref {ref!r} "
                  f"|diff| {abs(got - ref):.3e} bound {bound:.3e}")
            assert abs(got - ref) <= bound
            assert one.cpu().numpy().tobytes() == again.cpu().numpy().tobytes() == other.cpu().numpy().tobytes()


def test_a_nan_pixel_makes_its_sum_nan_and_no_other():
    import torch

    H, W = 67, 129
    images, k = _grid_case(H, W, 3, seed=5)
    ds = _dataset(images, False)
    out = torch.full((5,), SENTINEL, dtype=torch.float64, device="cuda")
    for img in range(N_IMAGES):
        rgb_h = (k[img] / 64.0).astype(np.float32)
        if img == 1:
            rgb_h[40 * W + 17, 2] = np.nan                # a ray that misses the sphere
        ds.image_sqerr(img, _device_rgb(rgb_h, 3), out=out, slot=img + 1)
    got = out.cpu().numpy()
    assert got[0] == SENTINEL and got[4] == SENTINEL and math.isnan(got[2])
    assert got[1] == _grid_reference(images, k, False, 0, 0, H) and got[3] == _grid_reference(images, k, False, 2, 0, H)
    assert math.isnan(float(ds.psnr_from_sqerr(out[2:3], 3 * H * W)[0]))


def test_refusals_before_any_launch():
    """What the host knows is refused by the entry itself (-1, NS_E_INVALID) and by the wrapper (ValueError); ``out`` and the
    workspace are never written."""
    import torch

    from nerf_sampling_amd import _lib

    H, W = 5, 7
    images, k = _grid_case(H, W, 4, seed=9)
    ds = _dataset(images, True)
    lib = _lib.load()
    rgb = _device_rgb((k[0] / 64.0).astype(np.float32), 3)
    out = torch.full((2,), SENTINEL, dtype=torch.float64, device="cuda")
    buf, ws = _guarded_workspace(ds, H * W)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                          # noqa: E731

    def entry(desc=ds.desc, img=0, r0=0, r1=H, rgb_p=p(rgb), stride=0, sum_p=p(out), ws_p=p(ws)):
        return lib.ns_image_sqerr(C.byref(desc), img, r0, r1, rgb_p, stride, sum_p, ws_p, stream)

    no_images = _lib.RayDataset.from_buffer_copy(ds.desc)
    no_images.images_dev = None
    for bad in (dict(img=-1), dict(img=N_IMAGES), dict(r0=2, r1=2), dict(r0=3, r1=2), dict(r0=-1), dict(r1=H + 1),
                dict(desc=no_images), dict(rgb_p=None), dict(sum_p=None), dict(ws_p=None), dict(stride=1), dict(stride=5),
                dict(stride=-3)):
        assert entry(**bad) == -1, bad
        assert b"ns_image_sqerr" in lib.ns_last_error()
    for bad in (dict(image_idx=-1), dict(image_idx=N_IMAGES), dict(rows=(2, 2)), dict(rows=(0, H + 1)), dict(rows=(-1, 2)),
                dict(rgb=rgb[:-1]), dict(rgb=rgb.double()), dict(rgb=rgb.cpu()), dict(rgb=rgb.t()),
                dict(out=out.float()), dict(slot=2), dict(slot=-1), dict(workspace=ws[:8].cpu()), dict(workspace=ws[:0])):
        args = dict(image_idx=0, rgb=rgb, out=out, slot=0, workspace=ws)
        args.update(bad)
        with pytest.raises(ValueError):
            ds.image_sqerr(**args)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (buf.cpu().numpy() == 0xA5).all()
    assert entry() == 0 and entry(stride=3) == 0                                     # and the call they vary is a good one
    assert float(out.cpu()[0]) == _grid_reference(images, k, True, 0, 0, H)
