"""Training ray batches from a device-resident dataset (ns_ray_batch_gather / ns_ray_batch_draw, ray_batches.py): the rays
are ns_get_rays' bits at the drawn pixels, the targets numpy's blend, the drawn indices those of the host restatement of the
generator; Trainer(device_batches="gather") repeats the default batches bit for bit; the draw is capturable in the graphed
training step."""

import copy
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

K_OFF = np.array([[11.3, 0.0, 3.1], [0.0, 9.7, 2.2], [0.0, 0.0, 1.0]])       # fx != fy, principal point off centre
SHAPES = {"5x7": (5, 7), "33x20": (33, 20)}
_cache = {}


def _scene(shape):
    """3 images [H,W,4] in [0,1] with a varied alpha, 3 poses [4,4], and ops.get_rays of every image (computed once)."""
    if shape not in _cache:
        from nerf_sampling_amd import ops

        H, W = SHAPES[shape]
        rng = np.random.default_rng(H * 100 + W)
        images = rng.random((3, H, W, 4), dtype=np.float32)
        images[..., 3] = np.where(rng.random((3, H, W)) < 0.3, np.float32(1.0), images[..., 3])
        poses = np.stack([O.pose_spherical(a, -30.0 + 7 * k, 4.0 + 0.3 * k).numpy() for k, a in enumerate((10.0, 130.0, 250.0))])
        poses = poses.astype(np.float32)
        ref = [tuple(t.cpu() for t in ops.get_rays(H, W, K_OFF, poses[n][:3, :4])) for n in range(3)]
        ref = tuple(torch.stack([r[k] for r in ref]) for k in range(3))               # o, d, viewdirs: [3, H*W, 3]
        _cache[shape] = (images, poses, ref)
    return _cache[shape]


def _dataset(shape, channels=4, white=True, stride=16, i_train=(0, 1, 2)):
    from nerf_sampling_amd.ray_batches import DeviceRayDataset

    images, poses, _ = _scene(shape)
    return DeviceRayDataset(np.ascontiguousarray(images[..., :channels]), poses if stride == 16 else poses[:, :3],
                            K_OFF, list(i_train), white_bkgd=white)


def _host_target(shape, channels, white, img, pix):
    images, _, _ = _scene(shape)
    flat = images.reshape(3, -1, 4)
    if channels == 4 and white:
        flat = flat[..., :3] * flat[..., -1:] + (1.0 - flat[..., -1:])          # BlenderTrainer.load_data's expression
    return torch.from_numpy(np.ascontiguousarray(flat[img, pix, :3]))


def _indices(shape, B, seed):
    H, W = SHAPES[shape]
    rng = np.random.default_rng(seed)
    pix = rng.integers(0, H * W, B)
    if B >= 2:
        pix[0], pix[-1] = 0, H * W - 1                                           # the frame's corners
    return rng.integers(0, 3, B), pix


@pytest.mark.parametrize("stride", [12, 16])
@pytest.mark.parametrize("channels,white", [(3, False), (3, True), (4, False), (4, True)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gather_equals_get_rays_and_the_host_blend(shape, channels, white, stride):
    ds = _dataset(shape, channels, white, stride)
    assert ds.desc.pose_stride == stride and ds.desc.C == channels
    _, _, (ro, rd, rv) = _scene(shape)
    for B in (1, 63, 64, 65, 1000):                                              # 1000 > H*W of either frame: repeats
        img, pix = _indices(shape, B, B)
        for per_ray in (False, True):
            im = img if per_ray else int(img[0])
            idx = img if per_ray else np.full(B, int(img[0]))
            rays, target, view = ds.gather(im, pix, want_viewdirs=True)
            assert rays.shape == (2, B, 3) and target.shape == view.shape == (B, 3)
            assert torch.equal(rays[0].cpu(), ro[idx, pix]) and torch.equal(rays[1].cpu(), rd[idx, pix])
            assert torch.equal(view.cpu(), rv[idx, pix])
            assert torch.equal(target.cpu(), _host_target(shape, channels, white, idx, pix))
    # device index tensors are taken as they are (int32 or int64), and out= writes in place
    img, pix = _indices(shape, 65, 3)
    out = (torch.zeros(2, 65, 3).cuda(), torch.zeros(65, 3).cuda())
    rays, target = ds.gather(torch.from_numpy(img).cuda(), torch.from_numpy(pix).cuda().to(torch.int32), out=out)
    assert rays is out[0] and target is out[1]
    assert torch.equal(rays[1].cpu(), rd[img, pix]) and torch.equal(target.cpu(), _host_target(shape, channels, white, img, pix))


def test_gather_with_each_output_null_in_turn():
    from nerf_sampling_amd import _lib, ops

    lib, ds = _lib.load(), _dataset("33x20")
    _, _, (ro, rd, rv) = _scene("33x20")
    img, pix = _indices("33x20", 65, 11)
    want = [ro[img, pix], rd[img, pix], rv[img, pix], _host_target("33x20", 4, True, img, pix)]
    img_d, pix_d = (torch.from_numpy(a.astype(np.int32)).cuda() for a in (img, pix))
    for skip in range(4):
        bufs = [torch.full((65, 3), -7.0).cuda() for _ in range(4)]
        ptrs = [None if k == skip else ops._ptr(b) for k, b in enumerate(bufs)]
        assert lib.ns_ray_batch_gather(C.byref(ds.desc), ops._ptr(img_d), 0, ops._ptr(pix_d), 65, *ptrs, ops._stream("cuda")) == 0
        for k in range(4):
            assert torch.equal(bufs[k].cpu(), torch.full((65, 3), -7.0) if k == skip else want[k]), (skip, k)
    # device indices out of range are clamped by the kernel, never read out of bounds
    far = torch.tensor([-5, 10 ** 9, 3], dtype=torch.int32).cuda()
    rays, target = ds.gather(torch.tensor([-1, 7, 1], dtype=torch.int32).cuda(), far)
    assert torch.equal(rays[1].cpu(), rd[[0, 2, 1], [0, 33 * 20 - 1, 3]])
    assert torch.equal(target.cpu(), _host_target("33x20", 4, True, np.array([0, 2, 1]), np.array([0, 659, 3])))


@pytest.mark.parametrize("window,B", [((16, 17, 9, 10), 1), ((10, 13, 6, 11), 15), ((10, 13, 6, 11), 7), (None, 660), (None, 65)])
def test_draw_per_image_equals_the_host_generator(window, B):
    from nerf_sampling_amd import ray_batches as RB

    train = (2, 0, 1)
    ds = _dataset("33x20", i_train=train)
    for step in (0, 1, 5, 1000):
        for seed in (0, 0x1234567890ABCDEF):
            rays, target, view, (img, pix) = ds.draw(B, step=step, window=window, seed=seed, want_viewdirs=True, want_indices=True)
            e_img, e_pix = RB.draw_indices(B, step, seed, "per_image", 33, 20, train, window=window)
            assert img.dtype == pix.dtype == torch.int32
            assert np.array_equal(img.cpu().numpy(), e_img) and np.array_equal(pix.cpu().numpy(), e_pix)
            g_rays, g_target, g_view = ds.gather(e_img, e_pix, want_viewdirs=True)
            assert torch.equal(rays, g_rays) and torch.equal(target, g_target) and torch.equal(view, g_view)
            if B == 660:                                                          # a whole permutation of the frame
                assert np.array_equal(np.sort(e_pix), np.arange(660))
            # the same launch with {step, window} read from device memory
            w = RB.full_window(33, 20) if window is None else window
            params = torch.tensor([step, *w], dtype=torch.int32).cuda()
            d_rays, d_target, (d_img, d_pix) = ds.draw(B, seed=seed, params_dev=params, want_indices=True)
            assert torch.equal(d_rays, rays) and torch.equal(d_target, target)
            assert torch.equal(d_img, img) and torch.equal(d_pix, pix)


def test_draw_all_images_walks_each_epoch_once():
    from nerf_sampling_amd import ray_batches as RB

    train, B, N = (2, 0, 1), 64, 105                                              # the host test's case: three epochs in steps 0..4
    ds = _dataset("5x7", channels=3, white=False, stride=12, i_train=train)
    seen = []
    for step in range(5):
        rays, target, (img, pix) = ds.draw(B, step=step, scope="all_images", seed=9, want_indices=True)
        e_img, e_pix = RB.draw_indices(B, step, 9, "all_images", 5, 7, train)
        assert np.array_equal(img.cpu().numpy(), e_img) and np.array_equal(pix.cpu().numpy(), e_pix)
        g_rays, g_target = ds.gather(e_img, e_pix)
        assert torch.equal(rays, g_rays) and torch.equal(target, g_target)
        params = torch.tensor([step, 0, 5, 0, 7], dtype=torch.int32).cuda()
        d_rays, d_target, (d_img, d_pix) = ds.draw(B, scope="all_images", seed=9, params_dev=params, want_indices=True)
        assert torch.equal(d_rays, rays) and torch.equal(d_target, target) and torch.equal(d_img, img) and torch.equal(d_pix, pix)
        seen.append(img.cpu().numpy().astype(np.int64) * 35 + pix.cpu().numpy())
    seen = np.concatenate(seen)
    for e in range(3):
        assert np.array_equal(np.sort(seen[e * N:(e + 1) * N]), np.arange(N))


def test_draw_source_advances_its_device_step():
    from nerf_sampling_amd import ray_batches as RB

    ds = _dataset("33x20")
    crop = RB.precrop_window(33, 20, 0.5)
    src = RB.DrawBatchSource(ds, 64, seed=4, first_step=3, window_fn=lambda i: crop if i < 5 else None)
    for i in range(3, 8):
        rays, target = src(i)
        e_rays, e_target = ds.draw(64, step=i, window=crop if i < 5 else None, seed=4)
        assert torch.equal(rays, e_rays) and torch.equal(target, e_target), i
    assert src.params.cpu().tolist() == [8, 0, 33, 0, 20]


def test_refusals_raise_before_any_launch():
    from nerf_sampling_amd import _lib
    from nerf_sampling_amd.ray_batches import DeviceRayDataset, DrawBatchSource

    images, poses, _ = _scene("5x7")
    ds = _dataset("5x7")
    for img, pix in ((3, [0]), (-1, [0]), (0, [35]), (0, [-1]), ([0, 3], [0, 1]), ([0], [0, 1])):
        with pytest.raises(ValueError):
            ds.gather(img, pix)
    with pytest.raises(TypeError):
        ds.gather(0, [0.5])
    for kw in (dict(B=-1), dict(B=1, window=(2, 2, 0, 7)), dict(B=1, window=(0, 5, 4, 3)), dict(B=1, window=(0, 6, 0, 7)),
               dict(B=36), dict(B=16, window=(1, 4, 1, 6)), dict(B=1, step=-1), dict(B=1, scope="some_images")):
        with pytest.raises(ValueError):
            ds.draw(**kw)
    with pytest.raises(ValueError):
        DrawBatchSource(ds, 36)
    # the entries themselves refuse what the wrappers would (a wrapper bug cannot reach a launch)
    lib, one = _lib.load(), C.c_void_p(ds.images.data_ptr())
    bad = _lib.RayDrawParams(0, 2, 2, 0, 7)
    assert lib.ns_ray_batch_draw(C.byref(ds.desc), one, 3, 0, None, C.byref(bad), 0, 1, None, None, None, None, None, one, None) == -1
    whole = _lib.RayDrawParams(0, 0, 5, 0, 7)
    assert lib.ns_ray_batch_draw(C.byref(ds.desc), one, 3, 0, None, C.byref(whole), 0, 36, None, None, None, None, None, one, None) == -1
    assert lib.ns_ray_batch_gather(C.byref(ds.desc), None, 3, one, 1, None, None, None, one, None) == -1
    # the dataset refuses what the kernels are not built for
    with pytest.raises(TypeError):
        DeviceRayDataset((images * 255).astype(np.uint8), poses, K_OFF, [0])
    with pytest.raises(ValueError):
        DeviceRayDataset(images[..., :2], poses, K_OFF, [0])
    with pytest.raises(ValueError):
        DeviceRayDataset(images, poses, K_OFF, [3])
    with pytest.raises(ValueError):
        DeviceRayDataset(images, poses, K_OFF, [])
    with pytest.raises(ValueError):
        DeviceRayDataset(images, poses[:2], K_OFF, [0])
    with pytest.raises(ValueError):
        DeviceRayDataset(images, poses, [5, 8, 10.0], [0])


def _plain_trainer(shape, **over):
    from nerf_sampling_amd.trainers import Trainer

    H, W = SHAPES[shape]
    kw = dict(dataset_type="blender", basedir="", expname="", no_batching=True, datadir="", device="cuda", N_rand=64)
    kw.update(over)
    tr = Trainer(**kw)
    tr.H, tr.W, tr.K = H, W, K_OFF
    return tr


@pytest.mark.parametrize("over", [dict(), dict(precrop_iters=2, precrop_frac=0.5), dict(single_ray=True),
                                  dict(single_ray=True, precrop_iters=2)], ids=["plain", "precrop", "single_ray", "single_ray_crop"])
def test_trainer_gather_mode_repeats_the_default_batches(over):
    """Iterations 0..3 (inside and after precrop_iters = 2) on a split of two of the three images."""
    images4, poses, _ = _scene("33x20")
    images = images4[..., :3] * images4[..., -1:] + (1.0 - images4[..., -1:])     # what load_data hands the trainer
    poses_t = torch.from_numpy(poses).cuda()
    i_train = np.array([2, 0])
    got = {}
    for mode in (False, "gather"):
        tr = _plain_trainer("33x20", device_batches=mode, **over)
        np.random.seed(5)
        got[mode] = [tr.sample_random_ray_batch(None, None, i_train, images, poses_t, i)[2:] + (tr.c2w.clone(),) for i in range(4)]
        got[mode].append(np.random.rand())                                       # the stream was consumed alike
    for (rays, target, c2w), (e_rays, e_target, e_c2w) in zip(got["gather"][:4], got[False][:4]):
        assert rays.shape == e_rays.shape and rays.is_cuda and target.is_cuda
        assert torch.equal(rays, e_rays) and torch.equal(target, e_target) and torch.equal(c2w, e_c2w)
    assert got["gather"][4] == got[False][4]


def test_trainer_option_is_validated():
    with pytest.raises(ValueError):
        _plain_trainer("5x7", device_batches="scatter")
    with pytest.raises(ValueError):
        _plain_trainer("5x7", device_batches="gather", no_batching=False)
    with pytest.raises(ValueError):
        _plain_trainer("5x7", device_batches="draw", single_ray=True)


def test_trainer_draw_mode_batches():
    """'draw' through Trainer.sample_random_ray_batch: the pre-crop is the window, use_batching the all-images scope (and no
    rays_rgb tensor is built); the indices are the host generator's."""
    from nerf_sampling_amd import ray_batches as RB

    images4, poses, _ = _scene("33x20")
    images = np.ascontiguousarray(images4[..., :3])
    poses_t = torch.from_numpy(poses).cuda()
    i_train = np.array([2, 0])
    tr = _plain_trainer("33x20", device_batches="draw", batch_seed=21, precrop_iters=3, precrop_frac=0.5)
    ds = tr.ray_dataset(i_train, images, poses_t)
    for i in range(1, 6):
        _, _, rays, target = tr.sample_random_ray_batch(None, None, i_train, images, poses_t, i)
        img, pix = RB.draw_indices(64, i, 21, "per_image", 33, 20, i_train, window=RB.precrop_window(33, 20, 0.5) if i < 3 else None)
        e_rays, e_target = ds.gather(img, pix)
        assert torch.equal(rays, e_rays) and torch.equal(target, e_target), i
    tb = _plain_trainer("33x20", device_batches="draw", batch_seed=21, no_batching=False, N_rand=500)
    assert tb.prepare_raybatch_tensor_if_batching_random_rays(poses, images, i_train)[2] is None
    ds = tb.ray_dataset(i_train, images, poses_t)
    for i in range(1, 5):                                                         # 1320 rays: the epoch ends inside step 2
        rays, target = tb.sample_random_ray_batch(None, 0, i_train, images, poses_t, i)[2:]
        e_rays, e_target = ds.gather(*RB.draw_indices(500, i, 21, "all_images", 33, 20, i_train))
        assert torch.equal(rays, e_rays) and torch.equal(target, e_target), i


def test_field_fitter_source_in_gather_mode():
    """FieldFitter._blender_source(device_batches='gather'): 4-channel images blended per pixel in the kernel == blended whole
    on the host, under the same np.random seed."""
    from nerf_sampling_amd.run_nerf_helpers import NeRF
    from nerf_sampling_amd.trainers import FieldFitter

    images4, poses, _ = _scene("33x20")
    split = dict(images=images4, poses=poses, hwf=[33, 20, 15.0], i_train=np.array([1, 2]))
    fitter = FieldFitter(NeRF(D=2, W=32, input_ch=63, input_ch_views=27, output_ch=5, skips=[], use_viewdirs=True).cuda(),
                         N_samples=8, N_importance=0, white_bkgd=True)
    got = {}
    for mode in (False, "gather"):
        draw = fitter._blender_source(split, 64, device_batches=mode)
        np.random.seed(8)
        got[mode] = [draw(i) for i in range(3)]
    for (rays, target), (e_rays, e_target) in zip(got["gather"], got[False]):
        assert torch.equal(rays, e_rays) and torch.equal(target, e_target)
    with pytest.raises(ValueError):
        fitter.fit(lambda: got[False][0], 1, device_batches="draw")


def _training_setup(gpu_modules, H=24, W=24):
    from test_gpu_render import make_trainer, render_kwargs

    from nerf_sampling_amd import ops
    from nerf_sampling_amd.ray_batches import DeviceRayDataset

    ops.set_compute_dtype("f32")
    base = dict(gpu_modules("tiny_synth"))
    _, K = O.blender_intrinsics(H, W)
    rng = np.random.default_rng(17)
    images = rng.random((3, H, W, 3), dtype=np.float32)
    poses = np.stack([O.pose_spherical(a, -30.0, 4.0).numpy() for a in (20.0, 140.0, 260.0)]).astype(np.float32)
    ds = DeviceRayDataset(images, poses, K, [0, 1, 2])

    def fresh():
        m = dict(base)
        m["depth"] = copy.deepcopy(base["depth"])
        for p in m["depth"].parameters():
            p.requires_grad_(True)
        tr = make_trainer()
        kw = render_kwargs(tr, m)
        tr.H, tr.W, tr.K = H, W, K
        kw.update(near=2.0, far=6.0, ndc=False)
        return m, tr, kw

    return ds, fresh


def test_graphed_step_with_a_captured_batch_source_equals_eager(gpu_modules):
    """Six steps in 'draw' mode, set up as test_graphed_step_equals_eager_step: two eager warm-up steps, the capture (draw launch
    + counter increment + step), four replays -- the pre-crop window ends after the third step, inside the replays -- against
    eager steps fed by a source of the same seed.  Both losses and every DepthNet parameter bit for bit."""
    from nerf_sampling_amd.autograd import HipAdam
    from nerf_sampling_amd.ray_batches import DrawBatchSource, precrop_window

    ds, fresh = _training_setup(gpu_modules)
    crop = precrop_window(24, 24, 0.75)
    results = {}
    for mode in ("eager", "graph"):
        m, tr, kw = fresh()
        src = DrawBatchSource(ds, 128, seed=13, first_step=0, window_fn=lambda i: crop if i < 3 else None)
        opt = HipAdam(list(m["depth"].parameters()), lr=1e-3)
        opt.use_device_step()
        step = tr.graphed_optimization_loop(opt, kw, batch_source=src) if mode == "graph" else None
        losses = []
        for i in range(6):
            if mode == "graph":
                loss, dn_loss, _psnr, _ = step(None, i, None)
            else:
                rays, target = src(i)
                loss, dn_loss, _psnr, _ = tr.core_optimization_loop(opt, kw, rays, i, target)
            losses.append((float(loss), float(dn_loss)))
        if mode == "graph":
            assert step.graph is not None and step.calls == 6
        assert src.params.cpu().tolist() == [6, 0, 24, 0, 24]
        results[mode] = (losses, [p.detach().clone() for p in m["depth"].parameters()])
    assert results["eager"][0] == results["graph"][0], results
    assert all(torch.equal(a, b) for a, b in zip(results["eager"][1], results["graph"][1]))
    assert len(set(results["eager"][0])) == 6                                     # six different batches


def test_optimization_loop_reduces_loss_in_draw_mode(gpu_modules):
    """test_core_optimization_loop_reduces_loss with the batches drawn on the device (Trainer(device_batches='draw')): eight
    updates; the depth regression loss goes down and only DepthNet weights move.  That test steps on one fixed batch, so its
    losses are comparable; here every step draws anew, and the loss of a 256-ray batch depends on which rays it holds (measured:
    0.3 .. 2.5 between batches of the untrained net, more than eight updates move it).  So the batch is the WHOLE pre-crop window,
    16 x 16 of one 24 x 24 image: each step sees the same 256 rays in a fresh order, and the losses are comparable again."""
    from nerf_sampling_amd.autograd import HipAdam

    ds, fresh = _training_setup(gpu_modules)
    m, tr, kw = fresh()
    tr.device_batches, tr.batch_seed, tr.N_rand = "draw", 2, 256
    tr.precrop_iters, tr.precrop_frac = 100, 0.67                               # rows and columns 4..20
    tr._ray_dataset = ds
    opt = HipAdam(list(m["depth"].parameters()), lr=1e-3)
    fine_before = [p.clone() for p in m["fine"].parameters()]
    losses = []
    for i in range(8):
        _, _, rays, target = tr.sample_random_ray_batch(None, None, np.array([1]), None, None, i)
        if i == 0:
            first = rays[1].clone()
        else:                                                                   # the same rays, another order
            assert not torch.equal(rays[1], first)
            assert torch.equal(torch.sort(rays[1][:, 0]).values, torch.sort(first[:, 0]).values)
        loss, dn_loss, psnr, _ = tr.core_optimization_loop(opt, kw, rays, i, target)
        losses.append(float(dn_loss))
    print("depth_net_loss:", [round(x, 5) for x in losses])
    assert losses[-1] < losses[0]
    assert all(torch.equal(a, b) for a, b in zip(fine_before, m["fine"].parameters()))


def test_train_loop_end_to_end_in_draw_mode(tmp_path, gpu_modules):
    """DepthNetTrainer.train(device_batches='draw') with the graphed step: the draw is captured with the step (no host batch
    is made), the pre-crop ends during the replays, checkpoints appear as usual."""
    import os

    from test_render_path import _write_dataset

    from nerf_sampling_amd import ops
    from nerf_sampling_amd.trainers import DepthNetTrainer

    ops.set_compute_dtype("f32")
    m = gpu_modules("tiny_synth")
    rng = np.random.default_rng(3)
    H = W = 20
    frames = [np.concatenate([rng.integers(0, 256, (H, W, 3), dtype=np.uint8), np.full((H, W, 1), 255, np.uint8)], -1)
              for _ in range(3)]
    poses = [O.pose_spherical(a, -30.0, 4.0).numpy() for a in (0.0, 120.0, 240.0)]
    data, logs = str(tmp_path / "data"), str(tmp_path / "logs")
    _write_dataset(data, {"train": frames, "val": frames[:1], "test": frames[:1]},
                   {"train": poses, "val": poses[:1], "test": poses[:1]})
    nerf_ckpt = str(tmp_path / "nerf.tar")
    both = list(m["coarse"].parameters()) + list(m["fine"].parameters())
    torch.save({"global_step": 0, "network_fn_state_dict": m["coarse"].state_dict(),
                "network_fine_state_dict": m["fine"].state_dict(),
                "optimizer_state_dict": torch.optim.Adam(both).state_dict()}, nerf_ckpt)
    kw = dict(dataset_type="blender", basedir=logs, expname="exp", no_batching=True, datadir=data, half_res=False,
              white_bkgd=True, testskip=1, device="cuda", N_rand=64, N_importance=128, N_samples=64, use_viewdirs=True,
              input_dims_embed=3, netdepth=4, netwidth=128, netdepth_fine=4, netwidth_fine=128, n_layers=3,
              layer_width=128, sphere_radius=2.0, ft_path=nerf_ckpt, depth_net_lr=1e-3, train_depth_net_only=True,
              i_weights=6, i_print=3, perturb=0.0, precrop_iters=4, precrop_frac=0.5, device_batches="draw")
    tr = DepthNetTrainer(**kw)
    called = []
    tr.sample_random_ray_batch = lambda *a, **k: called.append(1)                 # the graphed step draws its own batches
    psnr = tr.train(N_iters=7)
    assert psnr is not None and np.isfinite(float(psnr)) and not called
    assert tr._draw_source.params.cpu().tolist() == [7, 0, 20, 0, 20]              # iterations 1..6 drawn, the crop lifted
    assert sorted(f for f in os.listdir(os.path.join(logs, "exp")) if f.endswith(".tar")) == ["000006.tar"]
