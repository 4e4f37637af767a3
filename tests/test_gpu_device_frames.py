"""The frames of the device evaluation as PNGs (nerf_utils.FrameWriter behind evaluate_views / score_views(frames=True),
write_views, Trainer(device_frames=True), FieldFitter.fit(test_frames=True)) on the tiny scenes of tests/test_gpu_device_eval.py:
every file decodes to to8b of the frame the evaluation rendered, bit for bit, and is the file render_path's own
``Image.fromarray(to8b(rgb)).save`` writes; the scores and their text files keep their bytes."""

import copy
import io
import os
import threading

import numpy as np
import pytest
import torch

import test_gpu_device_eval as E

pytestmark = pytest.mark.gpu

H, W, TEST_IDS = E.H, E.W, E.TEST_IDS


def _to8b(frame, h=H, w=W):
    from nerf_sampling_amd.run_nerf_helpers import to8b

    return to8b(frame.cpu().numpy().reshape(h, w, 3))


def _png(path):
    from PIL import Image

    with Image.open(path) as im:
        return np.array(im)


def _png_bytes(rgb8, **save_kw):
    """the file render_path's call writes for these pixels (nerf_utils.py:311 here, :322-325 in the reference)"""
    from PIL import Image

    f = io.BytesIO()
    Image.fromarray(rgb8).save(f, format="PNG", **save_kw)
    return f.getvalue()


def _check_files(savedir, frames, extra=("psnr.txt",), h=H, w=W, **save_kw):
    names = [f"{k:03d}.png" for k in range(len(frames))]
    assert sorted(os.listdir(savedir)) == sorted(names + list(extra))
    for name, frame in zip(names, frames):
        want = _to8b(frame, h, w)
        got = _png(os.path.join(savedir, name))
        assert got.dtype == np.uint8 and got.shape == (h, w, 3) and np.array_equal(got, want), name
        assert open(os.path.join(savedir, name), "rb").read() == _png_bytes(want, **save_kw), name


def _eval(kw, savedir, ids=TEST_IDS, **opts):
    from nerf_sampling_amd import nerf_utils

    images, poses, focal, K, ds = E._scene()
    return nerf_utils.evaluate_views(ds, ids, torch.from_numpy(poses[ids]), (H, W, focal), K, kw, savedir=savedir, **opts)


@pytest.mark.parametrize("ssim", [False, True])
def test_evaluate_views_writes_the_frames_and_keeps_the_scores(tmp_path, gpu_modules, ssim):
    E._set_dtype("bf16")
    kw = E._kwargs(gpu_modules("tiny_synth"), sampling_mode="uniform", n_depth_samples=8)
    off, on = str(tmp_path / "off"), str(tmp_path / "on")
    plain = _eval(kw, off, ssim=ssim)
    got = _eval(kw, on, ssim=ssim, frames=True, return_frames=True)
    texts = ("psnr.txt", "ssim.txt") if ssim else ("psnr.txt",)
    assert sorted(os.listdir(off)) == sorted(texts)                                  # off: no PNG, as before
    _check_files(on, got[-1], extra=texts)
    for name in texts:
        assert open(os.path.join(on, name), "rb").read() == open(os.path.join(off, name), "rb").read()
    assert len(got) == len(plain) + 1
    for a, b in zip(plain, got):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert len({open(os.path.join(on, f"{k:03d}.png"), "rb").read() for k in range(3)}) == 3


@pytest.mark.parametrize("n_buffers,workers", [(2, 1), (1, 1), (1, 4), (3, 8)])
def test_few_slots_many_views(tmp_path, gpu_modules, n_buffers, workers):
    """five views through one or two slots: a slot that was reused before its copy or its file was done would show the next
    view's pixels"""
    E._set_dtype("f32")
    kw = E._kwargs(gpu_modules("tiny_synth"), sampling_mode="uniform", n_depth_samples=2)
    out = _eval(kw, str(tmp_path), ids=[0, 1, 2, 3, 4], frames=dict(n_buffers=n_buffers, workers=workers), return_frames=True)
    assert len(out[-1]) == 5
    _check_files(str(tmp_path), out[-1])


def test_frame_writer_alone(tmp_path):
    """twelve random 37 x 29 frames with an alpha channel through two slots and three workers at compress_level 1; put after
    close is refused, close twice is fine, and the writer holds no frame"""
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.run_nerf_helpers import to8b

    h, w = 37, 29
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    frames = [torch.rand(h * w, 3, device="cuda", generator=gen) * 1.2 - 0.1 for _ in range(12)]
    alphas = [torch.rand(h * w, device="cuda", generator=gen) for _ in range(12)]
    writer = nerf_utils.FrameWriter(str(tmp_path), h, w, channels=4, n_buffers=2, workers=3, compress_level=1)
    capped = nerf_utils.FrameWriter(str(tmp_path), h, w, workers=50)                 # never more than MAX_WORKERS threads
    assert writer.workers == 3 and capped.workers == 8 and len(capped._threads) == 8
    capped.close()
    for k, (f, a) in enumerate(zip(frames, alphas)):
        writer.put(k, f, a if k % 2 == 0 else None)
    writer.close()
    writer.close()
    assert writer.n_written == 12 and writer._dev is None and writer._host is None
    with pytest.raises(RuntimeError):
        writer.put(12, frames[0])
    for k, (f, a) in enumerate(zip(frames, alphas)):
        a8 = to8b(a.cpu().numpy().reshape(h, w, 1)) if k % 2 == 0 else np.full((h, w, 1), 255, np.uint8)
        want = np.concatenate([_to8b(f, h, w), a8], -1)
        path = os.path.join(str(tmp_path), f"{k:03d}.png")
        assert np.array_equal(_png(path), want), k
        assert open(path, "rb").read() == _png_bytes(want, compress_level=1)
    with nerf_utils.FrameWriter(str(tmp_path / "bad"), h, w) as wr:
        with pytest.raises(ValueError):
            wr.put(0, frames[0][:-1])                                                # refused before a slot is taken
        for k in range(6):
            wr.put(k, frames[k])
    assert sorted(os.listdir(str(tmp_path / "bad"))) == [f"{k:03d}.png" for k in range(6)]


def test_an_interleaved_frame_source_gives_the_same_files(tmp_path, gpu_modules):
    """the [:, :3] view of an [R,4] shard (the fused renderer's layout), its fourth float NaN"""
    from nerf_sampling_amd import nerf_utils

    E._set_dtype("f32")
    kw = E._kwargs(gpu_modules("tiny_synth"), sampling_mode="uniform", n_depth_samples=4)
    packed_dir, shard_dir = str(tmp_path / "packed"), str(tmp_path / "shard")
    psnrs, _avg, frames = _eval(kw, packed_dir, frames=True, return_frames=True)
    images, poses, focal, K, ds = E._scene()
    served = iter(frames)

    def render_frame(c2w, workspace):
        shard = torch.full((H * W, 4), float("nan"), device="cuda")
        shard[:, :3] = next(served)
        return shard[:, :3]

    got = nerf_utils.score_views(ds, TEST_IDS, torch.from_numpy(poses[TEST_IDS]), render_frame, savedir=shard_dir, frames=True)
    assert np.array_equal(got[0], psnrs)
    _check_files(shard_dir, frames)
    for name in sorted(os.listdir(packed_dir)):
        assert open(os.path.join(packed_dir, name), "rb").read() == open(os.path.join(shard_dir, name), "rb").read(), name


def test_a_worker_failure_surfaces_and_the_next_call_works(tmp_path, gpu_modules, monkeypatch):
    """savedir turns into a regular file behind the writer's back: the workers' NotADirectoryError comes out of the
    evaluate_views call, which returns instead of waiting for slots nobody frees"""
    from nerf_sampling_amd import nerf_utils

    E._set_dtype("f32")
    kw = E._kwargs(gpu_modules("tiny_synth"), sampling_mode="uniform", n_depth_samples=2)
    bad, good = str(tmp_path / "bad"), str(tmp_path / "good")
    made = []

    class Sabotaged(nerf_utils.FrameWriter):
        def __init__(self, savedir, *a, **k):
            super().__init__(savedir, *a, **k)
            os.rmdir(savedir)
            open(savedir, "w").close()
            made.append(self)

    monkeypatch.setattr(nerf_utils, "FrameWriter", Sabotaged)
    result = {}

    def call():
        try:
            result["out"] = _eval(kw, bad, ids=[0, 1, 2, 3, 4], frames=dict(n_buffers=1, workers=1))
        except BaseException as e:  # noqa: BLE001
            result["error"] = e

    t = threading.Thread(target=call)
    t.start()
    t.join(timeout=120)
    assert not t.is_alive(), "evaluate_views hangs after its workers failed"
    assert isinstance(result.get("error"), NotADirectoryError), result
    assert os.path.isfile(bad) and len(made) == 1 and made[0]._closed and made[0]._dev is None and made[0].n_written == 0
    monkeypatch.undo()
    out = _eval(kw, good, frames=True, return_frames=True)
    _check_files(good, out[-1])


def test_an_exception_of_the_loop_is_the_one_that_surfaces(tmp_path, gpu_modules):
    """the renderer fails on the third view: the writer is closed (two files, no thread left) and the renderer's error is
    the one raised"""
    from nerf_sampling_amd import nerf_utils

    images, poses, focal, K, ds = E._scene()
    before = threading.active_count()
    frame = torch.rand(H * W, 3, device="cuda")
    calls = []

    def render_frame(c2w, workspace):
        calls.append(1)
        if len(calls) == 3:
            raise KeyError("the renderer's own")
        return frame

    with pytest.raises(KeyError):
        nerf_utils.score_views(ds, TEST_IDS, torch.from_numpy(poses[TEST_IDS]), render_frame, savedir=str(tmp_path), frames=True)
    assert sorted(os.listdir(str(tmp_path))) == ["000.png", "001.png"] and threading.active_count() == before


def test_write_views_on_three_poses(tmp_path, gpu_modules):
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.synthetic import pose_spherical

    E._set_dtype("bf16")
    images, _poses, focal, K, ds = E._scene()
    kw = E._kwargs(gpu_modules("tiny_synth"), sampling_mode="uniform", n_depth_samples=8)
    spiral = torch.stack([pose_spherical(a, -30.0, 4.0) for a in (-180.0, -60.0, 60.0)]).float()
    n, frames = nerf_utils.write_views(spiral, (H, W, focal), K, kw, str(tmp_path / "a"), return_frames=True)
    assert n == 3 and len(frames) == 3
    _check_files(str(tmp_path / "a"), frames, extra=())
    assert nerf_utils.write_views(spiral, (H, W, focal), K, kw, str(tmp_path / "b"), n_buffers=1, workers=2) == 3
    for k in range(3):
        assert open(str(tmp_path / "a" / f"{k:03d}.png"), "rb").read() == open(str(tmp_path / "b" / f"{k:03d}.png"), "rb").read()


def test_trainer_render_with_device_frames(tmp_path, gpu_modules):
    """Trainer.render under device_eval + device_frames: the test views as evaluate_views(frames=True) writes them, and the
    poses without ground truth through write_views"""
    from nerf_sampling_amd import ops

    ops.set_compute_dtype("f32")
    images, poses, focal, K, ds = E._scene()
    kw = E._kwargs(gpu_modules("tiny_synth"), sampling_mode="uniform", n_depth_samples=4, device_eval=True, device_frames=True,
                   basedir=str(tmp_path / "r"), chunk=200)
    tr = kw["trainer"]
    tr.K, tr.global_step = K, 7
    avg = tr.render(True, False, images, TEST_IDS, torch.from_numpy(poses[TEST_IDS]), (H, W, focal), kw)
    d = os.path.join(tr.basedir, tr.expname, "renderonly_test_000007")
    out = _eval(kw, str(tmp_path / "direct"), frames=True, return_frames=True)
    assert abs(float(avg) - out[1]) <= E.GATE_DB               # (render uploads a dataset of the test views alone)
    _check_files(d, out[-1])
    assert tr.render(False, False, images, TEST_IDS, torch.from_numpy(poses[:2]), (H, W, focal), kw) == 0.0
    path_dir = os.path.join(tr.basedir, tr.expname, "renderonly_path_000007")
    _check_files(path_dir, _eval(kw, None, ids=[0, 1], return_frames=True)[-1], extra=())


def test_train_writes_the_testset_frames(tmp_path, gpu_modules):
    """device_eval + device_frames, i_testset=2, three iterations: testset_000002/ holds the three views and psnr.txt"""
    from nerf_sampling_amd import ops
    from nerf_sampling_amd.synthetic import pose_spherical
    from nerf_sampling_amd.trainers import DepthNetTrainer

    ops.set_compute_dtype("f32")
    m = gpu_modules("tiny_synth")
    rng = np.random.default_rng(3)
    frames = [E._rgba(rng, H, W) for _ in range(5)]
    poses = [pose_spherical(a, -30.0, 4.0).numpy() for a in (0.0, 72.0, 144.0, 216.0, 288.0)]
    data = str(tmp_path / "data")
    E._write_dataset(data, {"train": frames[:2], "val": frames[:1], "test": frames[2:]},
                     {"train": poses[:2], "val": poses[:1], "test": poses[2:]})
    nerf_ckpt = str(tmp_path / "nerf.tar")
    both = list(m["coarse"].parameters()) + list(m["fine"].parameters())
    torch.save({"global_step": 0, "network_fn_state_dict": m["coarse"].state_dict(),
                "network_fine_state_dict": m["fine"].state_dict(),
                "optimizer_state_dict": torch.optim.Adam(both).state_dict()}, nerf_ckpt)
    logs = str(tmp_path / "logs")
    np.random.seed(0); torch.manual_seed(0)
    tr = DepthNetTrainer(dataset_type="blender", basedir=logs, expname="exp", no_batching=True, datadir=data, half_res=False,
                         white_bkgd=True, testskip=1, device="cuda", N_rand=128, N_importance=128, N_samples=64,
                         use_viewdirs=True, input_dims_embed=3, netdepth=4, netwidth=128, netdepth_fine=4, netwidth_fine=128,
                         n_layers=3, layer_width=128, sphere_radius=2.0, ft_path=nerf_ckpt, depth_net_lr=1e-3,
                         train_depth_net_only=True, i_weights=100, i_print=100, perturb=1.0, i_testset=2, n_depth_samples=8,
                         sampling_mode="uniform", distance=0.1, hip_graph=False, device_eval=True, device_frames=True)
    assert tr.train(N_iters=4) is not None                                           # iterations 1..3
    exp = os.path.join(logs, "exp")
    assert sorted(d for d in os.listdir(exp) if d.startswith("testset_")) == ["testset_000002"]
    d = os.path.join(exp, "testset_000002")
    assert sorted(os.listdir(d)) == ["000.png", "001.png", "002.png", "psnr.txt"]
    vals, avg = E._parse(os.path.join(d, "psnr.txt"), 3)
    assert np.isfinite(vals).all()
    decoded = [_png(os.path.join(d, f"{k:03d}.png")) for k in range(3)]
    assert all(p.shape == (H, W, 3) and p.dtype == np.uint8 for p in decoded)
    # psnr.txt scores the fp32 frame, the PNG holds it to 8 bits: the PSNR of the decoded file agrees to quantisation
    gt = np.stack([f[..., :3].astype(np.float32) / np.float32(255) for f in frames[2:]])
    for p, g, v in zip(decoded, gt, vals):
        mse8 = np.mean((p.astype(np.float64) / 255.0 - g) ** 2)
        assert abs(-10.0 * np.log10(mse8) - v) < 0.1, (v, mse8)


def test_field_fit_writes_the_testset_frames(tmp_path, gpu_modules):
    """FieldFitter.fit(i_testset=2, test_frames=True), two steps: the files are those of evaluate_views on the final weights"""
    from nerf_sampling_amd import ops
    from nerf_sampling_amd.ray_batches import DeviceRayDataset
    from nerf_sampling_amd.synthetic import pose_spherical
    from nerf_sampling_amd.trainers import FieldFitter

    ops.set_compute_dtype("f32")
    Hf, Wf, focal = 33, 20, 28.0
    rng = np.random.default_rng(3320)
    images4 = rng.random((4, Hf, Wf, 4), dtype=np.float32)
    poses = np.stack([pose_spherical(a, -30.0, 4.0).numpy() for a in (10.0, 100.0, 190.0, 280.0)]).astype(np.float32)
    split = dict(images=images4, poses=poses, hwf=[Hf, Wf, focal], i_train=np.array([0, 1]), i_test=np.array([2, 3]))
    base = gpu_modules("tiny_synth")
    nets = {}
    for k in ("coarse", "fine"):
        nets[k] = copy.deepcopy(base[k])
        for p in nets[k].parameters():
            p.requires_grad_(True)
    fitter = FieldFitter(nets["coarse"], nets["fine"], N_samples=8, N_importance=8, white_bkgd=True, lindisp=False, perturb=1.0)
    np.random.seed(1); torch.manual_seed(1)
    fitter.fit(split, 2, N_rand=64, basedir=str(tmp_path), expname="field", i_print=0, i_testset=2, test_frames=True)
    d = os.path.join(str(tmp_path), "field", "testset_000002")
    K = np.array([[focal, 0, 0.5 * Wf], [0, focal, 0.5 * Hf], [0, 0, 1]])
    ds = DeviceRayDataset(images4, poses, K, [0, 1], white_bkgd=True)
    out = fitter.evaluate_views(ds, [2, 3], poses[[2, 3]], [Hf, Wf, focal], K, return_frames=True)
    _check_files(d, out[-1], h=Hf, w=Wf)
    vals, _avg = E._parse(os.path.join(d, "psnr.txt"), 2)
    assert np.array_equal(vals, out[0])
