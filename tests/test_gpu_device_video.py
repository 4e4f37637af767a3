"""The turntable's two sequences written on the device (nerf_utils.write_video, Trainer(device_video=True)) against the route
they stand in for -- render_path, then numpy's to8b(rgbs) and to8b(disps / np.max(disps)) (Trainer.py:350-376): every PNG
decodes to those bytes, bit for bit, and the maximum read back once is numpy's.

The scene is the fitted one (tests/golden/fitted_scene) at 24 x 24 through a lens four times the Blender one, from three
poses chosen with the CPU oracle so that no ray leaves the shapes: a single ray without opacity has disparity 1e10, which
makes that the maximum and every other pixel of the reference's sequence 0.  The test asserts that the expected sequence is
not such a degenerate one before it compares anything."""

import os
import warnings

import numpy as np
import pytest
import torch

import test_gpu_device_eval as E
import test_gpu_map_to8b as T

pytestmark = pytest.mark.gpu

H = W = 24
LENS = 4.0
ANGLES = [(270.0, -15.0), (45.0, -75.0), (0.0, -60.0)]          # (theta, phi) of pose_spherical at radius 4


def _camera():
    from nerf_sampling_amd.synthetic import blender_intrinsics, pose_spherical

    focal = blender_intrinsics(H, W)[0] * LENS
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = torch.stack([pose_spherical(t, p, 4.0) for t, p in ANGLES]).float()
    return (H, W, focal), K, poses


def _png(path):
    from PIL import Image

    with Image.open(path) as im:
        return im.mode, np.array(im)


def _produced(tmp_dir):
    """what a call left in its directory, the mp4s of a machine that has imageio aside"""
    return sorted(n for n in os.listdir(tmp_dir) if not n.endswith(".mp4"))


def _check_sequences(base, rgbs, disps, out, n):
    """{base}rgb/ and {base}disp/ against numpy on render_path's arrays; ``out``: what write_video returned"""
    from nerf_sampling_amd.run_nerf_helpers import to8b

    nan = np.isnan(disps)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = np.float32(np.nanmax(disps)) if not nan.all() else np.float32(-np.inf)
    want = T.expected(disps, m)
    names = [f"{k:03d}.png" for k in range(n)]
    assert sorted(os.listdir(base + "rgb")) == names and sorted(os.listdir(base + "disp")) == names
    for k, name in enumerate(names):
        mode, got = _png(os.path.join(base + "rgb", name))
        assert mode == "RGB" and got.shape == (H, W, 3) and np.array_equal(got, to8b(rgbs[k])), name
        mode, got = _png(os.path.join(base + "disp", name))
        assert mode == "L" and got.dtype == np.uint8 and got.shape == (H, W), name
        assert np.array_equal(got, want[k].reshape(H, W)), (name, int((got != want[k].reshape(H, W)).sum()))
    assert out["n_views"] == n and out["disp_max"] == float(m) and out["has_nan"] is bool(nan.any())
    return want


@pytest.mark.parametrize("frame", ["depthnet", "full_nerf"])
def test_write_video_is_render_path_and_numpy(tmp_path, gpu_modules, frame):
    from nerf_sampling_amd import nerf_utils

    E._set_dtype("f32")
    over = dict(use_full_nerf=True) if frame == "full_nerf" else dict(sampling_mode="uniform", n_depth_samples=16)
    kw = E._kwargs(gpu_modules("shapes_fit"), **over)
    hwf, K, poses = _camera()
    with torch.no_grad():
        rgbs, disps, _ = nerf_utils.render_path(poses, hwf, K, 200, kw, step=0)
    assert rgbs.shape == (3, H, W, 3) and disps.shape == (3, H, W) and disps.dtype == np.float32
    base = str(tmp_path / "exp_spiral_000002_")
    out = nerf_utils.write_video(poses, hwf, K, kw, base, return_maps=True)
    print(frame, "disp min / max", float(np.nanmin(disps)), float(np.nanmax(disps)), "reported", out["disp_max"], out["has_nan"])
    want = _check_sequences(base, rgbs, disps, out, 3)
    # the comparison above is not one of black frames: render_path's own sequence has grey levels and is mostly lit
    assert len(np.unique(want)) >= 16 and (want != 0).mean() >= 0.25, (len(np.unique(want)), float((want != 0).mean()))
    assert _produced(str(tmp_path)) == ["exp_spiral_000002_disp", "exp_spiral_000002_rgb"]
    maps = out["maps"]
    assert maps.is_cuda and tuple(maps.shape) == (3, H * W) and np.array_equal(maps.cpu().numpy().reshape(3, H, W), disps)
    # one slot and one worker, another compression: the same pixels
    other = str(tmp_path / "other_")
    again = nerf_utils.write_video(poses, hwf, K, kw, other, n_buffers=1, workers=1, compress_level=1)
    assert set(again) == {"n_views", "disp_max", "has_nan"} and again["disp_max"] == out["disp_max"]
    _check_sequences(other, rgbs, disps, again, 3)


def test_nan_maps_and_the_interleaved_layout_through_the_workflow(tmp_path, monkeypatch):
    """a renderer that hands back prepared frames, NaNs among their disparities and the [:, 3] column of a shard as the map:
    the maximum is the one over the values that are not NaN, NaN pixels are 0, has_nan says so; a sequence of nothing but NaN has
    the maximum -inf and black frames"""
    from nerf_sampling_amd import nerf_utils

    rng = np.random.default_rng(77)
    rgbs = rng.random((4, H, W, 3), dtype=np.float32)
    disps = (rng.random((4, H, W), dtype=np.float32) * np.float32(0.3) + np.float32(0.1))
    disps[2, 5, 7] = 0.6                                               # the maximum lies in the third frame
    disps[0, :3] = np.nan
    disps[3, 10, 10] = np.nan
    for name, d in (("some", disps), ("all", np.full((2, H, W), np.nan, np.float32))):
        served = iter(range(len(d)))

        def render_frame(c2w, workspace, d=d, served=served):
            k = next(served)
            shard = torch.full((H * W, 4), 9.0, device="cuda")
            shard[:, :3] = torch.from_numpy(rgbs[k].reshape(-1, 3))
            shard[:, 3] = torch.from_numpy(d[k].reshape(-1))
            return shard[:, :3], shard[:, 3]

        monkeypatch.setattr(nerf_utils, "_one_call_frame_renderer", lambda *a, **k: render_frame)
        base = str(tmp_path / f"{name}_")
        out = nerf_utils.write_video([torch.eye(4)] * len(d), (H, W, 1.0), None, dict(trainer=None), base)
        want = _check_sequences(base, rgbs, d, out, len(d))
        assert out["has_nan"] is True
        if name == "some":
            assert out["disp_max"] == float(np.float32(0.6)) and want[2, 5, 7] == 255 and (want[0, :3] == 0).all()
        else:
            assert out["disp_max"] == -np.inf and not want.any()


def test_an_ineligible_configuration_writes_the_same_files_through_render_path(tmp_path, gpu_modules):
    """a query function that is not the standard one: render_path and numpy, with the warning"""
    from nerf_sampling_amd import nerf_utils

    E._set_dtype("f32")
    kw = E._kwargs(gpu_modules("tiny_synth"), sampling_mode="uniform", n_depth_samples=4)
    std = kw["network_query_fn"]
    kw["network_query_fn"] = lambda i, v, f: std(i, v, f)
    hwf, K, poses = _camera()
    with torch.no_grad():
        rgbs, disps, _ = nerf_utils.render_path(poses[:2], hwf, K, 200, kw, step=0)
    nerf_utils._evaluate_fallback_warned = False
    base = str(tmp_path / "fallback_")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = nerf_utils.write_video(poses[:2], hwf, K, kw, base)
    assert any("render_path" in str(w.message) for w in caught)
    _check_sequences(base, rgbs, disps, out, 2)


def test_trainer_render_writes_the_spiral(tmp_path, gpu_modules):
    """Trainer.render without render_test under device_eval + device_video: renderonly_path_*/rgb and /disp"""
    from nerf_sampling_amd import nerf_utils, ops

    ops.set_compute_dtype("f32")
    kw = E._kwargs(gpu_modules("tiny_synth"), sampling_mode="uniform", n_depth_samples=4, device_eval=True, device_video=True,
                   basedir=str(tmp_path / "r"), chunk=200)
    hwf, K, poses = _camera()
    tr = kw["trainer"]
    tr.K, tr.global_step = K, 7
    assert tr.render(False, False, None, [], poses, hwf, kw) == 0.0
    d = os.path.join(tr.basedir, tr.expname, "renderonly_path_000007")
    assert _produced(d) == ["disp", "rgb"]
    with torch.no_grad():
        rgbs, disps, _ = nerf_utils.render_path(poses, hwf, K, 200, kw, step=0)
    state = {"n_views": 3, "disp_max": float(np.nanmax(disps)), "has_nan": bool(np.isnan(disps).any())}
    _check_sequences(os.path.join(d, ""), rgbs, disps, state, 3)


def test_train_honours_i_video_only_under_device_video(tmp_path, gpu_modules, capsys):
    """i_video=2 over four iterations: with device_video the ..._spiral_000002_ and ..._spiral_000004_ sets of the 40 render
    poses and nothing else new; without it no set at all -- i_video stays unread -- and every other file of the run (the
    progress psnr.txt, the test set's psnr.txt) has the same bytes in both runs: the videos leave the training alone"""
    from nerf_sampling_amd import ops
    from nerf_sampling_amd.synthetic import pose_spherical
    from nerf_sampling_amd.trainers import DepthNetTrainer

    ops.set_compute_dtype("f32")
    m = gpu_modules("tiny_synth")
    rng = np.random.default_rng(3)
    frames = [E._rgba(rng, E.H, E.W) for _ in range(5)]
    poses = [pose_spherical(a, -30.0, 4.0).numpy() for a in (0.0, 72.0, 144.0, 216.0, 288.0)]
    data = str(tmp_path / "data")
    E._write_dataset(data, {"train": frames[:2], "val": frames[:1], "test": frames[2:]},
                     {"train": poses[:2], "val": poses[:1], "test": poses[2:]})
    nerf_ckpt = str(tmp_path / "nerf.tar")
    both = list(m["coarse"].parameters()) + list(m["fine"].parameters())
    torch.save({"global_step": 0, "network_fn_state_dict": m["coarse"].state_dict(),
                "network_fine_state_dict": m["fine"].state_dict(),
                "optimizer_state_dict": torch.optim.Adam(both).state_dict()}, nerf_ckpt)
    files = {}
    for on in (False, True):
        logs = str(tmp_path / f"logs_{int(on)}")
        np.random.seed(0); torch.manual_seed(0)
        tr = DepthNetTrainer(dataset_type="blender", basedir=logs, expname="exp", no_batching=True, datadir=data, half_res=False,
                             white_bkgd=True, testskip=1, device="cuda", N_rand=128, N_importance=128, N_samples=64,
                             use_viewdirs=True, input_dims_embed=3, netdepth=4, netwidth=128, netdepth_fine=4, netwidth_fine=128,
                             n_layers=3, layer_width=128, sphere_radius=2.0, ft_path=nerf_ckpt, depth_net_lr=1e-3,
                             train_depth_net_only=True, i_weights=100, i_print=1, perturb=1.0, i_testset=3, i_video=2,
                             n_depth_samples=8, sampling_mode="uniform", distance=0.1, hip_graph=False, device_eval=True,
                             device_video=on)
        assert tr.train(N_iters=5) is not None                                           # iterations 1..4
        text = capsys.readouterr().out
        exp = os.path.join(logs, "exp")
        sets = sorted(d for d in _produced(exp) if "_spiral_" in d)
        if on:
            assert sets == [f"exp_spiral_{i:06d}_{kind}" for i in (2, 4) for kind in ("disp", "rgb")]
            for d in sets:
                names = sorted(os.listdir(os.path.join(exp, d)))
                assert names == [f"{k:03d}.png" for k in range(40)], d
                mode, img = _png(os.path.join(exp, d, "017.png"))
                assert img.shape[:2] == (E.H, E.W) and mode == ("L" if d.endswith("disp") else "RGB")
            assert "Iter: 2 spiral of 40 views" in text and "Iter: 4 spiral of 40 views" in text
        else:
            assert sets == [] and "spiral" not in text
        rest = {}
        for root, _dirs, names in os.walk(exp):
            if "_spiral_" in root:
                continue
            for n in names:
                if not n.endswith(".mp4"):
                    rest[os.path.relpath(os.path.join(root, n), exp)] = open(os.path.join(root, n), "rb").read()
        files[on] = rest
    assert sorted(files[False]) == ["psnr.txt", os.path.join("testset_000003", "psnr.txt")]
    assert files[True] == files[False]
