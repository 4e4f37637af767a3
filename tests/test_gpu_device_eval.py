"""Held-out views scored on the device (nerf_utils.evaluate_views, Trainer(device_eval=True), FieldFitter.fit(i_testset=...),
render.py --device-psnr) against render_path(gt_imgs=...), the host path they stand in for: 24 x 24 frames, three test views, the
small networks of the training tests.

The 1e-4 dB gate: both paths score the same frame bits; numpy's fp32 pairwise mean is off by at most about (log2 n + 1) 2^-24
relative, under 1e-5 dB even at 800 x 800, against the device's double sum -- the gate leaves a factor of ten."""

import copy
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 24
TEST_IDS = [2, 3, 4]
GATE_DB = 1e-4
_cache = {}


def _scene():
    """five random fp32 images [24,24,3] (two training, three test views), their poses, intrinsics and the device dataset"""
    if "scene" not in _cache:
        from nerf_sampling_amd.ray_batches import DeviceRayDataset
        from nerf_sampling_amd.synthetic import blender_intrinsics, pose_spherical

        focal, K = blender_intrinsics(H, W)
        images = np.random.default_rng(24).random((5, H, W, 3), dtype=np.float32)
        poses = np.stack([pose_spherical(a, -30.0, 4.0).numpy() for a in (0.0, 72.0, 144.0, 216.0, 288.0)]).astype(np.float32)
        _cache["scene"] = (images, poses, focal, K, DeviceRayDataset(images, poses, K, [0, 1]))
    return _cache["scene"]


def _kwargs(m, **trainer_over):
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.run_nerf_helpers import get_embedder
    from nerf_sampling_amd.trainers import DepthNetTrainer

    kw = dict(dataset_type="blender", basedir="/tmp", expname="eval", no_batching=True, datadir="", half_res=True,
              white_bkgd=True, N_importance=128, N_samples=64, use_viewdirs=True, input_dims_embed=3, device="cuda", distance=0.1)
    kw.update(trainer_over)
    tr = DepthNetTrainer(**kw)
    e1, _ = get_embedder(10, 0, 3)
    e2, _ = get_embedder(4, 0, 3)
    query = nerf_utils.standard_query_fn(lambda i, v, f: tr.run_network(i, v, f, embed_fn=e1, embeddirs_fn=e2))
    return dict(ndc=False, near=2.0, far=6.0, use_viewdirs=True, network_fn=m["coarse"], network_query_fn=query, N_samples=64,
                trainer=tr, network_fine=m["fine"], depth_network=m["depth"], white_bkgd=True, lindisp=True, perturb=0.0,
                raw_noise_std=0.0)


def _set_dtype(dtype):
    from nerf_sampling_amd import ops

    ops.set_compute_dtype(dtype)
    ops.set_psnr_guard(dtype != "f32")              # bf16 with the guard, f32 without


def _parse(path, n):
    """psnr.txt in render_path's layout -> (per-view values, average)"""
    lines = open(path).read().split("\n")
    assert len(lines) == n + 3 and lines[-1] == "" and lines[n] == f"Avg of {n} images:", lines
    vals = []
    for i in range(n):
        head = f"{i:03d}.png, PSNR: "
        assert lines[i].startswith(head), lines[i]
        vals.append(float(lines[i][len(head):]))
    assert lines[n + 1].startswith("PSNR: ")
    return np.array(vals), float(lines[n + 1][len("PSNR: "):])


def _host_psnr(frames, gt):
    """float64 PSNR of device frames [H*W,3] against ground truth [n,H,W,3]: the fp32 difference, everything after in double"""
    out = []
    for f, g in zip(frames, gt):
        d = (f.cpu().numpy().reshape(H, W, 3) - g).astype(np.float64)
        out.append(-10.0 * np.log10(np.sum(d * d) / d.size))
    return np.array(out)


def _check_own_frames(psnrs, avg, frames, gt):
    assert len(frames) == len(gt) and all(f.is_cuda and tuple(f.shape) == (H * W, 3) for f in frames)
    want = _host_psnr(frames, gt)
    print("reported", psnrs.tolist(), "host float64 of the returned frames", want.tolist())
    assert psnrs.dtype == np.float64 and np.isfinite(psnrs).all()
    np.testing.assert_allclose(psnrs, want, rtol=1e-9, atol=0)
    assert avg == float(np.mean(psnrs))


def _against_render_path(kw, tmp_path):
    from nerf_sampling_amd import nerf_utils

    images, poses, focal, K, ds = _scene()
    gt, test_poses = images[TEST_IDS], torch.from_numpy(poses[TEST_IDS])
    host_dir, dev_dir = str(tmp_path / "host"), str(tmp_path / "device")
    os.makedirs(host_dir)
    with torch.no_grad():
        rgbs, _disps, host_avg = nerf_utils.render_path(test_poses, (H, W, focal), K, 200, kw, step=0, gt_imgs=gt, savedir=host_dir)
    psnrs, avg, frames = nerf_utils.evaluate_views(ds, TEST_IDS, test_poses, (H, W, focal), K, kw, savedir=dev_dir,
                                                   return_frames=True)
    host_vals, host_avg_txt = _parse(os.path.join(host_dir, "psnr.txt"), 3)
    dev_vals, dev_avg_txt = _parse(os.path.join(dev_dir, "psnr.txt"), 3)
    same = [bool(np.array_equal(f.cpu().numpy().reshape(H, W, 3), r)) for f, r in zip(frames, rgbs)]
    print("render_path", host_vals.tolist(), "evaluate_views", psnrs.tolist(), "same frame bits", same)
    assert np.isfinite(host_vals).all()
    assert np.abs(psnrs - host_vals).max() <= GATE_DB and abs(avg - float(host_avg)) <= GATE_DB
    assert np.array_equal(dev_vals, psnrs) and dev_avg_txt == avg and abs(host_avg_txt - dev_avg_txt) <= GATE_DB
    assert os.listdir(dev_dir) == ["psnr.txt"]                                       # no PNG from the device path
    assert sorted(os.listdir(host_dir)) == ["000.png", "001.png", "002.png", "psnr.txt"]
    _check_own_frames(psnrs, avg, frames, gt)
    assert len(nerf_utils.evaluate_views(ds, TEST_IDS, test_poses, (H, W, focal), K, kw)) == 2


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("mode,n", [("uniform", 2), ("uniform", 64), ("depth_only", 1)])
def test_evaluate_views_equals_render_path(tmp_path, gpu_modules, mode, n, dtype):
    _set_dtype(dtype)
    _against_render_path(_kwargs(gpu_modules("tiny_synth"), sampling_mode=mode, n_depth_samples=n), tmp_path)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_gaussian_views_score_their_own_frames(gpu_modules, dtype):
    """Gaussian draws differ between a chunked and a whole-frame call, so the reported PSNR is checked against the frames the
    evaluation itself rendered; its draws leave the global generator alone."""
    from nerf_sampling_amd import nerf_utils

    _set_dtype(dtype)
    images, poses, focal, K, ds = _scene()
    kw = _kwargs(gpu_modules("tiny_synth"), sampling_mode="gaussian", n_depth_samples=16)
    state = torch.cuda.get_rng_state()
    psnrs, avg, frames = nerf_utils.evaluate_views(ds, TEST_IDS, torch.from_numpy(poses[TEST_IDS]), (H, W, focal), K, kw,
                                                   return_frames=True)
    assert torch.equal(torch.cuda.get_rng_state(), state)
    _check_own_frames(psnrs, avg, frames, images[TEST_IDS])
    assert len({f.cpu().numpy().tobytes() for f in frames}) == 3


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_full_nerf_views_through_the_hierarchical_renderer(tmp_path, gpu_modules, dtype):
    _set_dtype(dtype)
    _against_render_path(_kwargs(gpu_modules("tiny_synth"), use_full_nerf=True), tmp_path)


def test_ineligible_configuration_falls_back_to_render_path(gpu_modules):
    """a query function that is not the standard one: render_path's values, with a warning"""
    import warnings

    from nerf_sampling_amd import nerf_utils

    _set_dtype("f32")
    images, poses, focal, K, ds = _scene()
    kw = _kwargs(gpu_modules("tiny_synth"), sampling_mode="uniform", n_depth_samples=4)
    std = kw["network_query_fn"]
    want, _ = nerf_utils.evaluate_views(ds, TEST_IDS[:1], torch.from_numpy(poses[TEST_IDS[:1]]), (H, W, focal), K, kw)
    kw["network_query_fn"] = lambda i, v, f: std(i, v, f)
    nerf_utils._evaluate_fallback_warned = False
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got, avg = nerf_utils.evaluate_views(ds, TEST_IDS[:1], torch.from_numpy(poses[TEST_IDS[:1]]), (H, W, focal), K, kw)
    assert any("render_path" in str(w.message) for w in caught)
    assert got.shape == (1,) and abs(got[0] - want[0]) <= 1e-3 and abs(avg - got[0]) <= GATE_DB


# ---- the trainer -----------------------------------------------------------------------------------------------------
def _write_dataset(root, imgs_by_split, poses_by_split, angle=0.6911112070083618):
    """a Blender dataset on disk (tests/test_render_path.py's writer, restated)"""
    from PIL import Image

    for split, imgs in imgs_by_split.items():
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i, (im, pose) in enumerate(zip(imgs, poses_by_split[split])):
            Image.fromarray(im).save(os.path.join(root, split, f"r_{i}.png"))
            frames.append({"file_path": f"./{split}/r_{i}", "transform_matrix": np.asarray(pose).tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": angle, "frames": frames}, f)


def _rgba(rng, h, w):
    return np.concatenate([rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.full((h, w, 1), 255, np.uint8)], -1)


def test_train_honours_i_testset_and_leaves_the_step_alone(tmp_path, gpu_modules, capsys):
    """device_eval=True, i_testset=3, seven iterations on the graphed step: testset_000003 / _000006 hold three view lines and
    the average, and the final DepthNet equals the default run's bit for bit -- the evaluation disturbs neither the captured graph
    nor the generators the step draws from.  The default run writes no testset_* directory."""
    from nerf_sampling_amd import ops
    from nerf_sampling_amd.synthetic import pose_spherical
    from nerf_sampling_amd.trainers import DepthNetTrainer

    ops.set_compute_dtype("f32")
    m = gpu_modules("tiny_synth")
    rng = np.random.default_rng(3)
    frames = [_rgba(rng, H, W) for _ in range(5)]
    poses = [pose_spherical(a, -30.0, 4.0).numpy() for a in (0.0, 72.0, 144.0, 216.0, 288.0)]
    data = str(tmp_path / "data")
    _write_dataset(data, {"train": frames[:2], "val": frames[:1], "test": frames[2:]},
                   {"train": poses[:2], "val": poses[:1], "test": poses[2:]})
    nerf_ckpt = str(tmp_path / "nerf.tar")
    both = list(m["coarse"].parameters()) + list(m["fine"].parameters())
    torch.save({"global_step": 0, "network_fn_state_dict": m["coarse"].state_dict(),
                "network_fine_state_dict": m["fine"].state_dict(),
                "optimizer_state_dict": torch.optim.Adam(both).state_dict()}, nerf_ckpt)
    final = {}
    for on in (False, True):
        logs = str(tmp_path / f"logs_{int(on)}")
        kw = dict(dataset_type="blender", basedir=logs, expname="exp", no_batching=True, datadir=data, half_res=False,
                  white_bkgd=True, testskip=1, device="cuda", N_rand=128, N_importance=128, N_samples=64, use_viewdirs=True,
                  input_dims_embed=3, netdepth=4, netwidth=128, netdepth_fine=4, netwidth_fine=128, n_layers=3,
                  layer_width=128, sphere_radius=2.0, ft_path=nerf_ckpt, depth_net_lr=1e-3, train_depth_net_only=True,
                  i_weights=7, i_print=2, perturb=1.0, i_testset=3, n_depth_samples=8, sampling_mode="uniform", distance=0.1,
                  hip_graph=True, device_eval=on)
        np.random.seed(0); torch.manual_seed(0)
        tr = DepthNetTrainer(**kw)
        assert tr.train(N_iters=8) is not None                                   # iterations 1..7
        out = capsys.readouterr().out
        exp = os.path.join(logs, "exp")
        dirs = sorted(d for d in os.listdir(exp) if d.startswith("testset_"))
        if on:
            assert dirs == ["testset_000003", "testset_000006"]
            for d, it in zip(dirs, (3, 6)):
                assert os.listdir(os.path.join(exp, d)) == ["psnr.txt"]
                vals, avg = _parse(os.path.join(exp, d, "psnr.txt"), 3)
                assert np.isfinite(vals).all() and avg == float(np.mean(vals))
                assert f"[TRAIN] Iter: {it} test PSNR: {avg}" in out
        else:
            assert dirs == [] and "test PSNR" not in out
        final[on] = torch.load(os.path.join(exp, "000007.tar"), weights_only=True)["depth_network"]     # after both evaluations
    assert set(final[True]) == set(final[False])
    assert all(torch.equal(final[True][k], final[False][k]) for k in final[True])


def test_trainer_render_takes_the_device_path(tmp_path, gpu_modules):
    """Trainer.render(render_test=True) under device_eval: the same directory, psnr.txt and return value as render_path's,
    no PNG; without ground truth it keeps render_path."""
    from nerf_sampling_amd import ops

    ops.set_compute_dtype("f32")
    images, poses, focal, K, ds = _scene()
    out = {}
    for on in (False, True):
        kw = _kwargs(gpu_modules("tiny_synth"), sampling_mode="uniform", n_depth_samples=4, device_eval=on,
                     basedir=str(tmp_path / f"r{int(on)}"), chunk=200)
        tr = kw["trainer"]
        tr.K, tr.global_step = K, 7
        avg = tr.render(True, False, images, TEST_IDS, torch.from_numpy(poses[TEST_IDS]), (H, W, focal), kw)
        d = os.path.join(tr.basedir, tr.expname, "renderonly_test_000007")
        out[on] = (float(avg), _parse(os.path.join(d, "psnr.txt"), 3), sorted(os.listdir(d)))
    assert out[True][2] == ["psnr.txt"] and out[False][2] == ["000.png", "001.png", "002.png", "psnr.txt"]
    assert abs(out[True][0] - out[False][0]) <= GATE_DB and np.abs(out[True][1][0] - out[False][1][0]).max() <= GATE_DB
    tr.render(False, False, images, TEST_IDS, torch.from_numpy(poses[:1]), (H, W, focal), kw)
    assert sorted(os.listdir(os.path.join(tr.basedir, tr.expname, "renderonly_path_000007"))) == ["000.png"]


# ---- the field fit ---------------------------------------------------------------------------------------------------
def test_field_fit_reports_the_held_out_psnr(tmp_path, gpu_modules, capsys):
    """FieldFitter.fit on a 33 x 20 four-channel split, i_testset=2, four steps: the test PSNR printed last is
    evaluate_views' (use_full_nerf) on the final weights; a callable source has no held-out views."""
    from nerf_sampling_amd import nerf_utils, ops
    from nerf_sampling_amd.ray_batches import DeviceRayDataset
    from nerf_sampling_amd.synthetic import pose_spherical
    from nerf_sampling_amd.trainers import FieldFitter

    ops.set_compute_dtype("f32")
    Hf, Wf, focal = 33, 20, 28.0
    rng = np.random.default_rng(3320)
    images4 = rng.random((4, Hf, Wf, 4), dtype=np.float32)
    images4[..., 3] = np.where(rng.random((4, Hf, Wf)) < 0.3, np.float32(1.0), images4[..., 3])
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
    fitter.fit(split, 4, N_rand=64, basedir=str(tmp_path), expname="field", i_print=0, i_testset=2)
    printed = re.findall(r"\[FIT\] Iter: (\d+) test PSNR: (\S+)", capsys.readouterr().out)
    assert [int(i) for i, _ in printed] == [2, 4]
    for it in (2, 4):
        d = os.path.join(str(tmp_path), "field", f"testset_{it:06d}")
        assert os.listdir(d) == ["psnr.txt"]
        vals, avg = _parse(os.path.join(d, "psnr.txt"), 2)
        assert avg == float(dict((int(i), p) for i, p in printed)[it]) and np.isfinite(vals).all()
    # the same views through evaluate_views on the final weights
    for p in list(nets["coarse"].parameters()) + list(nets["fine"].parameters()):
        p.requires_grad_(False)
    K = np.array([[focal, 0, 0.5 * Wf], [0, focal, 0.5 * Hf], [0, 0, 1]])
    kw = _kwargs(dict(coarse=nets["coarse"], fine=nets["fine"], depth=base["depth"]), use_full_nerf=True, N_importance=8,
                 N_samples=8, lindisp=False)
    kw.update(N_samples=8, lindisp=False)
    ds = DeviceRayDataset(images4, poses, K, [0, 1], white_bkgd=True)
    psnrs, avg, frames = nerf_utils.evaluate_views(ds, [2, 3], poses[[2, 3]], (Hf, Wf, focal), K, kw, return_frames=True)
    print("fit printed", printed, "evaluate_views", psnrs.tolist(), avg)
    assert avg == float(printed[-1][1])
    gt = images4[[2, 3]]
    gt = gt[..., :3] * gt[..., 3:] + (np.float32(1.0) - gt[..., 3:])
    for f, g, p in zip(frames, gt, psnrs):
        d = (f.cpu().numpy().reshape(Hf, Wf, 3) - g).astype(np.float64)
        np.testing.assert_allclose(p, -10.0 * np.log10(np.sum(d * d) / d.size), rtol=1e-9, atol=0)
    with pytest.raises(ValueError, match="i_testset"):
        fitter.fit(lambda: None, 1, i_testset=2)


# ---- the CLI ---------------------------------------------------------------------------------------------------------
def _cli_root(root, m, n_test=9):
    """a reference-layout root with a random 'lego' of 32 x 32 files (tests/test_render_path.py's, restated); the yaml's
    testskip of 8 keeps test frames 0 and 8: two views"""
    from nerf_sampling_amd.synthetic import pose_spherical

    rng = np.random.default_rng(1)
    frames = [_rgba(rng, 32, 32) for _ in range(n_test)]
    poses = [pose_spherical(40.0 * k, -30.0, 4.0).cpu().numpy() for k in range(n_test)]     # (a CLI run leaves cuda the default)
    _write_dataset(os.path.join(root, "dataset", "lego"), {"train": frames[:1], "val": frames[:1], "test": frames},
                   {"train": poses[:1], "val": poses[:1], "test": poses})
    os.makedirs(os.path.join(root, "pretrained", "nerf", "lego"))
    os.makedirs(os.path.join(root, "pretrained", "depth_net", "lego", "files", "sampler_experiment"))
    both = list(m["coarse"].parameters()) + list(m["fine"].parameters())
    torch.save({"global_step": 200000, "network_fn_state_dict": m["coarse"].state_dict(),
                "network_fine_state_dict": m["fine"].state_dict(),
                "optimizer_state_dict": torch.optim.Adam(both).state_dict()},
               os.path.join(root, "pretrained", "nerf", "lego", "200000.tar"))
    torch.save({"global_step": 200000, "depth_network": m["depth"].state_dict(),
                "sampling_optimizer_state_dict": torch.optim.Adam(m["depth"].parameters()).state_dict()},
               os.path.join(root, "pretrained", "depth_net", "lego", "files", "sampler_experiment", "200000.tar"))
    return root


def test_render_cli_device_psnr(tmp_path, gpu_modules):
    """`render -d lego -rt --device-psnr`: psnr.txt agrees with the default run's within the gate, and no PNG is written"""
    from click.testing import CliRunner

    from nerf_sampling_amd.experiments.render import main

    exp = "lego_depth_net_render_n_samples_2_distance_0.01_sampling_mode_uniform"
    got = {}
    try:
        for flags in ((), ("--device-psnr",)):
            root = _cli_root(str(tmp_path / f"root{len(flags)}"), gpu_modules("lego_synth"))
            res = CliRunner().invoke(main, ["-d", "lego", "-rt", "--root", root, *flags], catch_exceptions=False)
            assert res.exit_code == 0, res.output
            final = float(re.search(r"Final psnr: (\S+)", res.output).group(1))
            d = os.path.join(root, "logs", "lego", exp, "renderonly_test_200000")
            got[flags] = (_parse(os.path.join(d, "psnr.txt"), 2), final, sorted(os.listdir(d)))
    finally:
        torch.set_default_device("cpu")   # the CLI switches the global default device like the reference does
    (h_vals, h_avg), h_final, h_files = got[()]
    (d_vals, d_avg), d_final, d_files = got[("--device-psnr",)]
    print("default", h_vals.tolist(), "device", d_vals.tolist())
    assert h_files == ["000.png", "001.png", "psnr.txt"] and d_files == ["psnr.txt"]
    assert np.isfinite(h_vals).all() and np.abs(h_vals - d_vals).max() <= GATE_DB
    assert abs(h_avg - d_avg) <= GATE_DB and abs(h_final - d_final) <= GATE_DB
