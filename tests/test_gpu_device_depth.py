"""The depth report of the device evaluation through every layer above ns_depth_sqerr: nerf_utils.evaluate_views(depth=True),
its cached field depths, Trainer(device_eval=True, device_depth=True) and render.py --device-depth -- on the 24 x 24 scene,
networks and dataset writers of tests/test_gpu_device_eval.py.

The two MSEs are checked against float64 numpy on the arrays the evaluation returns, within 1e-9 relative (the summation
bound, n 2^-52 with n = 24 * 24 * 8 elements, is 1e-12); the arrays themselves against what the chunked operators return for
the same view under compare_nerf -- nerf_utils.render_test, the renderer render_path's ``MSE:`` is computed from (its
depth_net_z_vals are the placed samples [R,N]), and nerf_utils.render, the training operator (its depth_net_z_vals are the
DepthNet's own depth [R,1]) -- bit for bit.  The PSNR and SSIM side must not notice the switch: same values, same files."""

import os
import re

import numpy as np
import pytest
import torch

import test_gpu_device_eval as E

pytestmark = pytest.mark.gpu

H, W, TEST_IDS = E.H, E.W, E.TEST_IDS
REL = 1e-9


def _parse_depth(path, n):
    """depth.txt -> (sample MSE per view, mean MSE per view, the two averages), the layout checked line by line"""
    lines = open(path).read().split("\n")
    assert len(lines) == n + 4 and lines[-1] == "" and lines[n] == f"Avg of {n} images:", lines
    sample, mean = [], []
    for i in range(n):
        m = re.fullmatch(rf"{i:03d}\.png, MSE: (\S+), mean MSE: (\S+)", lines[i])
        assert m, lines[i]
        sample.append(float(m.group(1)))
        mean.append(float(m.group(2)))
    assert lines[n + 1].startswith("MSE: ") and lines[n + 2].startswith("mean MSE: ")
    return np.array(sample), np.array(mean), float(lines[n + 1][len("MSE: "):]), float(lines[n + 2][len("mean MSE: "):])


def _count_hierarchical(monkeypatch):
    from nerf_sampling_amd import ops

    calls = []
    real = ops.render_rays_hierarchical

    def counted(*a, **k):
        calls.append(bool(k.get("max_sample", False)))
        return real(*a, **k)

    monkeypatch.setattr(ops, "render_rays_hierarchical", counted)
    return calls


def _mse64(a, b):
    d = (a.cpu().numpy().reshape(H * W, -1) - b.cpu().numpy().reshape(H * W, 1)).astype(np.float64)    # one fp32 subtraction
    return float(np.sum(d * d) / d.size)


@pytest.mark.parametrize("mode,n,dtype", [("uniform", 2, "f32"), ("uniform", 8, "f32"), ("depth_only", 1, "f32"),
                                          ("uniform", 4, "bf16")])
def test_evaluate_views_reports_the_depth_of_its_frames(tmp_path, gpu_modules, monkeypatch, mode, n, dtype):
    from nerf_sampling_amd import nerf_utils

    E._set_dtype(dtype)
    m = gpu_modules("tiny_synth")
    kw = E._kwargs(m, sampling_mode=mode, n_depth_samples=n)
    images, poses, focal, K, ds = E._scene()
    test_poses = torch.from_numpy(poses[TEST_IDS])
    calls = _count_hierarchical(monkeypatch)
    off_dir, on_dir = str(tmp_path / "off"), str(tmp_path / "on")
    off = nerf_utils.evaluate_views(ds, TEST_IDS, test_poses, (H, W, focal), K, kw, savedir=off_dir, ssim=True)
    assert len(off) == 4 and calls == []                                          # the switch off: no new launch, the old tuple
    on = nerf_utils.evaluate_views(ds, TEST_IDS, test_poses, (H, W, focal), K, kw, savedir=on_dir, ssim=True, depth=True,
                                   return_depths=True)
    assert len(on) == 9 and calls == [True] * 3
    psnrs, avg, ssims, avg_ssim, sample, avg_sample, mean, avg_mean, depths = on
    # the other scores: the same bits, the same files
    assert psnrs.tobytes() == off[0].tobytes() and avg == off[1] and ssims.tobytes() == off[2].tobytes() and avg_ssim == off[3]
    for name in ("psnr.txt", "ssim.txt"):
        assert open(os.path.join(on_dir, name), "rb").read() == open(os.path.join(off_dir, name), "rb").read()
    assert sorted(os.listdir(on_dir)) == ["depth.txt", "psnr.txt", "ssim.txt"] and sorted(os.listdir(off_dir)) == ["psnr.txt", "ssim.txt"]
    # the two numbers against float64 numpy on the returned arrays
    N = 1 if mode == "depth_only" else n
    assert len(depths) == 3
    for z, mu, max_z in depths:
        assert z.is_cuda and tuple(z.shape) == (H * W, N) and mu.numel() == H * W and tuple(max_z.shape) == (H * W, 1)
    want_sample = np.array([_mse64(z, max_z) for z, _mu, max_z in depths])
    want_mean = np.array([_mse64(mu, max_z) for _z, mu, max_z in depths])
    print(f"{mode} n={n} {dtype}: sample MSE {sample.tolist()} float64 {want_sample.tolist()}; mean MSE {mean.tolist()} "
          f"float64 {want_mean.tolist()}")
    assert sample.dtype == np.float64 and mean.dtype == np.float64 and sample.shape == mean.shape == (3,)
    assert np.isfinite(sample).all() and np.isfinite(mean).all() and (sample > 0).all()
    assert (np.abs(sample - want_sample) <= REL * want_sample).all() and (np.abs(mean - want_mean) <= REL * want_mean).all()
    assert avg_sample == float(np.mean(sample)) and avg_mean == float(np.mean(mean))
    if mode == "depth_only":
        assert sample.tobytes() == mean.tobytes()                                  # z is the mean
        assert all(torch.equal(z.reshape(-1), mu.reshape(-1)) for z, mu, _ in depths)
    # the file
    f_sample, f_mean, f_avg_sample, f_avg_mean = _parse_depth(os.path.join(on_dir, "depth.txt"), 3)
    assert np.array_equal(f_sample, sample) and np.array_equal(f_mean, mean) and (f_avg_sample, f_avg_mean) == (avg_sample, avg_mean)
    assert open(os.path.join(on_dir, "depth.txt")).read() == nerf_utils.format_depth_txt(sample, avg_sample, mean, avg_mean)
    # without return_depths the tuple ends with the averages; with frames they come before the depths
    short = nerf_utils.evaluate_views(ds, TEST_IDS[:1], test_poses[:1], (H, W, focal), K, kw, depth=True)
    assert len(short) == 6 and short[2][0] == sample[0] and short[4][0] == mean[0]
    both = nerf_utils.evaluate_views(ds, TEST_IDS[:1], test_poses[:1], (H, W, focal), K, kw, depth=True, return_frames=True,
                                     return_depths=True)
    assert len(both) == 8 and tuple(both[6][0].shape) == (H * W, 3) and len(both[7][0]) == 3
    # the arrays are the chunked operators' under compare_nerf, bit for bit
    ref_kw = E._kwargs(m, sampling_mode=mode, n_depth_samples=n, compare_nerf=True)
    with torch.no_grad():
        for (z, mu, max_z), c2w in zip(depths, test_poses):
            _rgb, _disp, ex = nerf_utils.render_test(H, W, K, chunk=200, c2w=c2w[:3, :4], **ref_kw)
            assert torch.equal(ex["depth_net_z_vals"].cpu().reshape(H * W, N), z.cpu())
            assert torch.equal(ex["max_z_vals"].cpu().reshape(H * W, 1), max_z.cpu())
            _rgb, _disp, ex = nerf_utils.render(H, W, K, chunk=200, c2w=c2w[:3, :4], **ref_kw)
            assert torch.equal(ex["depth_net_z_vals"].cpu().reshape(H * W), mu.cpu().reshape(H * W))
            assert torch.equal(ex["max_z_vals"].cpu().reshape(H * W, 1), max_z.cpu())
    nerf_utils.drain_host_copies()


def test_cached_field_depths_launch_no_hierarchical_render(gpu_modules, monkeypatch):
    from nerf_sampling_amd import nerf_utils

    E._set_dtype("f32")
    kw = E._kwargs(gpu_modules("tiny_synth"), sampling_mode="uniform", n_depth_samples=4)
    images, poses, focal, K, ds = E._scene()
    test_poses = torch.from_numpy(poses[TEST_IDS])
    calls = _count_hierarchical(monkeypatch)
    first = nerf_utils.evaluate_views(ds, TEST_IDS, test_poses, (H, W, focal), K, kw, depth=True, return_depths=True)
    assert len(calls) == 3
    field = [max_z for _z, _mu, max_z in first[-1]]
    kept = [t.clone() for t in field]
    again = nerf_utils.evaluate_views(ds, TEST_IDS, test_poses, (H, W, focal), K, kw, depth=True, field_depths=field,
                                      return_depths=True)
    assert len(calls) == 3                                                       # not one more
    for a, b in zip(first[:-1], again[:-1]):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert all(d[2] is f for d, f in zip(again[-1], field)) and all(torch.equal(f, k) for f, k in zip(field, kept))
    fresh = nerf_utils.evaluate_views(ds, TEST_IDS, test_poses, (H, W, focal), K, kw, depth=True)
    assert len(calls) == 6 and all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(first[:-1], fresh))
    with pytest.raises(ValueError, match="field depths"):
        nerf_utils.evaluate_views(ds, TEST_IDS, test_poses, (H, W, focal), K, kw, depth=True, field_depths=field[:2])


def test_refusals(gpu_modules):
    """no render_path fallback for the depth report: what either one-call renderer does not take is an error that says so"""
    from nerf_sampling_amd import nerf_utils

    E._set_dtype("f32")
    m = gpu_modules("tiny_synth")
    images, poses, focal, K, ds = E._scene()
    args = (ds, TEST_IDS[:1], torch.from_numpy(poses[TEST_IDS[:1]]), (H, W, focal), K)
    kw = E._kwargs(m, sampling_mode="uniform", n_depth_samples=4)
    std = kw["network_query_fn"]
    kw["network_query_fn"] = lambda i, v, f: std(i, v, f)                        # not the standard query function
    with pytest.raises(ValueError, match="one-call DepthNet renderer"):
        nerf_utils.evaluate_views(*args, kw, depth=True)
    with pytest.raises(ValueError, match="hierarchical renderer"):                # no fine pass: no max-weight fine sample
        nerf_utils.evaluate_views(*args, E._kwargs(m, sampling_mode="uniform", n_depth_samples=4, N_importance=0), depth=True)
    with pytest.raises(ValueError, match="use_full_nerf"):
        nerf_utils.evaluate_views(*args, E._kwargs(m, use_full_nerf=True), depth=True)
    assert len(nerf_utils.evaluate_views(*args, E._kwargs(m, use_full_nerf=True))) == 2     # and stays available without


def test_train_renders_the_field_once_and_leaves_the_step_alone(tmp_path, gpu_modules, capsys, monkeypatch):
    """device_eval with and without device_depth, train_depth_net_only, i_testset=2, seven iterations on the graphed step:
    testset_000002 / _000004 / _000006 hold psnr.txt and depth.txt, the line is printed, the field's depth maps are rendered at
    the first evaluation alone (three views, three hierarchical calls in the whole run), and the final DepthNet is the same bit
    for bit."""
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
    calls = _count_hierarchical(monkeypatch)
    final, psnr_txt, means = {}, {}, []
    for on in (False, True):
        logs = str(tmp_path / f"logs_{int(on)}")
        kw = dict(dataset_type="blender", basedir=logs, expname="exp", no_batching=True, datadir=data, half_res=False,
                  white_bkgd=True, testskip=1, device="cuda", N_rand=128, N_importance=128, N_samples=64, use_viewdirs=True,
                  input_dims_embed=3, netdepth=4, netwidth=128, netdepth_fine=4, netwidth_fine=128, n_layers=3,
                  layer_width=128, sphere_radius=2.0, ft_path=nerf_ckpt, depth_net_lr=1e-3, train_depth_net_only=True,
                  i_weights=7, i_print=2, perturb=1.0, i_testset=2, n_depth_samples=8, sampling_mode="uniform", distance=0.1,
                  hip_graph=True, device_eval=True, device_depth=on)
        np.random.seed(0); torch.manual_seed(0)
        tr = DepthNetTrainer(**kw)
        before = len(calls)
        assert tr.train(N_iters=8) is not None                                   # iterations 1..7
        out = capsys.readouterr().out
        exp = os.path.join(logs, "exp")
        assert sorted(d for d in os.listdir(exp) if d.startswith("testset_")) == ["testset_000002", "testset_000004", "testset_000006"]
        if on:
            assert calls[before:] == [True] * 3                                  # three views, once: not at every evaluation
            assert len(tr._field_depths) == 3
        else:
            assert len(calls) == before and "depth MSE" not in out and tr._field_depths is None
        for it in (2, 4, 6):
            d = os.path.join(exp, f"testset_{it:06d}")
            assert sorted(os.listdir(d)) == (["depth.txt", "psnr.txt"] if on else ["psnr.txt"])
            psnr_txt[on, it] = open(os.path.join(d, "psnr.txt"), "rb").read()
            _, avg = E._parse(os.path.join(d, "psnr.txt"), 3)
            assert f"[TRAIN] Iter: {it} test PSNR: {avg}" in out
            if on:
                sample, mean, avg_sample, avg_mean = _parse_depth(os.path.join(d, "depth.txt"), 3)
                assert np.isfinite(sample).all() and np.isfinite(mean).all()
                assert avg_sample == float(np.mean(sample)) and avg_mean == float(np.mean(mean))
                assert f"[TRAIN] Iter: {it} test depth MSE: {avg_sample} mean MSE: {avg_mean}" in out
                means.append(avg_mean)
        final[on] = torch.load(os.path.join(exp, "000007.tar"), weights_only=True)["depth_network"]
    print("held-out mean MSE at iterations 2, 4, 6:", means)
    assert len(set(means)) == 3                                                  # the DepthNet moves, so its held-out loss does
    assert all(psnr_txt[True, it] == psnr_txt[False, it] for it in (2, 4, 6))
    assert set(final[True]) == set(final[False])
    assert all(torch.equal(final[True][k], final[False][k]) for k in final[True])


@pytest.mark.parametrize("ssim", [False, True])
@pytest.mark.parametrize("frozen", [True, False])
def test_evaluate_testset_keeps_the_field_depths_only_while_the_field_is_frozen(tmp_path, gpu_modules, monkeypatch, ssim, frozen):
    """Trainer.evaluate_testset twice: (PSNR[, SSIM], (sample MSE, mean MSE)), the same bits both times; the hierarchical frames
    of the second call are rendered again unless train_depth_net_only says that the field cannot have moved"""
    E._set_dtype("f32")
    images, poses, focal, K, ds = E._scene()
    kw = E._kwargs(gpu_modules("tiny_synth"), sampling_mode="uniform", n_depth_samples=4, device_eval=True, device_ssim=ssim,
                   device_depth=True, train_depth_net_only=frozen, basedir=str(tmp_path))
    tr = kw["trainer"]
    tr.K, tr._ray_dataset = K, ds
    calls = _count_hierarchical(monkeypatch)
    got = [tr.evaluate_testset(i, TEST_IDS, poses[TEST_IDS], (H, W, focal), kw) for i in (2, 4)]
    assert len(calls) == (3 if frozen else 6) and (tr._field_depths is not None) == frozen
    assert got[0] == got[1] and len(got[0]) == (3 if ssim else 2) and len(got[0][-1]) == 2
    for i in (2, 4):
        d = os.path.join(str(tmp_path), "eval", f"testset_{i:06d}")
        assert sorted(os.listdir(d)) == ["depth.txt", "psnr.txt"] + (["ssim.txt"] if ssim else [])
        _, _, avg_sample, avg_mean = _parse_depth(os.path.join(d, "depth.txt"), 3)
        assert got[0][-1] == (avg_sample, avg_mean) and got[0][0] == E._parse(os.path.join(d, "psnr.txt"), 3)[1]


def test_render_cli_device_depth(tmp_path, gpu_modules):
    """`render -d lego -rt --device-depth` on three test views: the flag implies the device path (no PNG), psnr.txt is
    --device-psnr's byte for byte, and depth.txt stands beside it"""
    from click.testing import CliRunner

    from nerf_sampling_amd.experiments.render import main

    exp = "lego_depth_net_render_n_samples_2_distance_0.01_sampling_mode_uniform"
    got = {}
    try:
        for flag in ("--device-psnr", "--device-depth"):
            root = E._cli_root(str(tmp_path / flag.strip("-")), gpu_modules("lego_synth"), n_test=17)     # frames 0, 8, 16
            res = CliRunner().invoke(main, ["-d", "lego", "-rt", "--root", root, flag], catch_exceptions=False)
            assert res.exit_code == 0, res.output
            d = os.path.join(root, "logs", "lego", exp, "renderonly_test_200000")
            got[flag] = (d, sorted(os.listdir(d)), float(re.search(r"Final psnr: (\S+)", res.output).group(1)))
    finally:
        torch.set_default_device("cpu")   # the CLI switches the global default device like the reference does
    assert got["--device-psnr"][1] == ["psnr.txt"] and got["--device-depth"][1] == ["depth.txt", "psnr.txt"]
    assert got["--device-psnr"][2] == got["--device-depth"][2]
    assert (open(os.path.join(got["--device-psnr"][0], "psnr.txt"), "rb").read()
            == open(os.path.join(got["--device-depth"][0], "psnr.txt"), "rb").read())
    sample, mean, avg_sample, avg_mean = _parse_depth(os.path.join(got["--device-depth"][0], "depth.txt"), 3)
    print("sample MSE per view", sample.tolist(), "mean MSE per view", mean.tolist())
    assert np.isfinite(sample).all() and np.isfinite(mean).all() and (sample > 0).all()
    assert avg_sample == float(np.mean(sample)) and avg_mean == float(np.mean(mean))
