"""The mesh rasteriser through every layer above ns_mesh_raster: nerf_utils.render_mesh_views, score_mesh_views and
Trainer(device_mesh=True, device_mesh_eval=True), on the tiny_synth networks at 24 lattice points per axis, the threshold of
tests/test_gpu_device_mesh.py and the 16 x 20 frames of tests/test_gpu_device_cloud.py."""

import os
import re

import numpy as np
import pytest
import torch

import mesh_raster_reference as RR
import test_gpu_device_cloud as CL

pytestmark = pytest.mark.gpu

G, BOUND, THRESHOLD = 24, 1.5, 14.0
KW = dict(bound=BOUND, resolution=G, threshold=THRESHOLD)
H, W = CL.H, CL.W
NEAR = 2.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH_SHARE = int(re.search(r"#define NS_DEPTH_SQERR_SHARE (\d+)",
                            open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()).group(1))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _block_sum(v):
    """ns::block_sum of 256 doubles in its own order: per wave the xor tree with offsets 32 .. 1 (lane 0's value), then the four
    waves added in order"""
    waves = []
    for w in range(4):
        lane = np.array(v[64 * w:64 * w + 64], dtype=np.float64)
        off = 32
        while off:
            lane = lane + lane[np.arange(64) ^ off]
            off >>= 1
        waves.append(lane[0])
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]


def depth_sum_in_kernel_order(z, ref):
    """sum (double)(fl32(z - ref))^2 over [R] as ns_depth_sqerr adds it with one sample per ray: workgroup g owns DEPTH_SHARE
    elements, thread t adds g * SHARE + j * 256 + t in the order of j, ns::block_sum per workgroup, then one workgroup adds the
    partials (thread t: partials t, t + 256, .. in order) the same way"""
    d = (np.asarray(z, dtype=np.float32) - np.asarray(ref, dtype=np.float32)).astype(np.float64)
    sq = d * d
    groups = -(-sq.size // DEPTH_SHARE)
    sq = np.concatenate([sq, np.zeros(groups * DEPTH_SHARE - sq.size)]).reshape(groups, DEPTH_SHARE // 256, 256)
    partial = []
    for g in range(groups):
        acc = np.zeros(256)
        for j in range(sq.shape[1]):
            acc = acc + sq[g, j]
        partial.append(_block_sum(acc))
    acc = np.zeros(256)
    for i, p in enumerate(partial):
        acc[i % 256] = acc[i % 256] + p
    return _block_sum(acc)


@pytest.fixture(autouse=True)
def _f32_field():
    from nerf_sampling_amd import ops

    ops.set_compute_dtype("f32")
    ops.set_psnr_guard(False)


@pytest.fixture(scope="module")
def mesh(gpu_modules):
    """scene_mesh_shaded on the fine network, its largest component: computed once, shared, never modified"""
    from nerf_sampling_amd import nerf_utils, ops

    ops.set_compute_dtype("f32")
    return nerf_utils.scene_mesh_shaded(gpu_modules("tiny_synth")["fine"], keep_largest=1, normals=False, **KW)


@pytest.fixture(scope="module")
def dataset():
    from nerf_sampling_amd import ops

    focal, K, poses = CL._camera()
    images = np.random.default_rng(7).random((2, H, W, 3), dtype=np.float32)
    return ops.ray_dataset(images, poses.numpy(), K, [0]), images, focal, K, poses


def _restated(mesh, pose, K, background, cull=0):
    return RR.rasterize(mesh["vertices"].cpu().numpy(), mesh["faces"].cpu().numpy(), pose.numpy()[:3, :4], float(K[0][0]),
                        float(K[1][1]), float(K[0][2]), float(K[1][2]), H, W, NEAR, attr=mesh["rgb"].cpu().numpy(),
                        background=background, cull=cull)


def test_render_mesh_views_and_its_pngs(mesh, dataset, tmp_path):
    """every view is the restatement's bits; mesh_rgb/NNN.png decodes to to8b of the frame and mesh_depth/NNN.png to to8b of
    the depth divided by the maximum over all views"""
    from PIL import Image

    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.run_nerf_helpers import to8b

    _, _, focal, K, poses = dataset
    d = str(tmp_path / "views")
    views = nerf_utils.render_mesh_views(mesh, poses, (H, W, focal), K, NEAR, savedir=d, background=1.0)
    assert sorted(os.listdir(d)) == ["mesh_depth", "mesh_rgb"]
    deepest = max(float(v.max()) for v in views["depth"])
    assert deepest > NEAR
    for k, pose in enumerate(poses):
        want = _restated(mesh, pose, K, 1.0)
        print(f"view {k}: {mesh['faces'].shape[0]} faces, counts {want['counts'].tolist()}")
        assert want["counts"][3] > 20 and want["counts"][2] == 0
        assert (views["n_clipped"][k], views["n_degenerate"][k], views["n_invalid"][k], views["n_covered"][k]) == tuple(
            want["counts"].tolist())
        assert (_bits(views["depth"][k].cpu().numpy()) == _bits(want["depth"])).all()
        assert (views["tri"][k].cpu().numpy() == want["tri"]).all()
        assert (_bits(views["rgb"][k].cpu().numpy()) == _bits(want["rgb"])).all()
        rgb8 = np.array(Image.open(os.path.join(d, "mesh_rgb", f"{k:03d}.png")))
        assert rgb8.shape == (H, W, 3) and (rgb8 == to8b(want["rgb"].reshape(H, W, 3))).all()
        depth8 = np.array(Image.open(os.path.join(d, "mesh_depth", f"{k:03d}.png")))
        assert depth8.shape == (H, W) and (depth8 == nerf_utils.disp_to8b_host(want["depth"], deepest).reshape(H, W)).all()
    # without a directory nothing is written and the frames are the same; without colours there is no colour frame
    plain = nerf_utils.render_mesh_views(mesh, poses, (H, W, focal), K, NEAR, background=1.0)
    assert all(torch.equal(a, b) for name in ("rgb", "depth", "tri") for a, b in zip(plain[name], views[name]))
    bare = nerf_utils.render_mesh_views(dict(mesh, rgb=None), poses[:1], (H, W, focal), K, NEAR, cull=1)
    assert bare["rgb"] == [None] and bare["n_covered"][0] > 20


def test_score_mesh_views_against_numpy(mesh, dataset, gpu_modules, tmp_path):
    from nerf_sampling_amd import nerf_utils

    ds, images, focal, K, poses = dataset
    kw = CL._kwargs(gpu_modules, "n16")
    d = str(tmp_path / "scores")
    got = nerf_utils.score_mesh_views(ds, [0, 1], poses, (H, W, focal), K, mesh, NEAR, render_kwargs=kw, savedir=d,
                                      background=1.0)
    assert sorted(os.listdir(d)) == ["mesh_depth.txt", "mesh_iou.txt", "mesh_psnr.txt"]
    views = nerf_utils.render_mesh_views(mesh, poses, (H, W, focal), K, NEAR, background=1.0)
    for k in range(2):
        frame = views["rgb"][k].cpu().numpy().astype(np.float32)
        depth, tri = views["depth"][k].cpu().numpy(), views["tri"][k].cpu().numpy()
        field_depth, field_acc = got["field_depths"][k].cpu().numpy(), got["field_accs"][k].cpu().numpy()
        assert field_depth.shape == (H * W,) and field_acc.shape == (H * W,) and torch.equal(got["views"]["depth"][k], views["depth"][k])
        diff = (frame.reshape(H, W, 3) - images[k]).astype(np.float64)
        psnr = -10.0 * np.log10(np.mean(diff * diff))
        mse = depth_sum_in_kernel_order(depth, field_depth) / (H * W)
        solid, seen = field_acc > 0.5, tri >= 0
        iou = (solid & seen).sum() / max((solid | seen).sum(), 1)
        print(f"view {k}: mesh PSNR {got['mesh_psnr'][k]:.4f} dB (numpy {psnr:.4f}), depth MSE {got['depth_mse'][k]:.6e} "
              f"(numpy {mse:.6e}), IoU {got['silhouette_iou'][k]:.4f} (numpy {iou:.4f}), {seen.sum()} mesh and {solid.sum()} "
              f"field pixels")
        assert abs(got["mesh_psnr"][k] - psnr) < 1e-4
        assert got["depth_mse"][k] == mse
        assert got["silhouette_iou"][k] == iou and 0 < seen.sum() < H * W
    for name, label, key in (("mesh_psnr.txt", "PSNR", "mesh_psnr"), ("mesh_depth.txt", "MSE", "depth_mse"),
                             ("mesh_iou.txt", "IoU", "silhouette_iou")):
        assert open(os.path.join(d, name)).read() == nerf_utils.format_mesh_txt(label, got[key], float(np.mean(got[key])))
    # the field's maps handed back in: no field render, the same numbers
    again = nerf_utils.score_mesh_views(ds, [0, 1], poses, (H, W, focal), K, mesh, NEAR, field_depths=got["field_depths"],
                                        field_accs=got["field_accs"], background=1.0)
    for key in ("mesh_psnr", "depth_mse", "silhouette_iou"):
        assert (again[key] == got[key]).all()
    # the maps are the one-call renderer's extras for the same camera
    out = nerf_utils._depthnet_one_call(kw["depth_network"], kw["network_fine"], kw["trainer"],
                                        camera=(H, W, K, poses[0][:3, :4], 0, H), extras=("depth", "acc"),
                                        device=torch.device("cuda"))
    assert torch.equal(out["depth"], got["field_depths"][0]) and torch.equal(out["acc"], got["field_accs"][0])


def test_trainer_switch_adds_three_files_and_changes_nothing_else(tmp_path, gpu_modules, dataset):
    """Trainer(device_mesh=True, device_mesh_eval=True) in a render-only run: mesh_psnr.txt, mesh_depth.txt and mesh_iou.txt
    appear; every other file keeps its bytes; off, the directory is the one the run always wrote"""
    from nerf_sampling_amd import nerf_utils

    _, images, focal, K, poses = dataset
    files = {}
    for on in (False, True):
        kw = CL._kwargs(gpu_modules, "n16", basedir=str(tmp_path / f"r{int(on)}"), device_mesh=True, mesh_resolution=G,
                        mesh_threshold=THRESHOLD, mesh_bound=BOUND, mesh_keep_largest=1, device_mesh_eval=on)
        tr = kw["trainer"]
        tr.K, tr.global_step = K, 7
        tr.render(True, False, images, [0, 1], poses, (H, W, focal), kw)
        d = os.path.join(tr.basedir, tr.expname, "renderonly_test_000007")
        files[on] = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
    assert sorted(files[False]) == ["000.png", "001.png", "psnr.txt", "scene_mesh.ply"]
    assert sorted(files[True]) == sorted(list(files[False]) + ["mesh_depth.txt", "mesh_iou.txt", "mesh_psnr.txt"])
    assert all(files[True][f] == files[False][f] for f in files[False])
    mesh = nerf_utils.scene_mesh_shaded(gpu_modules("tiny_synth")["fine"], keep_largest=1, normals=False, **KW)
    ds = dataset[0]
    want = nerf_utils.score_mesh_views(ds, [0, 1], poses, (H, W, focal), K, mesh, NEAR,
                                       render_kwargs=CL._kwargs(gpu_modules, "n16"), background=1.0)
    assert files[True]["mesh_psnr.txt"].decode() == nerf_utils.format_mesh_txt("PSNR", want["mesh_psnr"], want["avg_mesh_psnr"])
    assert files[True]["mesh_iou.txt"].decode() == nerf_utils.format_mesh_txt("IoU", want["silhouette_iou"],
                                                                              want["avg_silhouette_iou"])
    assert files[True]["mesh_depth.txt"].decode() == nerf_utils.format_mesh_txt("MSE", want["depth_mse"], want["avg_depth_mse"])
    nerf_utils.drain_host_copies()
