"""The mesh simplification through every layer above ns_mesh_simplify: nerf_utils.scene_mesh_simplified, nerf_utils.mesh_simplify,
score_mesh_views on the result and Trainer(device_mesh=True, mesh_simplify=K), on the tiny_synth networks at 32 lattice points per
axis, the threshold of tests/test_gpu_device_mesh.py and the 16 x 20 frames of tests/test_gpu_device_cloud.py."""

import os

import numpy as np
import pytest
import torch

import mesh_simplify_reference as SR
import test_gpu_device_cloud as CL
from test_gpu_device_mesh_normals import _bits, _read_ply

pytestmark = pytest.mark.gpu

G, BOUND, THRESHOLD = 32, 1.5, 14.0
KW = dict(bound=BOUND, resolution=G, threshold=THRESHOLD)
H, W = CL.H, CL.W
NEAR = 2.0


@pytest.fixture(autouse=True)
def _f32_field():
    from nerf_sampling_amd import ops

    ops.set_compute_dtype("f32")
    ops.set_psnr_guard(False)


@pytest.fixture(scope="module")
def shaded(gpu_modules, tmp_path_factory):
    """scene_mesh_shaded's largest component with normals, and its PLY: computed once, shared, never modified"""
    from nerf_sampling_amd import nerf_utils, ops

    ops.set_compute_dtype("f32")
    d = str(tmp_path_factory.mktemp("shaded"))
    mesh = nerf_utils.scene_mesh_shaded(gpu_modules("tiny_synth")["fine"], keep_largest=1, savedir=d, **KW)
    return mesh, open(os.path.join(d, "scene_mesh.ply"), "rb").read()


def test_off_is_scene_mesh_shaded_to_the_byte(gpu_modules, shaded, tmp_path):
    from nerf_sampling_amd import nerf_utils

    base, ply = shaded
    d = str(tmp_path / "off")
    off = nerf_utils.scene_mesh_simplified(gpu_modules("tiny_synth")["fine"], keep_largest=1, savedir=d, simplify=0, **KW)
    assert sorted(off) == sorted(base)
    for k in base:
        assert torch.equal(off[k], base[k]) if isinstance(base[k], torch.Tensor) else off[k] == base[k], k
    assert open(os.path.join(d, "scene_mesh.ply"), "rb").read() == ply


def test_simplified_scene_mesh(gpu_modules, shaded, tmp_path):
    from nerf_sampling_amd import nerf_utils, ops
    from nerf_sampling_amd.run_nerf_helpers import to8b

    base, ply = shaded
    d = str(tmp_path / "two")
    got = nerf_utils.scene_mesh_simplified(gpu_modules("tiny_synth")["fine"], keep_largest=1, savedir=d, simplify=2, **KW)
    assert sorted(got) == sorted(list(base) + ["n_input_vertices", "n_input_faces", "simplify_index"] + list(nerf_utils.SIMPLIFY_COUNTERS))
    V0, F0, V1, F1 = base["vertices"].shape[0], base["faces"].shape[0], got["vertices"].shape[0], got["faces"].shape[0]
    print(f"{F0} faces on {V0} vertices -> {F1} on {V1}; " + ", ".join(f"{k} {got[k]}" for k in nerf_utils.SIMPLIFY_COUNTERS))
    assert (got["n_input_vertices"], got["n_input_faces"]) == (V0, F0) and got["n_triangles"] == base["n_triangles"]
    assert 0 < F1 < F0 / 2 and 0 < V1 == got["n_clusters"] < V0 and got["n_invalid"] == got["n_nonfinite"] == got["n_nonfinite_faces"] == 0
    assert got["n_collapsed"] + got["n_duplicate"] + F1 == F0
    # vertices, normals and colours are rows of the unsimplified result, matched through the index
    index = got["simplify_index"]
    kept = torch.nonzero(index >= 0)[:, 0]
    assert index.dtype == torch.int64 and tuple(index.shape) == (V0,) and torch.equal(index[kept], torch.arange(V1, device="cuda"))
    assert torch.equal(got["vertices"].view(torch.int32), base["vertices"][kept].view(torch.int32))
    assert torch.equal(got["normals"].view(torch.int32), base["normals"][kept].view(torch.int32))
    assert torch.equal(got["rgb"], base["rgb"][kept])                          # field rows are independent
    assert int(got["faces"].min()) >= 0 and int(got["faces"].max()) < V1
    # the numpy restatement on the unsimplified mesh, and nerf_utils.mesh_simplify on its dict
    lo, cell, dims = nerf_utils.simplify_lattice(base["lo"], base["h"], (G, G, G), 2)
    assert dims == [16, 16, 16]
    want = SR.simplify(base["vertices"].cpu().numpy(), base["faces"].cpu().numpy(), lo, cell, dims)
    assert np.array_equal(got["faces"].cpu().numpy(), want["faces"]) and np.array_equal(index.cpu().numpy(), want["index"])
    assert all(got[k] == want[k] for k in nerf_utils.SIMPLIFY_COUNTERS)
    direct = nerf_utils.mesh_simplify(base, lo, cell, dims)
    assert all(torch.equal(direct[k], got[k]) for k in ("vertices", "faces", "normals", "rgb"))
    assert torch.equal(direct["index"], index) and torch.equal(direct["rep"].cpu(), torch.from_numpy(want["rep"]))
    assert (direct["n_input_vertices"], direct["n_input_faces"]) == (V0, F0) and direct["n_triangles"] == base["n_triangles"]
    # the PLY parses back to the same arrays, and is not the unsimplified one
    vertex, idx = _read_ply(os.path.join(d, "scene_mesh.ply"))
    assert (_bits(vertex["xyz"]) == _bits(got["vertices"].cpu().numpy())).all() and (idx == got["faces"].cpu().numpy()).all()
    assert (_bits(vertex["n"]) == _bits(got["normals"].cpu().numpy())).all() and (vertex["rgb"] == to8b(got["rgb"].cpu().numpy())).all()
    assert len(open(os.path.join(d, "scene_mesh.ply"), "rb").read()) < len(ply) / 2
    # score_mesh_views runs on the result: finite scores, no threshold asserted
    focal, K, poses = CL._camera()
    images = np.random.default_rng(7).random((2, H, W, 3), dtype=np.float32)
    ds = ops.ray_dataset(images, poses.numpy(), K, [0])
    scored = nerf_utils.score_mesh_views(ds, [0, 1], poses, (H, W, focal), K, got, NEAR, render_kwargs=CL._kwargs(gpu_modules, "n16"),
                                         background=1.0)
    for key in ("mesh_psnr", "depth_mse", "silhouette_iou"):
        print(f"{key}: {[float(v) for v in scored[key]]}")
        assert len(scored[key]) == 2 and np.isfinite(np.asarray(scored[key], dtype=np.float64)).all()
    assert all(n > 0 for n in scored["views"]["n_covered"]) and all(n == 0 for n in scored["views"]["n_invalid"])


def test_trainer_writes_the_simplified_mesh(tmp_path, gpu_modules):
    """Trainer(device_mesh=True, mesh_simplify=2) in a render-only run: scene_mesh.ply is scene_mesh_simplified(simplify=2)'s; the
    frames and psnr.txt are those of the run without the switch, byte for byte, and so is the switch at 0"""
    from nerf_sampling_amd import nerf_utils

    focal, K, poses = CL._camera()
    images = np.random.default_rng(7).random((2, H, W, 3), dtype=np.float32)
    files = {}
    for name, over in (("never", {}), ("off", dict(mesh_simplify=0)), ("on", dict(mesh_simplify=2))):
        kw = CL._kwargs(gpu_modules, "n16", basedir=str(tmp_path / name), device_mesh=True, mesh_resolution=G,
                        mesh_threshold=THRESHOLD, mesh_bound=BOUND, mesh_keep_largest=1, mesh_normals=True, **over)
        tr = kw["trainer"]
        tr.K, tr.global_step = K, 7
        tr.render(True, False, images, [0, 1], poses, (H, W, focal), kw)
        d = os.path.join(tr.basedir, tr.expname, "renderonly_test_000007")
        files[name] = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
        files[name + " dir"] = d
    assert sorted(files["never"]) == sorted(files["off"]) == sorted(files["on"]) == ["000.png", "001.png", "psnr.txt", "scene_mesh.ply"]
    assert files["off"] == files["never"]
    assert all(files["on"][f] == files["never"][f] for f in ("000.png", "001.png", "psnr.txt"))
    direct = nerf_utils.scene_mesh_simplified(gpu_modules("tiny_synth")["fine"], keep_largest=1, simplify=2, **KW)
    vertex, idx = _read_ply(os.path.join(files["on dir"], "scene_mesh.ply"))
    assert (_bits(vertex["xyz"]) == _bits(direct["vertices"].cpu().numpy())).all() and (idx == direct["faces"].cpu().numpy()).all()
    assert (_bits(vertex["n"]) == _bits(direct["normals"].cpu().numpy())).all()
    nerf_utils.drain_host_copies()
