"""The mesh normals through every layer above ns_mesh_normals: nerf_utils.scene_mesh_shaded, its scene_mesh.ply and
Trainer(device_mesh=True, mesh_normals=True), on the tiny_synth networks at 24 lattice points per axis and the threshold of
tests/test_gpu_device_mesh.py (the upper quartile of the fine network's density on that lattice)."""

import os

import numpy as np
import pytest
import torch

import mesh_normals_reference as NR
import mesh_reference as MR
import test_gpu_device_cloud as CL

pytestmark = pytest.mark.gpu

G, BOUND, THRESHOLD = 24, 1.5, 14.0
KW = dict(bound=BOUND, resolution=G, threshold=THRESHOLD)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _read_ply(path):
    """-> (vertex records with xyz[, n][, rgb], face indices) of a scene_mesh.ply, every byte accounted for"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and "property list uchar int vertex_indices" in lines
    V = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    F = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    props = [ln.split()[-1] for ln in lines if ln.startswith("property") and "list" not in ln]
    fields = [("xyz", "<f4", (3,))]
    if "nx" in props:
        assert props[:6] == ["x", "y", "z", "nx", "ny", "nz"]                             # directly after z, before the colours
        fields.append(("n", "<f4", (3,)))
    if "red" in props:
        assert props[-3:] == ["red", "green", "blue"]
        fields.append(("rgb", "u1", (3,)))
    assert len(props) == sum(f[2][0] for f in fields)
    vertex = np.frombuffer(body, dtype=fields, count=V)
    face = np.frombuffer(body, dtype=[("c", "u1"), ("idx", "<i4", (3,))], count=F, offset=vertex.nbytes)
    assert len(body) == vertex.nbytes + face.nbytes and (face["c"] == 3).all()
    return vertex, face["idx"]


@pytest.fixture(autouse=True)
def _f32_field():
    """every test here compares against the shared mesh: one compute dtype for all of them"""
    from nerf_sampling_amd import ops

    ops.set_compute_dtype("f32")


@pytest.fixture(scope="module")
def shaded(gpu_modules, tmp_path_factory):
    """scene_mesh_shaded on the fine network, with its grid and its file: computed once, shared, never modified"""
    from nerf_sampling_amd import nerf_utils, ops

    ops.set_compute_dtype("f32")
    d = str(tmp_path_factory.mktemp("shaded"))
    got = nerf_utils.scene_mesh_shaded(gpu_modules("tiny_synth")["fine"], savedir=d, return_grid=True, **KW)
    return got, os.path.join(d, "scene_mesh.ply")


def test_normals_are_the_restatement_on_its_own_grid_and_keys(shaded, gpu_modules):
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.run_nerf_helpers import to8b

    got, ply = shaded
    grid = got["grid"].cpu().numpy()
    tri, keys, _ = MR.march(grid, THRESHOLD, got["lo"], got["h"])
    unique = np.unique(keys)                                                              # the welded vertices' order
    want, n_degenerate, n_invalid, _ = NR.normals(grid, THRESHOLD, got["h"], unique)
    normals = got["normals"]
    print(f"{unique.size} vertices, {n_degenerate} degenerate normals")
    assert unique.size > 500 and n_invalid == 0
    assert normals.is_cuda and normals.dtype == torch.float32 and tuple(normals.shape) == (unique.size, 3)
    assert got["n_degenerate_normals"] == n_degenerate
    assert (_bits(normals.cpu().numpy()) == _bits(want)).all()
    # everything else is scene_mesh_filtered's: the dict gains two keys, the tensors keep their bits
    plain = nerf_utils.scene_mesh_filtered(gpu_modules("tiny_synth")["fine"], return_grid=True, **KW)
    assert sorted(got) == sorted(list(plain) + ["normals", "n_degenerate_normals"])
    assert all(torch.equal(got[k], plain[k]) for k in ("vertices", "faces", "rgb", "grid"))
    # the file carries the normals' bytes between the positions and the colours
    vertex, idx = _read_ply(ply)
    assert vertex.dtype.names == ("xyz", "n", "rgb")
    assert (_bits(vertex["n"]) == _bits(want)).all() and (_bits(vertex["xyz"]) == _bits(got["vertices"].cpu().numpy())).all()
    assert (idx == got["faces"].cpu().numpy()).all() and (vertex["rgb"] == to8b(got["rgb"].cpu().numpy())).all()


def test_the_filter_cuts_the_normals_as_it_cuts_the_vertices(shaded, gpu_modules, tmp_path):
    from nerf_sampling_amd import nerf_utils

    whole, _ = shaded
    d = str(tmp_path / "mesh")
    got = nerf_utils.scene_mesh_shaded(gpu_modules("tiny_synth")["fine"], keep_largest=1, colours=False, savedir=d, **KW)
    want = nerf_utils.mesh_filter(whole["vertices"], whole["faces"], None, keep_largest=1)
    stays = want["index"] >= 0
    assert got["n_components"] > 1 and 0 < int(stays.sum()) < stays.numel(), "the filter drops nothing: the case shows nothing"
    assert torch.equal(got["vertices"], want["vertices"]) and torch.equal(got["faces"], want["faces"])
    assert torch.equal(got["normals"], whole["normals"][stays])
    assert got["n_degenerate_normals"] == whole["n_degenerate_normals"] and got["rgb"] is None
    vertex, idx = _read_ply(os.path.join(d, "scene_mesh.ply"))
    assert vertex.dtype.names == ("xyz", "n") and (_bits(vertex["n"]) == _bits(got["normals"].cpu().numpy())).all()
    assert (idx == got["faces"].cpu().numpy()).all()


@pytest.mark.parametrize("keep_largest", [0, 1])
def test_without_normals_it_is_scene_mesh_filtered(gpu_modules, tmp_path, keep_largest):
    from nerf_sampling_amd import nerf_utils

    net = gpu_modules("tiny_synth")["fine"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    want = nerf_utils.scene_mesh_filtered(net, keep_largest=keep_largest, savedir=a, **KW)
    got = nerf_utils.scene_mesh_shaded(net, keep_largest=keep_largest, savedir=b, normals=False, colour_view="centre", **KW)
    assert list(got) == list(want) and "normals" not in got
    for k in want:
        assert torch.equal(got[k], want[k]) if isinstance(want[k], torch.Tensor) else got[k] == want[k], k
    assert open(os.path.join(a, "scene_mesh.ply"), "rb").read() == open(os.path.join(b, "scene_mesh.ply"), "rb").read()
    with pytest.raises(ValueError):
        nerf_utils.scene_mesh_shaded(net, normals=False, colour_view="normal", **KW)


def test_colour_view_normal_looks_along_the_inward_normal(shaded, gpu_modules, monkeypatch):
    """the colour query's directions, recorded: -n, and the unit vector towards the box centre exactly where n is (0, 0, 0) --
    every fifth normal is zeroed on its way out of ops.mesh_normals, so that the second kind occurs"""
    from nerf_sampling_amd import nerf_utils, ops

    whole, _ = shaded
    net = gpu_modules("tiny_synth")["fine"]
    seen = []
    real_forward, real_normals = ops.nerf_forward, ops.mesh_normals

    def spy(handle, pts, viewdirs):
        seen.append((pts.clone(), viewdirs.clone()))
        return real_forward(handle, pts, viewdirs)

    def some_zero(*args, **kw):
        out = real_normals(*args, **kw)
        out["normals"][::5] = 0.0
        return out

    monkeypatch.setattr(ops, "nerf_forward", spy)
    monkeypatch.setattr(ops, "mesh_normals", some_zero)
    got = nerf_utils.scene_mesh_shaded(net, colour_view="normal", **KW)
    centre = nerf_utils.scene_mesh_shaded(net, colour_view="centre", **KW)
    monkeypatch.undo()
    v, n = got["vertices"], got["normals"]
    assert torch.equal(v, whole["vertices"])
    zero = (n == 0).all(dim=1)
    assert torch.equal(n[~zero], whole["normals"][~zero]) and int(zero.sum()) >= v.shape[0] // 5 and not bool(zero.all())
    towards = -v / (-v).norm(dim=-1, keepdim=True).clamp_min(1e-12)
    # the last call of each run is its colour query: the calls before it sample the lattice (view (0, 0, -1))
    per_run = len(seen) // 2
    (pts, dirs), (pts_centre, dirs_centre) = seen[per_run - 1], seen[-1]
    assert torch.equal(pts[:, 0], v) and torch.equal(pts_centre[:, 0], v)
    assert torch.equal(dirs[~zero], -n[~zero]) and torch.equal(dirs[zero], towards[zero])
    assert torch.equal(dirs_centre, towards)                                              # "centre" is the query it always was
    assert torch.equal(got["rgb"], torch.sigmoid(real_forward(net.packed(), v[:, None, :], dirs)[:, 0, :3]))
    assert torch.equal(centre["rgb"], whole["rgb"]) and not torch.equal(got["rgb"], whole["rgb"])


def test_trainer_writes_the_normals(tmp_path, gpu_modules, shaded):
    """Trainer(device_mesh=True, mesh_normals=True) in a render-only run: scene_mesh.ply is scene_mesh_shaded's; the frames and
    psnr.txt are those of the run without the switch, byte for byte, and without it the file has no normals"""
    from nerf_sampling_amd import nerf_utils, ops

    whole, ply = shaded
    ops.set_compute_dtype("f32")
    focal, K, poses = CL._camera()
    images = np.random.default_rng(7).random((2, CL.H, CL.W, 3), dtype=np.float32)
    files = {}
    for on in (False, True):
        kw = CL._kwargs(gpu_modules, "n16", basedir=str(tmp_path / f"r{int(on)}"), device_mesh=True, mesh_resolution=G,
                        mesh_threshold=THRESHOLD, mesh_bound=BOUND, mesh_normals=on)
        tr = kw["trainer"]
        tr.K, tr.global_step = K, 7
        tr.render(True, False, images, [0, 1], poses, (CL.H, CL.W, focal), kw)
        d = os.path.join(tr.basedir, tr.expname, "renderonly_test_000007")
        files[on] = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
    assert sorted(files[False]) == sorted(files[True]) == ["000.png", "001.png", "psnr.txt", "scene_mesh.ply"]
    assert all(files[True][f] == files[False][f] for f in ("000.png", "001.png", "psnr.txt"))
    assert files[True]["scene_mesh.ply"] == open(ply, "rb").read()
    assert b"property float nx" not in files[False]["scene_mesh.ply"]
    vertex, _ = _read_ply(os.path.join(str(tmp_path / "r1"), "eval", "renderonly_test_000007", "scene_mesh.ply"))
    assert (_bits(vertex["n"]) == _bits(whole["normals"].cpu().numpy())).all()
    nerf_utils.drain_host_copies()
