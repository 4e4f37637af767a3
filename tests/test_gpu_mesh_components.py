"""ns_mesh_components / ops.mesh_components / nerf_utils.mesh_filter: the connected components of a mesh's faces on the device,
and the floater filter of nerf_utils.scene_mesh_filtered built on them.  Yardstick: tests/mesh_components_reference.py, a plain union-find
on the host that restates the header's contract.  Everything is integers: every comparison is exact.

S, the number of faces one workgroup takes per launch, is the header's NS_MESH_COMPONENTS_SHARE.  Every call of ``run`` goes
through the C ABI with the three outputs, the counters and the workspace fenced by FENCE sentinel elements before and after, all
of them holding garbage before the call."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mesh_components_reference as CR
import test_gpu_device_cloud as CL
from test_gpu_device_mesh import BOUND, G, THRESHOLD, _bits, _read_ply

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = int(re.search(r"#define NS_MESH_COMPONENTS_SHARE (\d+)",
                  open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()).group(1))
FENCE = 64                                                   # sentinel elements on either side of every output
SENTINEL = -0x5A5A5A5B
_reference = {}


def reference(name, make):
    """(faces [F,3] int64, V, labels, tri_count, vert_count, n_components, n_ignored) of a named mesh: built and labelled on
    the host once, shared, never modified"""
    if name not in _reference:
        faces, V = make()
        faces = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
        labels, tri, vert, n, ignored = CR.components(faces, V)
        for a in (faces, labels, tri, vert):
            a.setflags(write=False)
        _reference[name] = (faces, int(V), labels, tri, vert, n, ignored)
    return _reference[name]


def run(faces, V, stream=None, workspace_byte=0xA5):
    """One call through the C ABI -> (labels, tri_count, vert_count, n_components, n_ignored) as host arrays, after checking
    that no fence element around the outputs, the counters or the workspace was written"""
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    faces = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    F = faces.shape[0]
    stream = stream or torch.cuda.current_stream()
    need = lib.ns_mesh_components_workspace_bytes(V, F)
    assert need > 0 and need % 8 == 0
    with torch.cuda.stream(stream):
        dev = torch.from_numpy(faces.copy()).cuda() if F else None
        outs = [torch.full((V + 2 * FENCE,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
        counters = torch.full((2 + 2 * FENCE,), SENTINEL, dtype=torch.int64, device="cuda")
        ws = torch.full((need + 2 * FENCE * 8,), workspace_byte, dtype=torch.uint8, device="cuda")
        p = lambda t, off: C.c_void_p(t.data_ptr() + off)                                # noqa: E731
        rc = lib.ns_mesh_components(None if dev is None else C.c_void_p(dev.data_ptr()), F, V, *(p(o, 4 * FENCE) for o in outs),
                                    p(counters, 8 * FENCE), p(ws, 8 * FENCE), C.c_void_p(stream.cuda_stream))
        assert rc == 0, lib.ns_last_error()
        stream.synchronize()
    host = [o.cpu().numpy() for o in outs]
    for h in host:
        assert (h[:FENCE] == SENTINEL).all() and (h[FENCE + V:] == SENTINEL).all(), "written outside [0, V)"
    c = counters.cpu().numpy()
    assert (c[:FENCE] == SENTINEL).all() and (c[FENCE + 2:] == SENTINEL).all(), "written around the counters"
    w = ws.cpu().numpy()
    assert (w[:8 * FENCE] == workspace_byte).all() and (w[8 * FENCE + need:] == workspace_byte).all(), "written outside the workspace"
    labels, tri, vert = (h[FENCE:FENCE + V] for h in host)
    return labels, tri, vert, int(c[FENCE]), int(c[FENCE + 1])


def check(name, make, **kw):
    faces, V, labels, tri, vert, n, ignored = reference(name, make)
    got = run(faces, V, **kw)
    assert got[3:] == (n, ignored), f"{name}: (components, ignored) = {got[3:]}, want {(n, ignored)}"
    assert np.array_equal(got[0], labels), f"{name}: {(got[0] != labels).sum()} labels differ"
    assert np.array_equal(got[1], tri) and np.array_equal(got[2], vert), f"{name}: counts differ"
    return got


@pytest.mark.parametrize("case", CR.HAND_CASES, ids=[c[0] for c in CR.HAND_CASES])
def test_hand_cases(case):
    faces, V, labels, tri, vert, n, ignored = CR.hand_case(case)
    got = run(faces, V)
    assert np.array_equal(got[0], labels) and np.array_equal(got[1], tri) and np.array_equal(got[2], vert)
    assert got[3:] == (n, ignored)


CHAIN = 3 * S + 5


def _numbering(order):
    V = CHAIN + 2
    if order == "in order":
        return np.arange(V)
    if order == "reversed":
        return np.arange(V)[::-1].copy()
    return np.random.default_rng(20).permutation(V)


@pytest.mark.parametrize("order", ["in order", "reversed", "permuted"])
def test_long_chain(order):
    """a strip across more than three shares: the longest walks there are.  One component, every label 0; then the same strip in
    seven pieces"""
    number = _numbering(order)
    got = check(f"chain {order}", lambda: (number[CR.strip(CHAIN)], CHAIN + 2))
    assert (got[0] == 0).all() and got[1][0] == CHAIN and got[2][0] == CHAIN + 2 and got[3] == 1
    gone = np.concatenate([[c, c + 1] for c in (S // 2, S - 1, S + 7, 2 * S - 1, 2 * S + 300, 3 * S - 2)])
    got = check(f"chain {order} cut", lambda: (number[np.delete(CR.strip(CHAIN), gone, axis=0)], CHAIN + 2))
    assert got[3] == 7 and got[1].sum() == CHAIN - 12 and got[2].sum() == CHAIN + 2


@pytest.mark.parametrize("F", [0, 1, S - 1, S, S + 1, 2 * S + 1])
def test_share_boundaries(F):
    got = check(f"strip {F}", lambda: (CR.strip(F), F + 2))
    assert got[3] == (1 if F else 2)


def test_no_vertices_and_one_vertex():
    assert run(np.empty((0, 3), np.int64), 0)[3:] == (0, 0)
    labels, tri, vert, n, ignored = run(CR.strip(5), 0)                                    # every face is out of range
    assert (n, ignored) == (0, 5) and labels.size == tri.size == vert.size == 0
    labels, tri, vert, n, ignored = run(np.empty((0, 3), np.int64), 1)
    assert (labels.tolist(), tri.tolist(), vert.tolist(), n, ignored) == ([0], [0], [1], 1, 0)
    labels, tri, vert, n, ignored = run([(0, 0, 0), (0, 1, 0)], 1)
    assert (labels.tolist(), tri.tolist(), vert.tolist(), n, ignored) == ([0], [1], [1], 1, 1)


def _random_faces(F, V=5000, bad=0):
    rng = np.random.default_rng(1000 + F + bad)
    faces = rng.integers(0, V, size=(F, 3), dtype=np.int64)
    if bad:
        rows = rng.choice(F, size=bad, replace=False)
        faces[rows, rng.integers(0, 3, size=bad)] = rng.choice([-1, V, V + 1, -2 ** 40, 2 ** 40, 2 ** 31, 2 ** 32 + 7], size=bad)
    return faces, V


@pytest.mark.parametrize("F,bad", [(1200, 0), (20000, 0), (1200, 9), (20000, 9)])
def test_random_faces(F, bad):
    got = check(f"random {F} {bad}", lambda: _random_faces(F, bad=bad))
    assert got[4] == bad
    print(f"F = {F}: {got[3]} components, the largest of {got[2].max()} vertices")
    assert (got[3] > 1000 and got[2].max() < 2500) if F == 1200 else (1 <= got[3] < 100 and got[2].max() > 4900)


# ---- extracted surfaces: a 40^3 lattice over [-1, 1]^3 through ops.mesh_extract + ops.mesh_weld -----------------------------
N = 40


def _points():
    x = np.linspace(-1.0, 1.0, N).astype(np.float32).astype(np.float64)
    return np.meshgrid(x, x, x, indexing="ij")[::-1]                                       # sigma is [Gz,Gy,Gx]


def _ball(centre, radius):
    X, Y, Z = _points()
    return radius - np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2)


def _surface(sigma):
    """the welded mesh of sigma == 0 as device tensors"""
    from nerf_sampling_amd import ops

    h = float(np.float32(2.0 / (N - 1)))
    got = ops.mesh_extract(torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float32)).cuda(), 0.0, [-1.0] * 3, [h] * 3)
    assert got["n_skipped"] == 0
    return ops.mesh_weld(got["triangles"], got["keys"])


def _shapes():
    X, Y, Z = _points()
    r = np.sqrt(X ** 2 + Y ** 2 + Z ** 2)
    return {
        "balls": (np.maximum.reduce([_ball((-0.5, -0.5, -0.5), 0.3), _ball((0.45, 0.4, -0.3), 0.35), _ball((0.0, -0.3, 0.55), 0.25)]),
                  [2, 2, 2]),
        "shell": (np.minimum(0.7 - r, r - 0.35), [2, 2]),                                  # the outer surface and the cavity's
        "torus": (0.2 - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - 0.55) ** 2 + Z ** 2), [0]),
    }


@pytest.mark.parametrize("shape", ["balls", "shell", "torus"])
def test_extracted_surfaces(shape):
    """three balls, a hollow shell and a torus: six closed surfaces in all.  A closed surface has E = 3 F / 2, so
    V - F / 2 is its Euler characteristic: 2 for the sphere-like ones, 0 for the torus"""
    from nerf_sampling_amd import ops

    sigma, chi = _shapes()[shape]
    vertices, faces = _surface(sigma)
    V = int(vertices.shape[0])
    got = ops.mesh_components(faces, V)
    labels, tri, vert, n, ignored = CR.components(faces.cpu().numpy(), V)
    assert (got["n_components"], got["n_ignored"]) == (n, ignored) == (len(chi), 0)
    assert all(got[k].dtype == torch.int32 and got[k].is_cuda and tuple(got[k].shape) == (V,) for k in ("labels", "triangles", "vertices"))
    assert np.array_equal(got["labels"].cpu().numpy(), labels) and np.array_equal(got["triangles"].cpu().numpy(), tri)
    assert np.array_equal(got["vertices"].cpu().numpy(), vert)
    roots = np.flatnonzero(labels == np.arange(V))
    print(f"{shape}: {faces.shape[0]} triangles on {V} vertices; per component {tri[roots].tolist()} on {vert[roots].tolist()}")
    assert (tri[roots] % 2 == 0).all() and sorted((vert[roots] - tri[roots] // 2).tolist()) == sorted(chi)


BLOBS = [((0.75, 0.02, 0.01), 0.08), ((-0.76, 0.03, 0.0), 0.09), ((0.01, 0.77, -0.02), 0.10), ((0.0, -0.02, -0.78), 0.07)]


def test_filter_gives_back_the_ball_bit_for_bit():
    """lattice A: a ball.  Lattice B: the ball and four blobs, every field clipped to +-1.5 cells, and the blobs' surfaces 3.9
    cells from the ball's and 2.5 from the boundary or more: where one field is above its floor the other one is at it, so the
    cells that cross the ball's surface hold the same values in both.  Order is kept and a vertex's bits depend on its lattice edge
    alone: the filtered mesh of B IS A's"""
    from nerf_sampling_amd import nerf_utils

    c = 1.5 * 2.0 / (N - 1)
    A = np.clip(_ball((0.0, 0.0, 0.0), 0.45), -c, c)
    B = np.maximum.reduce([A] + [np.clip(_ball(centre, radius), -c, c) for centre, radius in BLOBS])
    assert ((B != A) <= (A == -c)).all() and (B != A).any()
    va, fa = _surface(A)
    vb, fb = _surface(B)
    tag = torch.arange(vb.shape[0], device="cuda", dtype=torch.float32)[:, None].expand(-1, 3).contiguous()
    for kw in (dict(keep_largest=1), dict(min_component_triangles=1000), dict(min_component_triangles=1000, keep_largest=3)):
        got = nerf_utils.mesh_filter(vb, fb, tag, **kw)
        sizes = got["component_triangles"].cpu().numpy()
        assert got["n_components"] == 5 == sizes.size and got["n_kept_components"] == 1
        assert sizes.sum() == fb.shape[0] and np.sort(sizes)[-2] < 1000 < sizes.max() == fa.shape[0]
        assert got["n_dropped_triangles"] == fb.shape[0] - fa.shape[0] > 0
        assert torch.equal(got["faces"], fa) and torch.equal(got["vertices"].view(torch.int32), va.view(torch.int32))
        kept = torch.nonzero(got["index"] >= 0)[:, 0]
        assert torch.equal(got["rgb"][:, 0].long(), kept) and torch.equal(got["index"][kept], torch.arange(va.shape[0], device="cuda"))
    everything = nerf_utils.mesh_filter(vb, fb)
    assert torch.equal(everything["faces"], fb) and torch.equal(everything["vertices"], vb) and everything["rgb"] is None
    assert everything["n_kept_components"] == 5 and everything["n_dropped_triangles"] == 0


# ---- through scene_mesh_filtered and the Trainer, on the tiny_synth field as tests/test_gpu_device_mesh.py ----------------------------
def test_scene_mesh_filters_before_it_colours(gpu_modules, tmp_path):
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.run_nerf_helpers import to8b

    net = gpu_modules("tiny_synth")["fine"]
    d = str(tmp_path / "mesh")
    plain = nerf_utils.scene_mesh(net, bound=BOUND, resolution=G, threshold=THRESHOLD)
    assert sorted(plain) == ["faces", "h", "lo", "n_skipped", "n_triangles", "rgb", "vertices"]              # today's keys
    off = nerf_utils.scene_mesh_filtered(net, bound=BOUND, resolution=G, threshold=THRESHOLD)                # both arguments 0
    assert sorted(off) == sorted(plain) and all(torch.equal(off[k], plain[k]) for k in ("vertices", "faces", "rgb"))
    got = nerf_utils.scene_mesh_filtered(net, bound=BOUND, resolution=G, threshold=THRESHOLD, keep_largest=1, savedir=d)
    assert sorted(got) == sorted(list(plain) + ["n_components", "n_kept_components", "n_dropped_triangles", "component_triangles"])
    sizes = got["component_triangles"]
    print(f"{got['n_components']} components of {sizes.cpu().tolist()} triangles; {got['n_dropped_triangles']} triangles dropped")
    assert got["n_triangles"] == plain["n_triangles"] == plain["faces"].shape[0] and got["n_kept_components"] == 1
    assert got["n_triangles"] - got["n_dropped_triangles"] == got["faces"].shape[0] == int(sizes.max())
    assert sizes.is_cuda and sizes.numel() == got["n_components"] and int(sizes.sum()) == got["n_triangles"]
    V = got["vertices"].shape[0]
    assert int(got["faces"].min()) == 0 and int(got["faces"].max()) == V - 1
    assert torch.unique(got["faces"]).numel() == V                                        # every kept vertex is in a kept face
    want = nerf_utils.mesh_filter(plain["vertices"], plain["faces"], plain["rgb"], keep_largest=1)
    assert torch.equal(got["faces"], want["faces"]) and torch.equal(got["vertices"], want["vertices"])
    assert torch.equal(got["rgb"], want["rgb"])                                           # field rows are independent
    vertex, idx = _read_ply(os.path.join(d, "scene_mesh.ply"))
    assert (_bits(vertex["xyz"]) == _bits(got["vertices"].cpu().numpy())).all() and (idx == got["faces"].cpu().numpy()).all()
    assert (vertex["rgb"] == to8b(got["rgb"].cpu().numpy())).all()
    both = nerf_utils.scene_mesh_filtered(net, bound=BOUND, resolution=G, threshold=THRESHOLD, min_component_triangles=int(sizes.max()),
                                 keep_largest=1, colours=False)
    assert torch.equal(both["faces"], got["faces"]) and both["rgb"] is None and both["n_kept_components"] == 1


def test_trainer_writes_the_filtered_mesh(tmp_path, gpu_modules):
    """Trainer(device_mesh=True, mesh_keep_largest=1) in a render-only run: scene_mesh.ply is scene_mesh_filtered(keep_largest=1)'s; the
    frames and psnr.txt are those of the run without the filter, byte for byte"""
    from nerf_sampling_amd import nerf_utils, ops

    ops.set_compute_dtype("f32")
    focal, K, poses = CL._camera()
    images = np.random.default_rng(7).random((2, CL.H, CL.W, 3), dtype=np.float32)
    files = {}
    for largest in (0, 1):
        kw = CL._kwargs(gpu_modules, "n16", basedir=str(tmp_path / f"r{largest}"), device_mesh=True, mesh_resolution=G,
                        mesh_threshold=THRESHOLD, mesh_bound=BOUND, mesh_keep_largest=largest)
        tr = kw["trainer"]
        tr.K, tr.global_step = K, 7
        tr.render(True, False, images, [0, 1], poses, (CL.H, CL.W, focal), kw)
        d = os.path.join(tr.basedir, tr.expname, "renderonly_test_000007")
        files[largest] = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
    assert sorted(files[0]) == sorted(files[1]) == ["000.png", "001.png", "psnr.txt", "scene_mesh.ply"]
    assert all(files[1][f] == files[0][f] for f in ("000.png", "001.png", "psnr.txt"))
    vertex, idx = _read_ply(os.path.join(str(tmp_path / "r1"), "eval", "renderonly_test_000007", "scene_mesh.ply"))
    direct = nerf_utils.scene_mesh_filtered(gpu_modules("tiny_synth")["fine"], bound=BOUND, resolution=G, threshold=THRESHOLD,
                                             keep_largest=1)
    assert (_bits(vertex["xyz"]) == _bits(direct["vertices"].cpu().numpy())).all() and (idx == direct["faces"].cpu().numpy()).all()
    nerf_utils.drain_host_copies()


# ---- the result depends on the inputs alone ---------------------------------------------------------------------------------
def test_two_runs_streams_and_workspace_contents():
    name, make = "random 20000 9", lambda: _random_faces(20000, bad=9)
    first = check(name, make)
    second = check(name, make, stream=torch.cuda.Stream())
    third = check(name, make, workspace_byte=0xFF)
    for other in (second, third):
        assert all(np.array_equal(a, b) for a, b in zip(first[:3], other[:3])) and first[3:] == other[3:]
    from nerf_sampling_amd import ops

    faces, V = reference(name, make)[:2]
    dev = torch.from_numpy(faces.copy()).cuda()
    ws = torch.full((ops.mesh_components_workspace_bytes(V, faces.shape[0]),), 0xFF, dtype=torch.uint8, device="cuda")
    a, b = ops.mesh_components(dev, V), ops.mesh_components(dev, V, workspace=ws)
    assert all(torch.equal(a[k], b[k]) for k in ("labels", "triangles", "vertices")) and a["n_components"] == b["n_components"] == first[3]
    assert np.array_equal(a["labels"].cpu().numpy(), first[0]) and a["n_ignored"] == 9
    with pytest.raises(ValueError):
        ops.mesh_components(dev, V, workspace=ws[1:])                                      # misaligned and too small
    with pytest.raises(ValueError):
        ops.mesh_components(dev.to(torch.int32), V)
    with pytest.raises(ValueError):
        ops.mesh_components(dev.t(), V)
