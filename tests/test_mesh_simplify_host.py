"""The mesh simplification's host side: the numpy restatement (tests/mesh_simplify_reference.py) on cases worked out by hand and on
the analytic ball; the library's own cluster arithmetic (csrc/ns_mesh_cluster.h through ns_mesh_cluster_coord and
ns_mesh_cluster_distance, which run on the host) against it, bit for bit; the argument checks and workspace sizes of
ns_mesh_simplify through the library on a machine without a GPU; ops.mesh_simplify's argument errors and its plain-torch parts on
CPU tensors; the new switches."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mesh_reference as MR
import mesh_simplify_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = int(re.search(r"#define NS_MESH_SIMPLIFY_SHARE (\d+)", open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()).group(1))


@pytest.mark.parametrize("case", SR.HAND_CASES, ids=[c[0] for c in SR.HAND_CASES])
def test_reference_on_hand_cases(case):
    vertices, faces, lo, cell, dims, rep, faces_out, count, index, new_faces, n_duplicate = SR.hand_case(case)
    got_rep, got_faces, got_count = SR.entry(vertices, faces, lo, cell, dims)
    assert got_rep.dtype == np.int32 and np.array_equal(got_rep, rep)
    assert np.array_equal(got_faces, faces_out) and np.array_equal(got_count, count)
    whole = SR.simplify(vertices, faces, lo, cell, dims)
    assert np.array_equal(whole["index"], index) and np.array_equal(whole["faces"], new_faces)
    assert whole["n_duplicate"] == n_duplicate and whole["vertices"].shape[0] == count[5] == (index >= 0).sum()
    kept = np.flatnonzero(index >= 0)
    assert np.array_equal(whole["vertices"].view(np.int32), vertices[kept].view(np.int32))
    undeduped = SR.simplify(vertices, faces, lo, cell, dims, dedupe_faces=False)
    assert undeduped["n_duplicate"] == 0 and undeduped["faces"].shape[0] == count[0]
    # a capacity below the kept faces cuts the output and leaves the counters
    _, cut, cut_count = SR.entry(vertices, faces, lo, cell, dims, capacity=1)
    assert np.array_equal(cut, faces_out[:1]) and np.array_equal(cut_count, count)


def test_reference_words_by_hand():
    """the tie case's numbers: u, S, n, d, d32 and the 64-bit word"""
    vertices = np.array([(0.25, 0.5, 0.5), (0.75, 0.5, 0.5)], dtype=np.float32)
    c = SR.clusters(vertices, (0, 0, 0), (1, 1, 1), (1, 1, 1))
    assert c["u"].tolist() == [[16384, 32768, 32768], [49152, 32768, 32768]] and c["lin"].tolist() == [0, 0]
    assert c["S"].tolist() == [[65536, 65536, 65536]] and c["n"].tolist() == [1 + 1]
    assert c["d32"].tolist() == [2.0 ** 28, 2.0 ** 28] and c["d32"].dtype == np.float32
    assert c["word"].tolist() == [0x4D800000 << 32, (0x4D800000 << 32) | 1] and c["word"].dtype == np.uint64
    # a cell of 0.5 from -1: u = (v + 1) / 0.5 * 65536, and the cell index along y and z
    c = SR.clusters(np.array([(-1.0, 0.0, 0.75)], dtype=np.float32), (-1, -1, -1), (0.5, 0.5, 0.5), (4, 4, 4))
    assert c["u"].tolist() == [[0, 131072, 229376]] and c["lin"].tolist() == [(3 * 4 + 2) * 4 + 0] and c["rep"].tolist() == [0]


def _ball(G=24):
    sigma, lo, h = MR.sphere(G)
    triangles, keys, _ = MR.march(sigma, 0.0, lo, h)
    vertices, faces = MR.weld(triangles, keys)
    return vertices, faces, lo, h


def ball_lattice(lo, h, G, factor):
    cell = (h * np.float32(factor)).astype(np.float32)
    return lo, cell, [int(np.ceil((G - 1) / factor))] * 3


@pytest.mark.parametrize("factor", [2, 3])
def test_the_volume_bound_holds_for_the_reference(factor):
    """the analytic ball on 24^3, by numpy alone: a vertex and its representative lie in one cell, so no vertex moves farther than
    a cell's diagonal, and the signed volume changes by no more than the input's area times that -- which
    tests/test_gpu_mesh_simplify.py then asks of the kernel"""
    G = 24
    vertices, faces, lo, h = _ball(G)
    lo, cell, dims = ball_lattice(lo, h, G, factor)
    got = SR.simplify(vertices, faces, lo, cell, dims)
    diagonal = float(np.linalg.norm(cell.astype(np.float64)))
    moved = np.linalg.norm(vertices.astype(np.float64) - vertices[got["rep"]].astype(np.float64), axis=1)
    volume_in, volume_out = SR.signed_volume(vertices, faces), SR.signed_volume(got["vertices"], got["faces"])
    bound = SR.surface_area(vertices, faces) * diagonal
    print(f"factor {factor}: {faces.shape[0]} -> {got['faces'].shape[0]} faces, {vertices.shape[0]} -> {got['vertices'].shape[0]} "
          f"vertices, {got['n_duplicate']} duplicates; moved at most {moved.max():.4f} of {diagonal:.4f}; volume {volume_in:.4f} -> "
          f"{volume_out:.4f}, bound {bound:.4f}")
    assert moved.max() <= diagonal and abs(volume_out - volume_in) <= bound
    assert 0 < got["faces"].shape[0] < faces.shape[0] / factor and got["n_invalid"] == got["n_nonfinite"] == 0
    sets = {tuple(sorted(f)) for f in got["faces"].tolist()}
    assert len(sets) == got["faces"].shape[0]                                  # after dedupe no two faces share a vertex set


# ---- the library's own text (csrc/ns_mesh_cluster.h) on the host ------------------------------------------------------------
def _lib_coord(lib, vertex, lo, cell, dims):
    v, l, c = (np.array(a, dtype=np.float32) for a in (vertex, lo, cell))
    d = np.array(dims, dtype=np.int32)
    u, lin = np.zeros(3, dtype=np.int32), np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                 # noqa: E731
    rc = lib.ns_mesh_cluster_coord(p(v), p(l), p(c), p(d), p(u), p(lin))
    return rc, u.tolist(), int(lin[0])


def test_cluster_header_on_boundary_cases():
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    lo, cell, dims = (0, 0, 0), (1, 1, 1), (2, 2, 1)
    top = 2 * 65536 - 1
    for x, u, cx in [(1.0, 65536, 1), (SR._A, 65536, 1), (SR._B, 65534, 0), (0.0, 0, 0), (-0.0, 0, 0), (-3.0, 0, 0),
                     (-3e38, 0, 0), (2.0, top, 1), (7.0, top, 1), (3e38, top, 1), (2.0 - 2.0 ** -17, top, 1),
                     (2.0 ** -17, 0, 0), (3 * 2.0 ** -17, 2, 0), (1e-45, 0, 0)]:
        rc, got_u, lin = _lib_coord(lib, (x, 0.5, 0.5), lo, cell, dims)
        assert (rc, got_u, lin) == (1, [u, 32768, 32768], cx), x
        ref_u, ref_lin, _ = SR.coords(np.array([(x, 0.5, 0.5)], dtype=np.float32), lo, cell, dims)
        assert ref_u[0].tolist() == got_u and ref_lin[0] == lin
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            v = [0.5, 0.5, 0.5]
            v[axis] = bad
            assert _lib_coord(lib, v, lo, cell, dims) == (0, [0, 0, 0], -1)
    # the smallest cell and the largest distance there are: the quotient is finite and clamps
    assert _lib_coord(lib, (3e38, -3e38, 0.0), (-3e38, 3e38, 0), (1e-45, 1e-45, 1), (32768, 1, 1))[1] == [2 ** 31 - 1, 0, 0]
    for kw in (dict(dims=(0, 1, 1)), dict(dims=(1, 32769, 1)), dict(dims=(512, 512, 128)), dict(cell=(0, 1, 1)),
               dict(cell=(1, -1, 1)), dict(cell=(1, 1, np.nan)), dict(cell=(np.inf, 1, 1)), dict(lo=(np.nan, 0, 0)),
               dict(lo=(0, np.inf, 0))):
        args = dict(lo=lo, cell=cell, dims=dims)
        args.update(kw)
        assert _lib_coord(lib, (0.5, 0.5, 0.5), args["lo"], args["cell"], args["dims"])[0] == -1, kw


def test_cluster_header_against_the_reference_on_random_vertices():
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(5)
    lo, cell, dims = (-0.7, 0.1, 2.5), (0.013, 0.37, 1.1), (150, 9, 4)
    vertices = (rng.uniform(-0.2, 1.2, size=(400, 3)) * (np.array(cell) * np.array(dims)) + np.array(lo)).astype(np.float32)
    u, lin, finite = SR.coords(vertices, lo, cell, dims)
    assert finite.all() and (lin >= 0).all() and lin.max() < 150 * 9 * 4 and len(set(lin.tolist())) > 200
    for v in range(vertices.shape[0]):
        assert _lib_coord(lib, vertices[v], lo, cell, dims) == (1, u[v].tolist(), int(lin[v])), v
    # the distance: random members of random clusters, small and at the largest sums there are
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                 # noqa: E731
    for _ in range(300):
        n = int(rng.choice([1, 2, 3, 7, 1000, 2 ** 31 - 1]))
        centre = rng.integers(0, 2 ** 31, size=3)
        sums = np.array([int(c) * n - int(rng.integers(0, n)) for c in centre], dtype=np.int64)
        uu = rng.integers(0, 2 ** 31, size=3).astype(np.int32)
        d = np.zeros(1, dtype=np.float32)
        assert lib.ns_mesh_cluster_distance(p(uu), p(sums), n, p(d)) == 0
        want = SR.distance2(uu.astype(np.int64), sums, n)
        assert d.view(np.int32)[0] == np.float32(want).view(np.int32), (uu, sums, n)
    assert lib.ns_mesh_cluster_distance(p(uu), p(sums), 0, p(d)) == -1


# ---- ns_mesh_simplify's refusals and sizes, without a device ------------------------------------------------------------------
def test_argument_checks_without_a_gpu():
    """every refusal comes before any HIP call: -1 (NS_E_INVALID) on a machine without a GPU, the device pointers never
    dereferenced"""
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    p = C.c_void_p
    vertices, faces, rep, out, count, ws = p(0x1000), p(0x2000), p(0x3000), p(0x4000), p(0x5000), p(0x6000)
    host = lambda a: a.ctypes.data_as(C.c_void_p)                              # noqa: E731

    def call(vertices=vertices, V=9, faces=faces, F=8, lo=(0, 0, 0), cell=(1, 1, 1), dims=(4, 4, 4), rep=rep, out=out,
             capacity=8, count=count, ws=ws):
        lo, cell = (None if a is None else np.array(a, dtype=np.float32) for a in (lo, cell))
        dims = None if dims is None else np.array(dims, dtype=np.int32)
        return lib.ns_mesh_simplify(vertices, V, faces, F, *(None if a is None else host(a) for a in (lo, cell, dims)), rep, out,
                                    capacity, count, ws, None)

    bad = [dict(V=-1), dict(F=-1), dict(V=2 ** 31), dict(F=2 ** 31), dict(V=-2 ** 63), dict(F=2 ** 62),
           dict(dims=(0, 4, 4)), dict(dims=(4, -1, 4)), dict(dims=(4, 4, 2 ** 15 + 1)), dict(dims=(257, 256, 256)),
           dict(dims=(2 ** 15, 2 ** 15, 2 ** 15)), dict(dims=(2 ** 15, 513, 1)),
           dict(cell=(0, 1, 1)), dict(cell=(1, -1, 1)), dict(cell=(1, 1, -0.0)), dict(cell=(np.nan, 1, 1)), dict(cell=(1, np.inf, 1)),
           dict(lo=(np.nan, 0, 0)), dict(lo=(0, -np.inf, 0)), dict(lo=None), dict(cell=None), dict(dims=None),
           dict(capacity=-1), dict(count=None), dict(ws=None), dict(count=None, V=0, F=0), dict(ws=None, V=0, F=0),
           dict(vertices=None), dict(rep=None), dict(faces=None), dict(out=None), dict(out=None, V=0), dict(faces=None, V=0),
           dict(faces=p(0x2004)), dict(out=p(0x4004)), dict(count=p(0x5004)), dict(ws=p(0x6004)), dict(vertices=p(0x1002)),
           dict(rep=p(0x3002)), dict(rep=p(0x3001))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"ns_mesh_simplify" in lib.ns_last_error()
    size = lib.ns_mesh_simplify_workspace_bytes
    table = lambda cells: (cells * 40 + 255) // 256 * 256                      # noqa: E731
    counts = lambda F: (-(-F // S) * 32 + 255) // 256 * 256                    # noqa: E731
    assert size(9, 8, 4, 4, 4) == 256 + counts(8) + table(64) and size(0, 0, 1, 1, 1) == 256 + 0 + 256
    assert size(5000, 10000, 8, 8, 8) == 256 + counts(10000) + table(512)
    assert size(2 ** 31 - 1, 2 ** 31 - 1, 256, 256, 256) == 256 + counts(2 ** 31 - 1) + 40 * 2 ** 24
    assert size(1, 1, 2 ** 15, 512, 1) == 256 + 256 + 40 * 2 ** 24 and size(1, 1, 128, 128, 128) == 256 + 256 + 40 * 2 ** 21
    for args in ((-1, 8, 4, 4, 4), (9, -1, 4, 4, 4), (2 ** 31, 8, 4, 4, 4), (9, 2 ** 31, 4, 4, 4), (9, 8, 0, 4, 4), (9, 8, 4, 4, -4),
                 (9, 8, 2 ** 15 + 1, 1, 1), (9, 8, 257, 256, 256), (9, 8, 2 ** 15, 2 ** 15, 2 ** 15), (-2 ** 63, 0, 1, 1, 1)):
        assert size(*args) == 0, args
    assert S > 0 and S % 256 == 0


def test_ops_mesh_simplify_refuses_before_any_launch():
    from nerf_sampling_amd import ops

    vertices, faces = torch.zeros((5, 3)), torch.zeros((4, 3), dtype=torch.int64)
    lattice = ((0, 0, 0), (1, 1, 1), (2, 2, 2))
    for v, f in ((vertices, faces), (vertices.numpy(), faces.numpy()), (None, None)):              # not on the device
        with pytest.raises(ValueError, match="vertices"):
            ops.mesh_simplify(v, f, *lattice)
    for lo, cell, dims, word in [((0, 0), (1, 1, 1), (2, 2, 2), "three"), ((0, 0, np.nan), (1, 1, 1), (2, 2, 2), "lo"),
                                 ((0, 0, 0), (1, 0, 1), (2, 2, 2), "cell"), ((0, 0, 0), (1, 1e-60, 1), (2, 2, 2), "cell"),
                                 ((0, 0, 0), (1, np.inf, 1), (2, 2, 2), "cell"), ((0, 0, 0), (1, 1, 1), (2, 0, 2), "dims"),
                                 ((0, 0, 0), (1, 1, 1), (2, 2.5, 2), "dims"), ((0, 0, 0), (1, 1, 1), (2 ** 15 + 1, 1, 1), "dims"),
                                 ((0, 0, 0), (1, 1, 1), (257, 256, 256), "dims"), ((0, 0, 0), (1, 1, 1), None, "three")]:
        with pytest.raises(ValueError, match=word):
            ops.mesh_simplify(vertices, faces, lo, cell, dims)
    s = inspect.signature(ops.mesh_simplify).parameters
    assert list(s) == ["vertices", "faces", "lo", "cell", "dims", "extras", "dedupe", "workspace"]
    assert (s["extras"].default, s["dedupe"].default, s["workspace"].default) == ((), True, None)
    assert ops.mesh_simplify_workspace_bytes(9, 8, (4, 4, 4)) == 256 + 256 + 2560
    assert ops.mesh_simplify_workspace_bytes(9, 8, (0, 4, 4)) == 0 and ops.mesh_simplify_workspace_bytes(9, 8, (2 ** 40, 1, 1)) == 0


def test_first_of_each_vertex_set_is_the_reference_dedupe():
    """ops.mesh_simplify's plain-torch dedupe on CPU tensors: the first occurrence of a vertex set stays, whatever its winding"""
    from nerf_sampling_amd import ops

    rng = np.random.default_rng(3)
    for V, F in ((4, 60), (9, 400), (2 ** 31 - 1, 50), (1, 0)):
        faces = rng.integers(0, min(V, 12), size=(F, 3), dtype=np.int64)
        if V > 12:
            faces[::3] += V - 12                                               # the largest indices there are: no overflow
        want, n_duplicate = SR.dedupe(faces)
        first = ops._first_of_each_vertex_set(torch.from_numpy(faces), V)
        assert first.dtype == torch.bool and np.array_equal(faces[first.numpy()], want) and int((~first).sum()) == n_duplicate
        assert n_duplicate > 0 or F < 60


def test_new_switch_defaults_off_and_rejects_negatives():
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.experiments.render import main
    from nerf_sampling_amd.experiments.run import main as run_main
    from nerf_sampling_amd.trainers import Trainer

    assert inspect.signature(Trainer.__init__).parameters["mesh_simplify"].default == 0
    shaded = inspect.signature(nerf_utils.scene_mesh_shaded).parameters
    s = inspect.signature(nerf_utils.scene_mesh_simplified).parameters
    assert list(s) == list(shaded) + ["simplify"] and s["simplify"].default == 0
    assert all(s[k].default == v.default for k, v in shaded.items())
    assert list(inspect.signature(nerf_utils.mesh_simplify).parameters)[:4] == ["mesh", "lo", "cell", "dims"]
    base = dict(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="")
    assert Trainer(**base).mesh_simplify == 0 and Trainer(**base, device_mesh=True, mesh_simplify=2.5).mesh_simplify == 2.5
    for value in (-1, -0.5, "2", True, float("nan"), float("inf"), None):
        with pytest.raises(ValueError):
            Trainer(**base, mesh_simplify=value)
    for command in (main, run_main):
        opt = {o.name: o for o in command.params}["mesh_simplify"]
        assert opt.default == 0 and "--mesh-simplify" in opt.opts and opt.type.convert("2.5", opt, None) == 2.5
        with pytest.raises(Exception):
            opt.type.convert("-1", opt, None)
    for value in (-1, float("nan"), "2", True):
        with pytest.raises(ValueError):
            nerf_utils.scene_mesh_simplified(None, simplify=value)
    # the cluster lattice of a factor: the density lattice's own lo, cells of k h, enough of them to cover it
    lo, h, G = nerf_utils.mesh_lattice(-1.5, 1.5, 24)
    assert nerf_utils.simplify_lattice(lo, h, G, 2) == (lo, [float(np.float32(2 * v)) for v in h], [12, 12, 12])
    assert nerf_utils.simplify_lattice(lo, h, G, 3)[2] == [8, 8, 8] and nerf_utils.simplify_lattice(lo, h, G, 2.5)[2] == [10, 10, 10]
    assert nerf_utils.simplify_lattice(lo, h, G, 100)[2] == [1, 1, 1]
    with pytest.raises(ValueError):
        nerf_utils.scene_mesh_simplified(None, resolution=1024, simplify=1)       # 1023^3 cells: over the table's limit
