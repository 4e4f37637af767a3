"""The host side of the device mesh (not gpu): the numpy restatement tests/test_gpu_mesh_extract.py measures ns_mesh_extract
against -- on cells worked out by hand, and judged by the invariants of a closed oriented surface, which neither it nor the
kernel defines --, the PLY writer, the new switches and their defaults, and the entry's argument checks through the library."""

import ctypes as C
import inspect

import numpy as np
import pytest

import mesh_reference as MR

BALL = 4.0 / 3.0 * np.pi * 0.7 ** 3


def _cell(values):
    """one cell whose corner with code dx + 2 dy + 4 dz has values[code]"""
    return np.asarray(values, dtype=np.float32).reshape(2, 2, 2)


def test_corner_000_alone_inside_gives_six_triangles():
    """000 is a corner of all six tetrahedra: one triangle each, on the seven lattice edges that leave 000 (three axes, three
    face diagonals, the body diagonal), all at half way, around the corner and facing away from it"""
    s = _cell([1, -1, -1, -1, -1, -1, -1, -1])
    tri, keys, skipped = MR.march(s, 0.0, np.zeros(3), np.ones(3))
    assert tri.shape == (6, 3, 3) and keys.shape == (6, 3) and skipped == 0
    assert sorted(set(keys.reshape(-1).tolist())) == [1, 2, 3, 4, 5, 6, 7]                # lin(000) = 0: the key is d's code
    for p, k in zip(tri.reshape(-1, 3), keys.reshape(-1)):
        assert p.tolist() == [0.5 * (k & 1), 0.5 * ((k >> 1) & 1), 0.5 * (k >> 2)]
    # tetrahedron 0 is x, y, z: w1 = 100, w2 = 110, w3 = 111 -- its triangle is (000-100, 000-110, 000-111) or its mirror
    assert sorted(keys[0].tolist()) == [1, 3, 7]
    normals = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (normals @ np.ones(3) > 0).all()                                               # away from 000
    # the fan is the three far faces of the cube [0, 1/2]^3 (each Kuhn tetrahedron scaled by a half); the three near faces lie
    # in planes through the origin and add nothing to sum p0 . (p1 x p2)
    assert MR.invariants(tri, keys)[2] == 0.125
    inside_out = MR.march(-s, 0.0, np.zeros(3), np.ones(3))
    assert (inside_out[1][:, [0, 2, 1]] == keys).all()                                    # the complement: the same triangles, mirrored


def test_one_non_diagonal_corner_inside():
    """100 (code 1) is w1 of the tetrahedra xyz and xzy only: two triangles, on its edges to 000, 110, 101 (code differences) and
    111; the vertex between values 3 and -1 lies a quarter of the way from the outside end"""
    s = _cell([-1, 3, -1, -1, -1, -1, -1, -1])
    lo, h = np.array([10.0, 20.0, 30.0], np.float32), np.array([1.0, 2.0, 4.0], np.float32)
    tri, keys, skipped = MR.march(s, 0.0, lo, h)
    assert tri.shape[0] == 2 and skipped == 0
    # keys: the edge 000-100 starts at lin 0 with d = 100 -> 1; 100-110 starts at lin 1 with d = 010 -> 8 + 2; 100-101 -> 8 + 4;
    # 100-111 -> 8 + 6
    assert sorted(keys[0].tolist()) == [1, 10, 14] and sorted(keys[1].tolist()) == [1, 12, 14]
    where = {1: [10.25, 20.0, 30.0], 10: [11.0, 21.5, 30.0], 12: [11.0, 20.0, 33.0], 14: [11.0, 21.5, 33.0]}
    for p, k in zip(tri.reshape(-1, 3), keys.reshape(-1)):
        assert p.tolist() == where[int(k)]
    normals = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    centre_to_corner = np.array([11.0, 20.0, 30.0]) - tri.mean(axis=1)
    assert (np.einsum("ij,ij->i", normals, centre_to_corner) < 0).all()                   # facing away from the inside corner


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_corner_gives_nothing_and_one_skipped_cell(bad):
    s = _cell([1, -1, -1, bad, -1, -1, -1, -1])
    tri, keys, skipped = MR.march(s, 0.0, np.zeros(3), np.ones(3))
    assert tri.shape == (0, 3, 3) and keys.shape == (0, 3) and skipped == 1
    two = np.concatenate([_cell([1, -1, -1, -1, -1, -1, -1, -1]), _cell([-1, -1, -1, -1, -1, -1, -1, bad])[1:]], axis=0)
    tri, keys, skipped = MR.march(two, 0.0, np.zeros(3), np.ones(3))                      # [3,2,2]: the lower cell is whole
    assert tri.shape[0] == 6 and skipped == 1


def test_the_case_table_has_sixteen_entries_without_ambiguity():
    for t in range(6):
        assert MR.tet_codes(t)[0] == 0 and MR.tet_codes(t)[3] == 7
        for mask in range(16):
            n = bin(mask).count("1")
            assert len(MR.tet_case(t, mask)) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[n]
            # the complement crosses the same edges with the opposite winding
            a, b = MR.tet_case(t, mask), MR.tet_case(t, 15 - mask)
            assert sorted(tuple(sorted(e)) for tri in a for e in tri) == sorted(tuple(sorted(e)) for tri in b for e in tri)


def test_sphere_torus_and_noise_are_closed_oriented_surfaces():
    s, lo, h = MR.sphere(12)
    tri, keys, skipped = MR.march(s, 0.0, lo, h)
    paired, chi, volume = MR.invariants(tri, keys)
    assert paired and chi == 2 and volume > 0 and skipped == 0
    s, lo, h = MR.torus(20)
    paired, chi, volume = MR.invariants(*MR.march(s, 0.0, lo, h)[:2])
    assert paired and chi == 0 and volume > 0
    s, lo, h = MR.noise()
    tri, keys, _ = MR.march(s, 0.0, lo, h)
    paired, chi, volume = MR.invariants(tri, keys)
    assert paired and volume > 0 and tri.shape[0] > 1000                                  # 5.5 triangles per cell
    # the corner exactly at iso is inside, and its vertices lie ON it: triangles of zero area, which is why the winding is a table
    areas = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert (areas == 0).any()
    # welded: as many vertices as distinct keys, the faces index them and give the triangles back bit for bit
    vertices, faces = MR.weld(tri, keys)
    assert vertices.shape[0] == np.unique(keys).size and (vertices[faces].view(np.int32) == tri.view(np.int32)).all()


def test_sphere_volume_converges_with_second_order():
    """float64 restatement, ball of radius 0.7 in [-1, 1]^3: the enclosed volume is 3.4015 % below 4/3 pi r^3 on 12^3 lattice
    points and 0.7736 % below on 24^3 (h 2/11 and 2/23: 2.09 times finer), a ratio of 4.40 -- second order predicts
    (23/11)^2 = 4.37.  A first-order method would give 2.1; the assertion asks for more than 3."""
    errors = []
    for G in (12, 24):
        s, lo, h = MR.sphere(G)
        tri, keys, _ = MR.march(s.astype(np.float64), 0.0, lo, h, dtype=np.float64)
        paired, chi, volume = MR.invariants(tri, keys)
        assert paired and chi == 2
        errors.append(abs(volume / BALL - 1.0))
    print(f"relative volume errors {errors}, ratio {errors[0] / errors[1]}")
    assert errors[0] < 0.04 and errors[1] < 0.009
    assert errors[0] / errors[1] > 3.0


def test_fp32_and_fp64_restatements_agree_on_everything_but_rounding():
    s, lo, h = MR.sphere(12)
    t32, k32, _ = MR.march(s, 0.0, lo, h)
    t64, k64, _ = MR.march(s, 0.0, lo, h, dtype=np.float64)
    assert t32.dtype == np.float32 and t64.dtype == np.float64 and (k32 == k64).all()
    assert np.abs(t32 - t64).max() < 4 * np.finfo(np.float32).eps                         # positions of magnitude <= 1


def test_mesh_ply_writer(tmp_path):
    from nerf_sampling_amd.nerf_utils import write_mesh_ply

    v = np.array([[0.0, 1.0, -2.0], [3.5, np.nan, 1e-3], [7.0, 8.0, 9.0], [1.0, 1.0, 1.0]], dtype=np.float32)
    f = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int64)
    rgb = np.array([[0.0, 0.5, 1.0], [-0.25, 1.5, 0.999], [0.1, 0.2, 0.8], [1.0, 1.0, 1.0]], dtype=np.float32)
    path = str(tmp_path / "m.ply")
    write_mesh_ply(path, v, f, rgb)
    raw = open(path, "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 2\n"
              "property list uchar int vertex_indices\nend_header\n").encode("ascii")
    assert raw.startswith(header) and len(raw) == len(header) + 4 * 15 + 2 * 13
    body = raw[len(header):]
    for i in range(4):
        assert body[15 * i:15 * i + 12] == v[i].astype("<f4").tobytes()
    assert list(body[12:15]) == [0, 127, 255] and list(body[27:30]) == [0, 255, 254] and list(body[42:45]) == [25, 51, 204]
    faces = body[60:]
    assert faces[:13] == b"\x03" + np.array([0, 1, 2], "<i4").tobytes() and faces[13:] == b"\x03" + np.array([2, 1, 3], "<i4").tobytes()
    write_mesh_ply(path, v, f)                                                            # no colours: no colour properties
    plain = open(path, "rb").read()
    assert b"red" not in plain and len(plain) == len(header) - len("property uchar red\nproperty uchar green\nproperty uchar blue\n") + 4 * 12 + 26
    write_mesh_ply(path, v[:0], f[:0], rgb[:0])
    assert open(path, "rb").read() == header.replace(b"vertex 4", b"vertex 0").replace(b"face 2", b"face 0")
    with pytest.raises(ValueError):
        write_mesh_ply(path, v, f, rgb[:3])
    with pytest.raises(ValueError):
        write_mesh_ply(path, v[:3], f)                                                    # a face names vertex 3


def test_new_parameters_default_off():
    from nerf_sampling_amd import nerf_utils, ops
    from nerf_sampling_amd.trainers import Trainer

    p = inspect.signature(Trainer.__init__).parameters
    assert p["device_mesh"].default is False and p["mesh_resolution"].default == 256
    assert p["mesh_threshold"].default == 50.0 and p["mesh_bound"].default == 1.5
    assert p["device_cloud"].default is False and p["device_eval"].default is False
    s = inspect.signature(nerf_utils.scene_mesh).parameters
    assert list(s) == ["network", "bound", "resolution", "threshold", "colours", "savedir", "capacity", "return_grid"]
    assert [s[k].default for k in list(s)[1:]] == [1.5, 256, 50.0, True, None, None, False]
    assert list(inspect.signature(nerf_utils.field_density_grid).parameters) == ["network", "lo", "hi", "resolution", "chunk"]
    assert list(inspect.signature(nerf_utils.write_mesh_ply).parameters) == ["path", "vertices", "faces", "rgb"]
    m = inspect.signature(ops.mesh_extract).parameters
    assert list(m) == ["sigma", "iso", "lo", "h", "capacity", "workspace"] and m["capacity"].default is None
    assert list(inspect.signature(ops.mesh_weld).parameters) == ["triangles", "keys"]
    with pytest.raises(ValueError):
        Trainer(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="", device_mesh=True,
                mesh_resolution=1)
    lo, h, G = nerf_utils.mesh_lattice(-1.5, 1.5, 256)
    assert G == (256, 256, 256) and lo == [-1.5] * 3 and h == [float(np.float32(3.0 / 255))] * 3
    assert nerf_utils.mesh_lattice((0, 0, 0), (1, 2, 3), (2, 3, 4))[1] == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError):
        nerf_utils.mesh_lattice(1.0, 1.0, 8)


def test_render_cli_has_the_four_flags():
    from nerf_sampling_amd.experiments.render import main

    opts = {o.name: o for o in main.params}
    assert opts["device_mesh"].is_flag and opts["device_mesh"].default is False and "--device-mesh" in opts["device_mesh"].opts
    assert opts["mesh_resolution"].default == 256 and opts["mesh_threshold"].default == 50.0 and opts["mesh_bound"].default == 1.5
    assert "lower it" in opts["mesh_threshold"].help and "raise it" in opts["mesh_threshold"].help


def test_argument_checks_without_a_gpu():
    """every refusal comes before any HIP call: -1 (NS_E_INVALID) on a machine without a GPU, the pointers never dereferenced"""
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    p = C.c_void_p
    sigma, tri, keys, count, ws = p(0x1000), p(0x2000), p(0x3000), p(0x4000), p(0x5000)

    def call(sigma=sigma, stride=1, G=(4, 5, 6), iso=0.5, lo=(0.0, 0.0, 0.0), h=(1.0, 1.0, 1.0), tri=tri, keys=keys, capacity=7,
             count=count, ws=ws):
        return lib.ns_mesh_extract(sigma, stride, *G, iso, *lo, *h, tri, keys, capacity, count, ws, None)

    bad = [dict(G=(1, 5, 6)), dict(G=(4, 1, 6)), dict(G=(4, 5, 1)), dict(G=(0, 0, 0)), dict(G=(-4, 5, 6)),
           dict(G=(2048, 1024, 1024)), dict(G=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)),
           dict(stride=-1), dict(capacity=-1), dict(tri=None), dict(keys=None), dict(count=None), dict(sigma=None),
           dict(ws=None), dict(count=p(0x4004)), dict(keys=p(0x3004)), dict(ws=p(0x5004)),
           dict(iso=float("nan")), dict(iso=float("inf")), dict(lo=(0.0, float("nan"), 0.0)), dict(lo=(float("-inf"), 0.0, 0.0)),
           dict(h=(1.0, 1.0, float("inf"))), dict(h=(1.0, float("nan"), 1.0)), dict(h=(0.0, 1.0, 1.0)), dict(h=(1.0, 1.0, -1.0))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"ns_mesh_extract" in lib.ns_last_error()
    S = _share()
    assert lib.ns_mesh_workspace_bytes(2, 2, 2) == 256
    assert lib.ns_mesh_workspace_bytes(16 * S + 1, 2, 2) == 256 and lib.ns_mesh_workspace_bytes(16 * S + 2, 2, 2) == 512
    for G in ((1, 2, 2), (2, 2, 0), (2048, 1024, 1024), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.ns_mesh_workspace_bytes(*G) == 0, G
    assert lib.ns_mesh_workspace_bytes(2047, 1024, 1024) > 0


def _share():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "nerf_sampling_hip.h")).read()
    return int(re.search(r"#define NS_MESH_SHARE (\d+)", text).group(1))
