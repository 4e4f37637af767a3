"""The host side of the mesh normals (not gpu): the numpy restatement tests/test_gpu_mesh_normals.py measures ns_mesh_normals
against (tests/mesh_normals_reference.py) -- judged by what neither it nor the kernel defines: the analytic normals of a quadratic
field and of a ball, and the geometric normals of the triangles around a vertex --, the key decoding on cases named one by one,
the entry's argument checks through the library on a machine without a GPU, the PLY writer and the new switches."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import mesh_normals_reference as NR
import mesh_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float32).eps)


def _surface(sigma, lo, h, iso=0.0):
    """-> (vertices [V,3] float32, faces, keys [V] ascending, normals [V,3], n_degenerate) of the restatements"""
    tri, keys, _ = MR.march(sigma, iso, lo, h)
    vertices, faces = MR.weld(tri, keys)
    unique = np.unique(keys)
    normals, n_degenerate, n_invalid, _ = NR.normals(sigma, iso, h, unique)
    assert n_invalid == 0 and normals.dtype == np.float32 and normals.shape == (unique.size, 3)
    return vertices, faces, unique, normals, n_degenerate


def _angles(normals, want):
    cos = np.einsum("ij,ij->i", normals.astype(np.float64), want)
    return np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))


def test_quadratic_field_gives_the_analytic_normal():
    """sigma = 0.49 - |p|^2: central differences are exact for a quadratic and its gradient -2 p is linear along an edge, so the
    definition gives p / |p| at the vertex p up to fp32 rounding: 4 eps, the margin of
    test_fp32_and_fp64_restatements_agree_on_everything_but_rounding.  The surface stays off the lattice boundary (|p| = 0.7), so
    every stencil it reads is central."""
    lo, h, ax = MR.axes(16)
    Z, Y, X = np.meshgrid(ax, ax, ax, indexing="ij")
    sigma = (0.49 - (X * X + Y * Y + Z * Z)).astype(np.float32)
    vertices, _, keys, normals, n_degenerate = _surface(sigma, lo, h)
    p = vertices.astype(np.float64)
    want = p / np.linalg.norm(p, axis=1, keepdims=True)
    worst = float(np.abs(normals - want).max())
    print(f"quadratic: {keys.size} vertices, {n_degenerate} degenerate, max |n - p/|p|| = {worst:.3e} ({worst / EPS:.2f} eps)")
    assert keys.size > 1000 and n_degenerate == 0
    assert worst < 4 * EPS
    assert np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1.0).max() < 2 * EPS


def test_sphere_normals_converge_with_second_order():
    """MR.sphere, sigma = 0.7 - |p|: the largest angle between the normal and p / |p| falls from G = 12 to G = 24 (h 2.09 times
    finer) by second order's (23/11)^2 = 4.4; a first-order method would give 2.1, the assertion asks for more than 3"""
    worst = []
    for G in (12, 24):
        sigma, lo, h = MR.sphere(G)
        vertices, _, keys, normals, n_degenerate = _surface(sigma, lo, h)
        p = vertices.astype(np.float64)
        worst.append(float(_angles(normals, p / np.linalg.norm(p, axis=1, keepdims=True)).max()))
        assert n_degenerate == 0
    print(f"sphere: largest angles {worst} degrees, ratio {worst[0] / worst[1]:.2f}")
    assert worst[0] < 2.0 and worst[0] / worst[1] >= 3.0


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_normals_face_the_way_the_triangles_do(name):
    """the dot product with the area-weighted normal of the triangles around the vertex (the winding's side) is positive at every
    vertex: > 0.9 (the restatement stands at 0.994 on the ball and 0.953 on the torus)"""
    sigma, lo, h = MR.sphere(24) if name == "sphere" else MR.torus(20)
    vertices, faces, keys, normals, n_degenerate = _surface(sigma, lo, h)
    geometric = NR.geometric_normals(vertices, faces)
    dots = np.einsum("ij,ij->i", normals.astype(np.float64), geometric)
    print(f"{name}: {keys.size} vertices, smallest dot {dots.min():.4f}")
    assert n_degenerate == 0 and dots.min() > 0.9


def test_geometric_normals_on_a_hand_case():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]])                     # z = 0 facing +z (area 1/2), x = 0 facing +x (area 1/2)
    n = NR.geometric_normals(v, f)
    r = np.sqrt(0.5)
    assert np.allclose(n, [[r, 0, r], [0, 0, 1], [r, 0, r], [1, 0, 0], [0, 0, 0]], atol=1e-15)


DIMS = (7, 6, 9)


def test_decode_every_code_at_an_interior_point():
    a = (3, 2, 4)
    keys = NR.lin(*a, DIMS) * 8 + np.arange(1, 8)
    valid, pa, pb = NR.decode(keys, DIMS)
    assert valid.all() and (pa == np.array(a)).all()
    assert (pb - pa).tolist() == [[1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1]]
    # the first and the last lattice edge there is
    valid, pa, pb = NR.decode([1, (NR.lin(5, 4, 7, DIMS)) * 8 + 7], DIMS)
    assert valid.all() and pa.tolist() == [[0, 0, 0], [5, 4, 7]] and pb.tolist() == [[1, 0, 0], [6, 5, 8]]


def test_decode_refuses_what_names_no_edge():
    bad = NR.invalid_keys(DIMS)
    valid, _, _ = NR.decode(bad, DIMS)
    assert bad.size == 21 and not valid.any()
    every = NR.all_edge_keys(DIMS)
    # per code, the points whose far end lies inside: (Gx - dx) (Gy - dy) (Gz - dz)
    assert every.size == sum((7 - (c & 1)) * (6 - ((c >> 1) & 1)) * (9 - (c >> 2)) for c in range(1, 8))
    assert NR.decode(every, DIMS)[0].all() and not np.isin(bad, every).any()
    sigma = np.random.default_rng(1).standard_normal((9, 6, 7)).astype(np.float32)
    mixed = np.concatenate([every[:5], bad, every[5:9]])
    normals, n_degenerate, n_invalid, _ = NR.normals(sigma, 0.1, (1.0, 1.0, 1.0), mixed)
    assert n_invalid == bad.size and n_degenerate == 0
    assert (normals[5:5 + bad.size] == 0).all() and (np.abs(normals[:5]).max(axis=1) > 0).all()
    alone = NR.normals(sigma, 0.1, (1.0, 1.0, 1.0), np.concatenate([every[:5], every[5:9]]))[0]
    assert (np.delete(normals, np.s_[5:5 + bad.size], axis=0).view(np.int32) == alone.view(np.int32)).all()


def test_degenerate_vertices_of_the_restatement():
    """s_a == s_b; the isolated point s_a = iso among zeros (tt = -0, g_a = 0: a zero gradient); NaN and inf in a stencil
    neighbour that is no endpoint; keys shaped [n,3] keep their shape"""
    s = np.zeros((5, 5, 5), dtype=np.float32)
    s[2, 2, 2] = 1.0
    dims = (5, 5, 5)
    at = NR.lin(2, 2, 2, dims) * 8
    n, deg, inv, length = NR.normals(s, 1.0, (1, 1, 1), np.array([at + 1, at + 2, at + 4, at + 7]))
    assert (deg, inv) == (4, 0) and (n == 0).all() and (length == 0).all()
    flat = NR.lin(0, 0, 0, dims) * 8 + 1                                                  # 0 and 0: tt = 1 / 0
    assert NR.normals(s, 1.0, (1, 1, 1), np.array([flat]))[1:3] == (1, 0)
    n, deg, inv, _ = NR.normals(s, 0.5, (1, 1, 1), np.array([[at + 1, at + 2, at + 4]]))
    assert n.shape == (1, 3, 3) and (deg, inv) == (0, 0)
    # the edge from the peak along +x: the gradient there points down the edge (and, by the far end's stencil, nowhere else)
    assert n[0, 0].tolist() == [1.0, 0.0, 0.0] and n[0, 1].tolist() == [0.0, 1.0, 0.0]
    for bad in (np.nan, np.inf, -np.inf):
        t = s.copy()
        t[2, 3, 3] = bad                                                                  # the +y neighbour of b = (3, 2, 2)
        n, deg, inv, _ = NR.normals(t, 0.5, (1, 1, 1), np.array([at + 1, at + 4]))
        assert (deg, inv) == (1, 0) and (n[0] == 0).all() and n[1].tolist() == [0.0, 0.0, 1.0]


def test_argument_checks_without_a_gpu():
    """every refusal comes before any HIP call: -1 (NS_E_INVALID) on a machine without a GPU, the pointers never dereferenced"""
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    p = C.c_void_p
    sigma, keys, normals, count, ws = p(0x1000), p(0x2000), p(0x3000), p(0x4000), p(0x5000)
    nan, inf = float("nan"), float("inf")

    def call(sigma=sigma, stride=1, G=(4, 4, 4), iso=0.0, h=(1.0, 1.0, 1.0), keys=keys, V=8, normals=normals, count=count, ws=ws):
        return lib.ns_mesh_normals(sigma, stride, *G, iso, *h, keys, V, normals, count, ws, None)

    bad = [dict(G=(1, 4, 4)), dict(G=(4, 1, 4)), dict(G=(4, 4, 1)), dict(G=(0, 4, 4)), dict(G=(4, -3, 4)),
           dict(G=(2048, 1024, 1024)), dict(G=(2 ** 31 - 1, 2 ** 31 - 1, 2)), dict(stride=-1), dict(stride=-2 ** 63),
           dict(iso=nan), dict(iso=inf), dict(iso=-inf),
           dict(h=(nan, 1, 1)), dict(h=(1, inf, 1)), dict(h=(1, 1, -inf)), dict(h=(0.0, 1, 1)), dict(h=(1, -0.0, 1)),
           dict(h=(1, 1, -1.0)),
           dict(V=-1), dict(V=-2 ** 63), dict(V=2 ** 31), dict(V=2 ** 62),
           dict(count=None), dict(count=None, V=0), dict(sigma=None), dict(keys=None), dict(normals=None), dict(ws=None),
           dict(keys=p(0x2004)), dict(count=p(0x4004)), dict(ws=p(0x5004)), dict(keys=p(0x2004), V=0),
           dict(normals=p(0x3001)), dict(normals=p(0x3002)), dict(normals=p(0x3003))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"ns_mesh_normals" in lib.ns_last_error()
    share = int(re.search(r"#define NS_MESH_NORMALS_SHARE (\d+)",
                          open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()).group(1))
    size = lib.ns_mesh_normals_workspace_bytes
    assert share == 1024
    # two int64 per share, in whole 256-byte lines; no key, no share
    assert [size(V) for V in (0, 1, share, share + 1)] == [0, 256, 256, 256]
    assert size(16 * share) == 256 and size(16 * share + 1) == 512 and size(2 ** 31 - 1) == 2 ** 21 * 16
    for V in (-1, -2 ** 63, 2 ** 31, 2 ** 62):
        assert size(V) == 0, V


def test_ops_mesh_normals_refuses_before_any_launch():
    import torch

    from nerf_sampling_amd import ops

    sigma = torch.zeros((4, 4, 4))
    for bad in (sigma, sigma.numpy(), None):                                              # not on the device
        with pytest.raises(ValueError):
            ops.mesh_normals(bad, 0.0, (1, 1, 1), torch.zeros(3, dtype=torch.int64))
    p = inspect.signature(ops.mesh_normals).parameters
    assert list(p) == ["sigma", "iso", "h", "keys", "workspace"] and p["workspace"].default is None
    assert list(inspect.signature(ops.mesh_normals_workspace_bytes).parameters) == ["n_vertices"]
    assert ops.mesh_normals_workspace_bytes(1) == 256 and ops.mesh_normals_workspace_bytes(-1) == 0


def test_ply_writer_with_normals(tmp_path):
    from nerf_sampling_amd.nerf_utils import write_mesh_ply, write_mesh_ply_normals

    v = np.array([[0.0, 1.0, -2.0], [3.5, np.nan, 1e-3], [7.0, 8.0, 9.0], [1.0, 1.0, 1.0]], dtype=np.float32)
    f = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int64)
    rgb = np.array([[0.0, 0.5, 1.0], [-0.25, 1.5, 0.999], [0.1, 0.2, 0.8], [1.0, 1.0, 1.0]], dtype=np.float32)
    n = np.array([[0.0, 0.0, 1.0], [0.6, -0.8, 0.0], [0.0, 0.0, 0.0], [-1.0, 0.0, -0.0]], dtype=np.float32)
    path, other = str(tmp_path / "m.ply"), str(tmp_path / "o.ply")
    xyz = "property float x\nproperty float y\nproperty float z\n"
    nxyz = "property float nx\nproperty float ny\nproperty float nz\n"
    colour = "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head = lambda *props: ("ply\nformat binary_little_endian 1.0\nelement vertex 4\n" + "".join(props)         # noqa: E731
                           + "element face 2\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    faces = b"\x03" + np.array([0, 1, 2], "<i4").tobytes() + b"\x03" + np.array([2, 1, 3], "<i4").tobytes()
    to8b = [[0, 127, 255], [0, 255, 254], [25, 51, 204], [255, 255, 255]]
    # normals and colours: x y z nx ny nz red green blue, 27 bytes per vertex
    write_mesh_ply_normals(path, v, f, rgb=rgb, normals=n)
    raw = open(path, "rb").read()
    assert raw == head(xyz, nxyz, colour) + b"".join(v[i].astype("<f4").tobytes() + n[i].astype("<f4").tobytes() + bytes(to8b[i])
                                                     for i in range(4)) + faces
    # normals alone: 24 bytes per vertex
    write_mesh_ply_normals(path, v, f, normals=n)
    assert open(path, "rb").read() == head(xyz, nxyz) + b"".join(v[i].astype("<f4").tobytes() + n[i].astype("<f4").tobytes()
                                                                 for i in range(4)) + faces
    # without normals it is write_mesh_ply's file, whose bytes are what they always were
    for colours in (rgb, None):
        write_mesh_ply_normals(path, v, f, rgb=colours)
        write_mesh_ply(other, v, f, colours)
        assert open(path, "rb").read() == open(other, "rb").read()
    write_mesh_ply(other, v, f, rgb)
    assert open(other, "rb").read() == head(xyz, colour) + b"".join(v[i].astype("<f4").tobytes() + bytes(to8b[i])
                                                                    for i in range(4)) + faces
    write_mesh_ply(other, v, f)
    assert open(other, "rb").read() == head(xyz) + v.astype("<f4").tobytes() + faces
    write_mesh_ply_normals(path, v[:0], f[:0], rgb[:0], n[:0])
    assert open(path, "rb").read() == head(xyz, nxyz, colour).replace(b"vertex 4", b"vertex 0").replace(b"face 2", b"face 0")
    with pytest.raises(ValueError):
        write_mesh_ply_normals(path, v, f, rgb, n[:3])                                    # three normals for four vertices
    with pytest.raises(ValueError):
        write_mesh_ply_normals(path, v, f, rgb[:3], n)
    p = inspect.signature(write_mesh_ply_normals).parameters
    assert list(p) == ["path", "vertices", "faces", "rgb", "normals"] and p["rgb"].default is None and p["normals"].default is None
    assert list(inspect.signature(write_mesh_ply).parameters) == ["path", "vertices", "faces", "rgb"]


def test_new_switches_default_off_and_reject_bad_values():
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.experiments.render import main
    from nerf_sampling_amd.trainers import Trainer

    p = inspect.signature(Trainer.__init__).parameters
    assert p["mesh_normals"].default is False and p["mesh_colour_view"].default == "centre"
    filtered = inspect.signature(nerf_utils.scene_mesh_filtered).parameters
    shaded = inspect.signature(nerf_utils.scene_mesh_shaded).parameters
    assert list(shaded) == list(filtered) + ["normals", "colour_view"]
    assert all(shaded[k].default == v.default for k, v in filtered.items())
    assert shaded["normals"].default is True and shaded["colour_view"].default == "centre"
    assert "normals" not in filtered and "colour_view" not in filtered
    assert list(inspect.signature(nerf_utils.mesh_filter).parameters) == ["vertices", "faces", "rgb", "min_component_triangles",
                                                                         "keep_largest"]
    base = dict(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="")
    t = Trainer(**base)
    assert (t.mesh_normals, t.mesh_colour_view) == (False, "centre")
    t = Trainer(**base, device_mesh=True, mesh_normals=True, mesh_colour_view="normal")
    assert (t.mesh_normals, t.mesh_colour_view) == (True, "normal")
    for kw in (dict(mesh_colour_view="normal"), dict(mesh_normals=True, mesh_colour_view="center"),
               dict(mesh_colour_view=None), dict(mesh_normals=1), dict(mesh_normals="yes")):
        with pytest.raises(ValueError):
            Trainer(**base, **kw)
    # scene_mesh_shaded refuses its own two before it touches the network
    for kw in (dict(normals=False, colour_view="normal"), dict(colour_view="outward")):
        with pytest.raises(ValueError):
            nerf_utils.scene_mesh_shaded(None, resolution=4, **kw)
    opts = {o.name: o for o in main.params}
    assert opts["mesh_normals"].is_flag and opts["mesh_normals"].default is False and "--mesh-normals" in opts["mesh_normals"].opts
    view = opts["mesh_colour_view"]
    assert view.default == "centre" and "--mesh-colour-view" in view.opts and list(view.type.choices) == ["centre", "normal"]
    with pytest.raises(Exception):
        view.type.convert("center", view, None)
