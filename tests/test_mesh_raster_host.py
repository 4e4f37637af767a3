"""The host side of the mesh rasteriser (not gpu): the numpy restatement tests/test_gpu_mesh_raster.py measures ns_mesh_raster
against (tests/mesh_raster_reference.py) -- judged by what neither it nor the kernel defines: frames worked out on paper, the
tie rule's exactly-once property on quads and fans, the exact ray-plane depth of a tilted quad, and the two-faces-per-pixel
property of a closed surface, which fixes the front-face sign --, the entry's argument checks through the library on a machine
without a GPU, and the switches of the Python layers."""

import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import mesh_raster_reference as RR
import mesh_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0)               # with RR.IDENTITY: screen (x, y) at depth z is p = (x z, -y z, -z)


def _raster(xy, z, faces, H, W, attr=None, **kw):
    return RR.rasterize(RR.screen_vertices(xy, z), faces, RR.IDENTITY, H=H, W=W, near=0.5, attr=attr, **UNIT, **kw)


def test_a_right_triangle_worked_out_on_paper():
    """Screen vertices (0,0), (4,0), (0,4) at depth 2: p = (x z, -y z, -z) = (0,0,-2), (8,0,-2), (0,-8,-2), and the projection
    gives them back exactly (q_0 / z = 8 / 2).  X, Y = 256 x, 256 y; area2 = E_01(V_2) = (1024)(1024) - 0 > 0, so the frame's
    orientation is the positive one and this winding is a BACK face (front is area2 < 0).  Edges in that orientation:
    0 -> 1 has d = (+, 0): a top edge, its centres (i, 0) are covered; 1 -> 2 has d = (-, +): neither top nor left, the centres
    with i + j = 4 are not; 2 -> 0 has d = (0, -): a left edge, its centres (0, j) are.  Covered: i, j >= 0, i + j < 4 -- ten
    pixels, all at depth exactly 2, the vertices (4, 0) and (0, 4) not among them."""
    tri = [[0, 1, 2]]
    got = _raster([(0, 0), (4, 0), (0, 4)], 2.0, tri, 6, 7)
    want = np.array([[i + j < 4 for i in range(7)] for j in range(6)])
    assert got["counts"].tolist() == [0, 0, 0, 10]
    assert ((got["tri"] == 0).reshape(6, 7) == want).all() and (got["tri"][~want.reshape(-1)] == -1).all()
    assert (got["depth"].reshape(6, 7)[want] == 2.0).all() and (got["depth"].reshape(6, 7)[~want] == 0.0).all()
    assert (got["n_front"] == 0).all()
    # the other winding is the same set of pixels (the rule looks at the edge and the side, not the winding), facing the camera
    other = _raster([(0, 0), (4, 0), (0, 4)], 2.0, [[0, 2, 1]], 6, 7)
    assert (other["tri"] == got["tri"]).all() and (other["n_front"] == other["n_cover"]).all()
    assert _raster([(0, 0), (4, 0), (0, 4)], 2.0, tri, 6, 7, cull=1)["counts"].tolist() == [0, 0, 0, 0]     # back face culled
    assert _raster([(0, 0), (4, 0), (0, 4)], 2.0, tri, 6, 7, cull=2)["counts"].tolist() == [0, 0, 0, 10]


def test_perspective_correct_depth_and_colour_on_paper():
    """Screen vertices (0,0), (4,0), (0,4) at depths 1, 2, 4, colours red, green, blue.  At pixel (1, 1) the screen barycentrics
    are b = (1/2, 1/4, 1/4) (w_k / area2: b_1 = x / 4, b_2 = y / 4).  1 / z is affine on the screen:
    1 / z = 1/2 + 1/8 + 1/16 = 11/16, z = 16/11; a colour channel is (b_k / z_k) / (1 / z): (8/11, 2/11, 1/11)."""
    attr = np.eye(3, dtype=np.float32)
    got = _raster([(0, 0), (4, 0), (0, 4)], [1.0, 2.0, 4.0], [[0, 1, 2]], 5, 5, attr=attr, background=0.25)
    at = 1 * 5 + 1
    assert got["depth"][at] == np.float32(16.0 / 11.0)
    assert got["rgb"][at].tolist() == [np.float32(8.0 / 11.0), np.float32(2.0 / 11.0), np.float32(1.0 / 11.0)]
    assert got["depth"][0] == 1.0 and got["rgb"][0].tolist() == [1.0, 0.0, 0.0]                             # vertex 0 itself
    assert got["tri"][4 * 5 + 4] == -1 and got["rgb"][4 * 5 + 4].tolist() == [0.25] * 3 and got["depth"][4 * 5 + 4] == 0.0


def _windings(tri):
    a, b, c = tri
    return [(a, b, c), (b, c, a), (c, a, b), (a, c, b), (c, b, a), (b, a, c)]


@pytest.mark.parametrize("corner", [0, 1])
def test_split_quad_covers_every_pixel_once(corner):
    """the square (1,1) .. (5,5), corners on pixel centres, split along either diagonal -- both pass through pixel centres --:
    for every winding of either triangle each centre with 1 <= i, j < 5 is covered exactly once (the top and left edges belong
    to the square, the bottom and right ones do not), and the diagonal's centres by exactly one of the two triangles"""
    xy = [(1, 1), (5, 1), (5, 5), (1, 5)]
    pair = [(0, 1, 2), (0, 2, 3)] if corner == 0 else [(1, 2, 3), (1, 3, 0)]
    want = np.zeros((7, 8), dtype=np.int32)
    want[1:5, 1:5] = 1
    for first, second in itertools.product(_windings(pair[0]), _windings(pair[1])):
        got = _raster(xy, 2.0, [first, second], 7, 8)
        assert (got["n_cover"].reshape(7, 8) == want).all(), (first, second)
        assert got["counts"].tolist() == [0, 0, 0, 16]


def _inside_after_shift(poly, i, j):
    """whether the point (i + eps, j + eps^2) lies strictly inside the convex polygon ``poly`` (integer corners, either
    orientation) -- exact, with eps = 2^-10 in integers scaled by 2^20: the statement of the top-left rule"""
    px, py = (i << 20) + (1 << 10), (j << 20) + 1
    sides = []
    for (ax, ay), (bx, by) in zip(poly, poly[1:] + poly[:1]):
        sides.append(RR.edge(ax << 20, ay << 20, bx << 20, by << 20, px, py))
    return all(s > 0 for s in sides) or all(s < 0 for s in sides)


def test_fan_covers_its_centre_once():
    """a fan of six triangles around the vertex (3, 3), a pixel centre, whose spokes to (3, 0) and (3, 6) run through pixel
    centres: whatever the windings, no centre is covered twice, the fan's centre and the spokes' centres exactly once, and the
    covered set is the hexagon's as the rule states it (the centres that lie inside after a shift by (eps, eps^2))"""
    ring = [(0, 1), (3, 0), (6, 1), (6, 5), (3, 6), (0, 5)]
    xy = [(3, 3)] + ring
    want = np.array([[_inside_after_shift(ring, i, j) for i in range(8)] for j in range(8)], dtype=np.int32)
    assert want[3, 3] == 1 and want[1, 3] == 1 and want[5, 3] == 1 and want.sum() > 20
    rng = np.random.default_rng(5)
    for trial in range(16):
        faces = []
        for k in range(6):
            tri = (0, 1 + k, 1 + (k + 1) % 6)
            faces.append(_windings(tri)[int(rng.integers(6))] if trial else tri)
        got = _raster(xy, 2.0, faces, 8, 8)
        assert (got["n_cover"].reshape(8, 8) == want).all(), faces


def _plane_depth(c2w, fx, fy, cx, cy, tri_xyz, i, j):
    """z* of the ray through the (real-valued) pixel (i, j) and the plane of the triangle, in float64: the ray is
    t + z d, d = R ((i - cx) / fx, -(j - cy) / fy, -1)"""
    c2w = np.asarray(c2w, dtype=np.float64)
    r, t = c2w[:, :3], c2w[:, 3]
    a, b, c = (np.asarray(v, dtype=np.float64) for v in tri_xyz)
    n = np.cross(b - a, c - a)
    cam = np.stack([(i - cx) / fx, -(j - cy) / fy, -np.ones_like(i)], axis=-1)
    d = cam @ r.T
    return (n @ (a - t)) / (d @ n)


@pytest.mark.parametrize("eye", [(1.5, -3.0, 1.0), (-0.5, -2.0, 2.5)])
def test_tilted_quad_against_the_exact_ray_plane_depth(eye):
    """A tilted planar quad on a 48 x 40 frame.  Snapping moves a vertex by at most 2^-9 px per axis, so a point of the moved
    triangle corresponds to a point of the original at most that far away; the bound per pixel is the largest
    |z*(i +- 2^-8, j +- 2^-8) - z*(i, j)| (twice the snapping step: the spare half absorbs the fp32 rounding of the projected
    coordinates) plus 4 fp32 ulps of z*."""
    H, W, f = 40, 48, 52.0
    cam = dict(fx=f, fy=f, cx=0.5 * W, cy=0.5 * H)
    c2w = RR.look_at(eye)
    quad = np.array([[-0.8, 0.3, -0.6], [0.7, -0.4, -0.5], [0.9, 0.5, 0.7], [-0.6, 1.2, 0.6]], dtype=np.float32)
    quad[3] = quad[0] + (quad[2] - quad[1])                                   # a parallelogram: planar up to fp32 rounding
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    got = RR.rasterize(quad, faces, c2w, H=H, W=W, near=0.5, **cam)
    assert got["counts"][:3].tolist() == [0, 0, 0] and got["counts"][3] > 300
    at = np.nonzero(got["tri"] >= 0)[0]
    i, j = (at % W).astype(np.float64), (at // W).astype(np.float64)
    worst = 0.0
    for f_ in range(2):
        sel = got["tri"][at] == f_
        tri_xyz = quad[faces[f_]]
        z0 = _plane_depth(c2w, **cam, tri_xyz=tri_xyz, i=i[sel], j=j[sel])
        step = 2.0 ** -8
        bound = np.zeros_like(z0)
        for di, dj in itertools.product((-step, step), repeat=2):
            bound = np.maximum(bound, np.abs(_plane_depth(c2w, **cam, tri_xyz=tri_xyz, i=i[sel] + di, j=j[sel] + dj) - z0))
        bound += 4 * np.spacing(z0.astype(np.float32)).astype(np.float64)
        err = np.abs(got["depth"][at][sel].astype(np.float64) - z0)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), float((err / bound).max())
    print(f"eye {eye}: {at.size} covered pixels, largest |depth - z*| / bound = {worst:.3f}")
    # the float64 projection of the same vertices lands within 2^-9 px of the snapped float32 one, rounding included
    x64, y64, _ = RR.project(quad, c2w, dtype=np.float64, **cam)
    assert np.abs(got["X"] / 256.0 - x64).max() <= 2.0 ** -9 + 1e-4 and np.abs(got["Y"] / 256.0 - y64).max() <= 2.0 ** -9 + 1e-4


_ball = {}


def ball(G=24):
    """(vertices, faces) of the extracted ball, welded; marched once"""
    if G not in _ball:
        sigma, lo, h = MR.sphere(G)
        tri, keys, _ = MR.march(sigma, 0.0, lo, h)
        v, f = MR.weld(tri, keys)
        v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int64)
        v.setflags(write=False)
        f.setflags(write=False)
        _ball[G] = (v, f)
    return _ball[G]


BALL_CAMERA = dict(H=40, W=48, fx=60.0, fy=60.0, cx=24.0, cy=20.0, near=0.5)


def test_ball_has_two_faces_per_pixel_and_the_front_one_is_nearer():
    """The extracted ball is closed and faces outwards.  Seen from outside every pixel centre inside the silhouette is covered by
    exactly two faces, one of each facing, and the front one -- area2 < 0 for ns_mesh_extract's outward winding, x to the
    right and y down -- is the nearer: cull = 1 (back faces dropped) leaves the frame as it is, cull = 2 shows the far side."""
    v, f = ball()
    c2w = RR.look_at((2.0, -2.5, 1.5))
    n_cover, n_front = RR.cover_counts(v, f, c2w, **BALL_CAMERA)
    inside = n_cover > 0
    assert 400 < inside.sum() < 48 * 40 and (n_cover[inside] == 2).all() and (n_front[inside] == 1).all()
    both = RR.rasterize(v, f, c2w, **BALL_CAMERA)
    front = RR.rasterize(v, f, c2w, cull=1, **BALL_CAMERA)
    back = RR.rasterize(v, f, c2w, cull=2, **BALL_CAMERA)
    # nothing clipped or invalid; the marched ball has slivers of zero area (lattice corners near the iso value), which cover nothing
    assert both["counts"][0] == 0 and both["counts"][2] == 0 and both["counts"][1] < f.shape[0] // 10
    assert (front["tri"] == both["tri"]).all() and (front["depth"] == both["depth"]).all()
    hit = both["tri"] >= 0
    assert ((back["tri"] >= 0) == hit).all() and (back["depth"][hit] > both["depth"][hit]).all()
    # the depth is the distance along the ray's unnormalised direction: the ball of radius 0.7 seen from |eye| = 3.84
    centre = 20 * 48 + 24
    assert abs(float(both["depth"][centre]) - (np.linalg.norm([2.0, -2.5, 1.5]) - 0.7)) < 0.02


def test_argument_checks_without_a_gpu():
    """every refusal comes before any HIP call: -1 (NS_E_INVALID) on a machine without a GPU, the pointers never dereferenced"""
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    p = C.c_void_p
    good_c2w = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    nan, inf = float("nan"), float("inf")

    def c2w_with(k, value):
        m = (C.c_float * 12)(*good_c2w)
        m[k] = value
        return m

    base = dict(v=p(0x1000), V=8, f=p(0x2000), F=4, attr=p(0x3000), c2w=good_c2w, fx=10.0, fy=10.0, cx=4.0, cy=4.0, H=8, W=8,
                near=0.5, cull=0, bg=0.0, depth=p(0x4000), tri=p(0x5000), rgb=p(0x6000), count=p(0x7000), ws=p(0x8000))

    def call(**kw):
        a = dict(base, **kw)
        return lib.ns_mesh_raster(a["v"], a["V"], a["f"], a["F"], a["attr"], a["c2w"], a["fx"], a["fy"], a["cx"], a["cy"], a["H"],
                                  a["W"], a["near"], a["cull"], a["bg"], a["depth"], a["tri"], a["rgb"], a["count"], a["ws"], None)

    bad = [dict(H=0), dict(W=0), dict(H=-1), dict(H=16385), dict(W=16385), dict(W=2 ** 31 - 1),
           dict(V=-1), dict(F=-1), dict(V=2 ** 31), dict(F=2 ** 31), dict(V=-2 ** 63), dict(F=2 ** 62),
           dict(c2w=None), dict(c2w=c2w_with(0, nan)), dict(c2w=c2w_with(7, inf)), dict(c2w=c2w_with(11, -inf)),
           dict(fx=nan), dict(fy=inf), dict(cx=-inf), dict(cy=nan), dict(fx=0.0), dict(fy=-0.0),
           dict(near=0.0), dict(near=-1.0), dict(near=nan), dict(near=inf), dict(bg=nan), dict(bg=inf),
           dict(cull=-1), dict(cull=3),
           dict(count=None), dict(count=None, F=0), dict(v=None), dict(f=None), dict(ws=None),
           dict(attr=None), dict(attr=None, F=0),
           dict(f=p(0x2004)), dict(count=p(0x7004)), dict(ws=p(0x8004)), dict(f=p(0x2004), F=0)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"ns_mesh_raster" in lib.ns_last_error()
    header = open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()
    share = int(re.search(r"#define NS_MESH_RASTER_SHARE (\d+)", header).group(1))
    assert share == 1024 and int(re.search(r"#define NS_MESH_RASTER_BIG_BOX (\d+)", header).group(1)) >= 1
    size = lib.ns_mesh_raster_workspace_bytes
    r256 = lambda n: (n + 255) // 256 * 256                                                    # noqa: E731
    # eight bytes per pixel, sixteen per vertex, four per face, one line for the list's length; no face, no workspace
    for V, F, H, W in ((8, 4, 8, 8), (0, 1, 1, 1), (1000, 2049, 37, 29), (2 ** 31 - 1, 2 ** 31 - 1, 16384, 16384)):
        assert size(V, F, H, W) == r256(8 * H * W) + r256(16 * V) + r256(4 * F) + 256, (V, F, H, W)
    assert size(8, 0, 8, 8) == 0
    for V, F, H, W in ((-1, 4, 8, 8), (8, -1, 8, 8), (2 ** 31, 4, 8, 8), (8, 2 ** 31, 8, 8), (8, 4, 0, 8), (8, 4, 8, 0),
                       (8, 4, 16385, 8), (8, 4, 8, 16385), (8, 4, -1, 8)):
        assert size(V, F, H, W) == 0, (V, F, H, W)


def test_ops_mesh_rasterize_refuses_before_any_launch():
    import torch

    from nerf_sampling_amd import ops

    v, f = torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int64)
    K = [[10.0, 0, 4.0], [0, 10.0, 4.0], [0, 0, 1]]
    for bad in (v, v.numpy(), None):                                                      # not on the device
        with pytest.raises(ValueError):
            ops.mesh_rasterize(bad, f, RR.IDENTITY, 8, 8, K, 0.5)
    p = inspect.signature(ops.mesh_rasterize).parameters
    assert list(p) == ["vertices", "faces", "c2w", "H", "W", "K", "near", "rgb", "background", "cull", "workspace"]
    assert (p["rgb"].default, p["background"].default, p["cull"].default, p["workspace"].default) == (None, 0.0, 0, None)
    assert list(inspect.signature(ops.mesh_raster_workspace_bytes).parameters) == ["n_vertices", "n_faces", "H", "W"]
    assert ops.mesh_raster_workspace_bytes(1, 1, 1, 1) == 4 * 256 and ops.mesh_raster_workspace_bytes(1, 1, 0, 1) == 0


def test_new_switch_defaults_off_and_needs_the_mesh():
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.experiments.render import main
    from nerf_sampling_amd.trainers import Trainer

    p = inspect.signature(Trainer.__init__).parameters
    assert p["device_mesh_eval"].default is False
    base = dict(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="")
    assert Trainer(**base).device_mesh_eval is False
    assert Trainer(**base, device_mesh=True, device_mesh_eval=True).device_mesh_eval is True
    for kw in (dict(device_mesh_eval=True), dict(device_mesh=True, device_mesh_eval=1), dict(device_mesh=True, device_mesh_eval="yes")):
        with pytest.raises(ValueError):
            Trainer(**base, **kw)
    opts = {o.name: o for o in main.params}
    flag = opts["device_mesh_eval"]
    assert flag.is_flag and flag.default is False and "--device-mesh-eval" in flag.opts
    views = inspect.signature(nerf_utils.render_mesh_views).parameters
    assert list(views)[:8] == ["mesh", "poses", "hwf", "K", "near", "savedir", "background", "cull"]
    assert views["savedir"].default is None and views["cull"].default == 0
    score = inspect.signature(nerf_utils.score_mesh_views).parameters
    assert list(score)[:11] == ["dataset", "image_ids", "poses", "hwf", "K", "mesh", "near", "field_depths", "field_accs",
                                "render_kwargs", "savedir"]
    assert all(score[k].default is None for k in ("field_depths", "field_accs", "render_kwargs", "savedir"))
    assert nerf_utils.format_mesh_txt("IoU", [0.5, 1.0], 0.75) == "000.png, IoU: 0.5\n001.png, IoU: 1.0\nAvg of 2 images:\nIoU: 0.75\n"
    # refused before anything is rasterised
    with pytest.raises(ValueError):
        nerf_utils.render_mesh_views({"vertices": None}, [], (8, 8, 1.0), None, 0.5)
    with pytest.raises(ValueError):
        nerf_utils.score_mesh_views(None, [0], [None], (8, 8, 1.0), None, {}, 0.5, field_depths=[None])
