"""ns_mesh_raster / ops.mesh_rasterize: the device mesh rasterised from a pinhole camera.
Yardstick (tests/mesh_raster_reference.py, numpy): the header's definition restated -- float32 projection operation by operation,
np.rint, int64 coverage with the tie rule, float64 depth and colour, a lexicographic minimum over (depth bits, face) --: the
depth, face and colour BITS of every pixel and the four counters are equal.

Every call of ``run`` goes through the C ABI with a workspace of exactly ns_mesh_raster_workspace_bytes, poisoned and fenced by
guard bytes, outputs poisoned with PAD elements behind them, and counters that hold garbage before the call.  No frame is larger
than 64 x 48 and no mesh has more than 20 000 faces."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_raster_reference as RR
import mesh_reference as MR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()
S = int(re.search(r"#define NS_MESH_RASTER_SHARE (\d+)", _HEADER).group(1))
BIG = int(re.search(r"#define NS_MESH_RASTER_BIG_BOX (\d+)", _HEADER).group(1))
POISON = 0xA5
PAD = 16
UNIT = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0)
_reference = {}


def case(vertices, faces, H, W, c2w=RR.IDENTITY, attr="ramp", near=0.5, cull=0, background=0.0, **cam):
    cam = dict(UNIT, **cam)
    vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    if isinstance(attr, str):                               # colours that differ per vertex and per channel, some beyond [0, 1]
        k = np.arange(vertices.shape[0], dtype=np.float64)[:, None]
        attr = (np.mod(k * np.array([0.37, 0.61, 0.13]) + np.array([0.1, 0.5, 0.9]), 1.25) - 0.1).astype(np.float32)
    return dict(vertices=vertices, faces=np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3), attr=attr,
                c2w=np.ascontiguousarray(c2w, dtype=np.float32), H=int(H), W=int(W), near=float(near), cull=int(cull),
                background=float(background), **cam)


def reference(name, make):
    """(case, restatement) of a named case: built and restated once, shared, never modified"""
    if name not in _reference:
        c = make()
        want = RR.rasterize(c["vertices"], c["faces"], c["c2w"], c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"], c["near"],
                            attr=c["attr"], background=c["background"], cull=c["cull"])
        for a in list(c.values()) + list(want.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _reference[name] = (c, want)
    return _reference[name]


def run(c, poison=POISON, null=(), stream=None):
    """One call through the C ABI -> dict(depth, tri, rgb: bits as int32, or None; counts), after checking that nothing behind
    the outputs, outside the workspace or behind the counters was written.  ``null``: the outputs passed as NULL."""
    import torch

    from nerf_sampling_amd import _lib

    lib = _lib.load()
    V, F, H, W = c["vertices"].shape[0], c["faces"].shape[0], c["H"], c["W"]
    need = lib.ns_mesh_raster_workspace_bytes(V, F, H, W)
    r256 = lambda n: (n + 255) // 256 * 256                                                   # noqa: E731
    assert need == (r256(8 * H * W) + r256(16 * V) + r256(4 * F) + 256 if F else 0)
    byte = lambda n, v=POISON: torch.full((n,), v, dtype=torch.uint8, device="cuda")          # noqa: E731
    ws = byte(need + 512, poison)
    ws[:256] = POISON
    ws[256 + need:] = POISON
    counters = byte(32 + 256)
    outs = {"depth": byte((H * W + PAD) * 4), "tri": byte((H * W + PAD) * 4), "rgb": byte((H * W + PAD) * 12)}
    vertices = torch.from_numpy(np.array(c["vertices"])).cuda() if V else byte(64)
    faces = torch.from_numpy(np.array(c["faces"])).cuda() if F else None
    attr = torch.from_numpy(np.array(c["attr"])).cuda() if c["attr"] is not None and V else (byte(64) if c["attr"] is not None else None)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())                             # noqa: E731
    out_ptr = {k: (None if (k in null or (k == "rgb" and c["attr"] is None)) else p(t)) for k, t in outs.items()}
    c2w = (C.c_float * 12)(*[float(v) for v in c["c2w"].reshape(-1)])
    where = torch.cuda.current_stream() if stream is None else stream
    rc = lib.ns_mesh_raster(p(vertices), V, p(faces), F, p(attr), c2w, c["fx"], c["fy"], c["cx"], c["cy"], H, W, c["near"],
                            c["cull"], c["background"], out_ptr["depth"], out_ptr["tri"], out_ptr["rgb"], p(counters),
                            C.c_void_p(ws.data_ptr() + 256) if F else None, C.c_void_p(where.cuda_stream))
    assert rc == 0, lib.ns_last_error()
    where.synchronize()
    b = ws.cpu().numpy()
    assert (b[:256] == POISON).all() and (b[256 + need:] == POISON).all(), "written outside the workspace"
    cb = counters.cpu().numpy()
    assert (cb[32:] == POISON).all(), "written behind the counters"
    got = {"counts": cb[:32].view(np.int64).copy()}
    for k, t in outs.items():
        raw, n = t.cpu().numpy(), H * W * (12 if k == "rgb" else 4)
        if out_ptr[k] is None:
            assert (raw == POISON).all(), f"{k} is NULL and was written"
            got[k] = None
        else:
            assert (raw[n:] == POISON).all(), f"written behind {k}"
            got[k] = raw[:n].view(np.int32).reshape((H * W, 3) if k == "rgb" else (H * W,)).copy()
    return got


def compare(got, want, what):
    assert got["counts"].tolist() == want["counts"].tolist(), what
    for k in ("depth", "tri", "rgb"):
        if got[k] is None:
            continue
        bits = want[k].view(np.int32) if k != "tri" else want[k]
        differ = int((got[k] != bits).sum())
        assert differ == 0, f"{what}: {differ} values of {k} differ from the restatement"


def check(name, make, **kw):
    c, want = reference(name, make)
    got = run(c, **kw)
    print(f"{name}: {c['faces'].shape[0]} faces on {c['vertices'].shape[0]} vertices, frame {c['W']} x {c['H']}, counts "
          f"{want['counts'].tolist()}")
    compare(got, want, name)
    return c, want, got


# ---- the cases ----
def _screen(xy, z, faces, H, W, **kw):
    return lambda: case(RR.screen_vertices(xy, z), faces, H, W, **kw)


def _windings(tri):
    a, b, c = tri
    return [(a, b, c), (b, c, a), (c, a, b), (a, c, b), (c, b, a), (b, a, c)]


def _random_faces(n, H, W, seed, size=3.0, c2w=None, **cam):
    """n small triangles scattered over and around the frame, in camera space at depths 1 .. 3, moved into the world of c2w"""
    def make():
        rng = np.random.default_rng(seed)
        base = rng.uniform([-3.0, -3.0], [W + 3.0, H + 3.0], size=(n, 1, 2))
        xy = (base + rng.uniform(-size, size, size=(n, 3, 2))).reshape(-1, 2)
        if seed % 2:
            xy = np.round(xy * 2.0) / 2.0                   # half pixels: centres on edges and on vertices occur
        z = rng.uniform(1.0, 3.0, size=3 * n)
        k = dict(UNIT, **cam)
        pc = RR.screen_vertices(xy, z, **k).astype(np.float64)
        m = RR.IDENTITY if c2w is None else c2w
        world = pc @ np.asarray(m[:, :3], dtype=np.float64).T + np.asarray(m[:, 3], dtype=np.float64)
        return case(world, np.arange(3 * n).reshape(n, 3), H, W, c2w=m, **cam)
    return make


POSE = RR.look_at((2.0, -2.5, 1.5))
CAM = dict(fx=21.5, fy=19.25, cx=17.75, cy=14.5)


def test_hand_cases():
    _, want, _ = check("right triangle", _screen([(0, 0), (4, 0), (0, 4)], 2.0, [[0, 1, 2]], 6, 7))
    assert want["counts"].tolist() == [0, 0, 0, 10]
    _, want, got = check("perspective", _screen([(0, 0), (4, 0), (0, 4)], [1.0, 2.0, 4.0], [[0, 1, 2]], 5, 5,
                                                attr=np.eye(3, dtype=np.float32), background=0.25))
    assert got["depth"][6] == np.float32(16.0 / 11.0).view(np.int32)
    assert got["rgb"][6].tolist() == np.array([8.0 / 11.0, 2.0 / 11.0, 1.0 / 11.0], dtype=np.float32).view(np.int32).tolist()


@pytest.mark.parametrize("corner", [0, 1])
def test_tie_rule_on_split_quads(corner):
    xy = [(1, 1), (5, 1), (5, 5), (1, 5)]
    pair = [(0, 1, 2), (0, 2, 3)] if corner == 0 else [(1, 2, 3), (1, 3, 0)]
    for a in (0, 3, 4):
        for b in (0, 2, 5):
            faces = [_windings(pair[0])[a], _windings(pair[1])[b]]
            _, want, got = check(f"quad {corner} {a} {b}", _screen(xy, 2.0, faces, 7, 8))
            assert want["counts"][3] == 16 and ((got["tri"] >= 0).reshape(7, 8)[1:5, 1:5]).all()


def test_tie_rule_on_a_fan():
    ring = [(0, 1), (3, 0), (6, 1), (6, 5), (3, 6), (0, 5)]
    covered = None
    for trial in range(4):
        rng = np.random.default_rng(trial)
        faces = [_windings((0, 1 + k, 1 + (k + 1) % 6))[int(rng.integers(6)) if trial else 0] for k in range(6)]
        _, want, got = check(f"fan {trial}", _screen([(3, 3)] + ring, 2.0, faces, 8, 8))
        assert got["tri"][3 * 8 + 3] >= 0 and want["n_cover"].max() == 1
        covered = (got["tri"] >= 0) if covered is None else covered
        assert ((got["tri"] >= 0) == covered).all()


def _frame(W, H):
    return f"frame {W} x {H}", _random_faces(300, H, W, seed=W + H, size=max(2.0, W / 6.0), c2w=POSE, fx=20.0, fy=20.0,
                                             cx=0.5 * W, cy=0.5 * H)


@pytest.mark.parametrize("W,H", [(1, 1), (1, 37), (37, 1), (37, 29), (64, 48)])
def test_frame_sizes(W, H):
    _, want, _ = check(*_frame(W, H))
    assert want["counts"][3] > 0


def _covering():
    # one back-facing and one front-facing triangle, each far larger than the 64 x 48 frame, at different depths
    xy = [(-200, -100), (400, -100), (-200, 500), (-150, -120), (-150, 600), (500, -120)]
    return case(RR.screen_vertices(xy, [2.0, 2.5, 3.0, 2.3, 2.4, 2.35]), [[0, 1, 2], [3, 4, 5]], 48, 64)


def test_one_face_covering_the_frame():
    """the workgroup path: every pixel of the frame is covered by both faces"""
    _, want, _ = check("covering", _covering)
    assert want["counts"][3] == 64 * 48 and (want["n_cover"] == 2).all() and set(np.unique(want["tri"])) == {0, 1}


@pytest.mark.parametrize("wide,tall", [(33, 31), (32, 32), (41, 25), (64, 48)])
def test_bounding_boxes_around_the_path_threshold(wide, tall):
    """right triangles whose clamped bounding boxes have BIG - 1, BIG and BIG + 1 pixels (and the whole frame): the last two
    take the workgroup launch, and nothing tells"""
    assert BIG == 1024 and wide * tall in (BIG - 1, BIG, BIG + 1, 64 * 48)
    xy = [(3, 2), (3 + wide - 1, 2), (3, 2 + tall - 1), (3 + wide - 1, 2 + tall - 1)]
    _, want, _ = check(f"box {wide} x {tall}", _screen(xy, [1.0, 2.0, 3.0, 1.5], [[0, 1, 2], [3, 2, 1]], 48, 64))
    assert want["counts"][3] > wide * tall // 2


def test_the_path_threshold_is_not_observable():
    """ns_debug_set("mesh_raster_big_box"): every face through the workgroup launch (1), none (2^30), and the default"""
    from nerf_sampling_amd import ops

    for name, make in (("covering", _covering), _frame(64, 48), _closed("ball", 0)):
        c, want = reference(name, make)
        for box in (1, 7, 256, 1 << 30):
            with ops.debug_switch(mesh_raster_big_box=box):
                compare(run(c), want, f"{name}, big box {box}")


@pytest.mark.parametrize("F", [0, 1, S - 1, S, S + 1, 2 * S + 1])
def test_face_counts_around_the_share(F):
    check(f"F = {F}", _random_faces(F, 29, 37, seed=11 + F, c2w=POSE, **CAM))


def test_no_vertices():
    """V == 0: every face is invalid, the frame is background"""
    c, want, got = check("V = 0", lambda: case(np.zeros((0, 3)), [[0, 1, 2], [0, 0, 0], [-1, 5, 2]], 5, 7, background=1.0))
    assert want["counts"].tolist() == [0, 0, 3, 0] and (got["tri"] == -1).all()
    assert (got["rgb"] == np.float32(1.0).view(np.int32)).all() and (got["depth"] == 0).all()


def test_equal_depths_go_to_the_smaller_index():
    # two coincident faces, then a third of another shape in the same plane z = 2: the depth bits are 2.0f for all of them
    xy = [(0, 0), (6, 0), (0, 6), (6, 6), (1, 5)]
    faces = [[1, 3, 4], [0, 1, 2], [0, 1, 2], [2, 1, 3]]
    _, want, got = check("coincident", _screen(xy, 2.0, faces, 8, 8))
    hit = got["tri"] >= 0
    assert (got["depth"][hit] == np.float32(2.0).view(np.int32)).all() and 2 not in set(got["tri"].tolist())
    assert (want["n_cover"] >= 2).sum() > 10 and {0, 1} <= set(got["tri"].tolist())
    # the same faces in another order: the winner at a pixel covered by several is the smallest index again
    check("coincident, reordered", _screen(xy, 2.0, faces[::-1], 8, 8))


def test_contention_on_few_words():
    _, want, _ = check("contention", _random_faces(5000, 16, 16, seed=2, size=6.0))
    assert want["n_cover"].min() > 20


def _unusable():
    z_near = np.float32(0.5)
    below = np.nextafter(z_near, np.float32(0.0))
    edge, beyond = np.float32(2.0 ** 20), np.nextafter(np.float32(2.0 ** 20), np.float32(np.inf))
    v = [(0, 0, -2), (8, 0, -2), (0, -8, -2),                 # 0-2: a usable triangle
         (0, 0, 1.0),                                         # 3: behind the camera
         (1, -1, -float(below)), (1, -1, -float(z_near)),     # 4: z just below near_; 5: exactly at it
         (np.nan, 0, -2), (0, np.inf, -2), (0, 0, -np.inf), (-np.inf, 0, -2),      # 6-9
         (float(edge), 0, -1), (float(beyond), 0, -1), (0, float(edge), -1), (0, -float(beyond), -1),   # 10-13: the band
         (0, 0, 0.0), (3e38, 3e38, -1e-38)]                   # 14: z = 0; 15: a quotient that overflows
    faces = [[0, 1, 2], [0, 1, 3], [0, 4, 2], [0, 5, 2], [6, 1, 2], [0, 7, 2], [0, 1, 8], [9, 1, 2], [0, 10, 2], [0, 11, 2],
             [0, 1, 12], [0, 1, 13], [14, 1, 2], [0, 15, 2], [10, 12, 5]]
    return case(np.array(v, dtype=np.float32), faces, 6, 7)


def test_unusable_vertices_drop_their_faces():
    _, want, got = check("unusable", _unusable)
    # usable: 0, 1, 2, 5, 10 and 12 (the band's edge is inside) -> faces 0, 3, 8, 10, 14 are rasterised, ten are clipped
    assert want["usable"].tolist() == [True, True, True, False, False, True] + [False] * 4 + [True, False, True, False, False, False]
    assert want["counts"][:3].tolist() == [10, 0, 0] and want["counts"][3] > 10
    assert {0, 3, 8, 10, 14} >= set(got["tri"][got["tri"] >= 0].tolist())


def test_off_frame_degenerate_and_invalid_faces():
    xy = [(0, 0), (4, 0), (0, 4), (-9, -9), (-3, -9), (-9, -2), (20, 1), (30, 1), (20, 9), (1, 1), (2, 2), (3, 3), (1, 40), (2, 50)]
    V = len(xy)
    faces = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [12, 13, 6],             # one on the frame, three wholly off it
             [9, 10, 11], [0, 0, 1], [2, 2, 2], [1, 0, 1],             # collinear, repeated vertices
             [-1, 1, 2], [0, V, 2], [0, 1, 2 ** 32 + 1], [2 ** 32, 2 ** 32 + 1, 2 ** 32 + 2], [-2 ** 63, 0, 1], [0, 1, 2 ** 63 - 1]]
    _, want, got = check("off frame", _screen(xy, 2.0, faces, 6, 7))
    assert want["counts"].tolist() == [0, 4, 6, 10] and set(got["tri"].tolist()) == {-1, 0}


_surfaces = {}


def _surface(which):
    if which not in _surfaces:
        sigma, lo, h = MR.sphere(24) if which == "ball" else MR.torus(24)
        tri, keys, _ = MR.march(sigma, 0.0, lo, h)
        _surfaces[which] = MR.weld(tri, keys)
    return _surfaces[which]


BALL_CAM = dict(fx=60.0, fy=60.0, cx=24.0, cy=20.0)


def _closed(which, cull):
    def make():
        v, f = _surface(which)
        return case(v, f, 40, 48, c2w=POSE, cull=cull, background=1.0 if cull == 1 else 0.0, **BALL_CAM)
    return f"{which} cull {cull}", make


@pytest.mark.parametrize("which", ["ball", "torus"])
@pytest.mark.parametrize("cull", [0, 1, 2])
def test_culling_on_closed_surfaces(which, cull):
    c, want, got = check(*_closed(which, cull))
    assert c["faces"].shape[0] < 20000 and want["counts"][3] > 300
    if cull == 1:                                           # the front faces are the nearer ones: the frame of cull = 0
        _, both = reference(*_closed(which, 0))
        assert (both["tri"] == want["tri"]).all() and (both["depth"] == want["depth"]).all()
    if cull == 0 and which == "ball":
        inside = want["n_cover"] > 0
        assert (want["n_cover"][inside] == 2).all() and (want["n_front"][inside] == 1).all()


def test_without_colours_and_each_output_null():
    c, want = reference(*_frame(37, 29))
    bare = dict(c, attr=None)
    got = run(bare)
    assert got["rgb"] is None
    compare(got, want, "no colours")
    for null in (("depth",), ("tri",), ("rgb",), ("depth", "tri", "rgb")):
        got = run(c, null=null)
        assert all(got[k] is None for k in null)
        compare(got, want, f"NULL {null}")


def test_workspace_contents_do_not_matter():
    for name, make in (_frame(37, 29), ("covering", _covering), _closed("torus", 0)):
        c, want = reference(name, make)
        for poison in (0x00, 0xFF):
            compare(run(c, poison=poison), want, f"{name}, workspace {poison:#x}")


def test_second_stream_and_repeatability():
    import torch

    c, want = reference("contention", _random_faces(5000, 16, 16, seed=2, size=6.0))
    first = run(c)
    again = run(c)
    for k in ("depth", "tri", "rgb", "counts"):
        assert (first[k] == again[k]).all(), k
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        compare(run(c, stream=side), want, "second stream")


def test_through_ops():
    """ops.mesh_rasterize on the ball: the same bits, the four counts as ints, and what it refuses"""
    import torch

    from nerf_sampling_amd import ops

    cam = BALL_CAM
    c, want = reference(*_closed("ball", 0))
    K = [[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1]]
    V, F, A = (torch.from_numpy(np.array(c[k])).cuda() for k in ("vertices", "faces", "attr"))
    got = ops.mesh_rasterize(V, F, torch.from_numpy(np.array(c["c2w"])), 40, 48, K, 0.5, rgb=A)
    assert (got["n_clipped"], got["n_degenerate"], got["n_invalid"], got["n_covered"]) == tuple(want["counts"].tolist())
    assert torch.equal(got["depth"].cpu(), torch.from_numpy(np.array(want["depth"])))
    assert torch.equal(got["tri"].cpu(), torch.from_numpy(np.array(want["tri"])))
    assert torch.equal(got["rgb"].cpu().view(torch.int32), torch.from_numpy(np.array(want["rgb"])).view(torch.int32))
    ws = torch.full((ops.mesh_raster_workspace_bytes(V.shape[0], F.shape[0], 40, 48),), 0xFF, dtype=torch.uint8, device="cuda")
    bare = ops.mesh_rasterize(V, F, c["c2w"], 40, 48, K, 0.5, workspace=ws)
    assert bare["rgb"] is None and torch.equal(bare["depth"], got["depth"]) and torch.equal(bare["tri"], got["tri"])
    empty = ops.mesh_rasterize(V[:0], F, c["c2w"], 40, 48, K, 0.5)
    assert empty["n_invalid"] == F.shape[0] and empty["n_covered"] == 0
    none = ops.mesh_rasterize(V, F[:0], c["c2w"], 4, 5, K, 0.5, rgb=A, background=1.0)
    assert none["n_covered"] == 0 and (none["rgb"] == 1.0).all() and (none["tri"] == -1).all()
    for bad in (dict(near=0.0), dict(cull=3), dict(background=float("nan")), dict(workspace=ws[1:]), dict(rgb=A[:-1]),
                dict(H=0), dict(W=16385)):
        kw = dict(H=40, W=48, near=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.mesh_rasterize(V, F, c["c2w"], kw.pop("H"), kw.pop("W"), K, kw.pop("near"), **kw)
    with pytest.raises(ValueError):
        ops.mesh_rasterize(V, F.int(), c["c2w"], 40, 48, K, 0.5)
