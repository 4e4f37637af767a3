"""ns_mesh_extract / ops.mesh_extract / ops.mesh_weld: the isosurface of a lattice by marching tetrahedra on the device.
Yardstick (tests/mesh_reference.py, numpy): the header's definition restated in float32 in the same order of operations -- the
triangle count, their order, the keys and the position BITS are equal --, and for the kernel's own output the invariants of a
closed oriented surface, which neither the kernel nor the restatement defines.

S, the number of cells one workgroup owns, is the header's NS_MESH_SHARE.  Every call of ``run`` goes through the C ABI with a
workspace of exactly ns_mesh_workspace_bytes, poisoned with 0xA5 and fenced by guard bytes, outputs poisoned the same way with
PAD records behind the capacity, and counters that hold garbage before the call."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_reference as MR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
PAD = 8                                                   # poisoned triangles behind the capacity
S = int(re.search(r"#define NS_MESH_SHARE (\d+)", open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()).group(1))
_reference = {}


def reference(name, make):
    """(sigma, iso, lo, h, triangles, keys, n_skipped) of a named lattice: built and marched once, shared, never modified"""
    if name not in _reference:
        sigma, iso, lo, h = make()
        sigma = np.ascontiguousarray(sigma, dtype=np.float32)
        tri, keys, skipped = MR.march(sigma, iso, lo, h)
        for a in (sigma, tri, keys):
            a.setflags(write=False)
        _reference[name] = (sigma, np.float32(iso), np.asarray(lo, np.float32), np.asarray(h, np.float32), tri, keys, skipped)
    return _reference[name]


def run(sigma, iso, lo, h, capacity, stride=1):
    """One call through the C ABI -> (triangle bits [m,3,3] int32, keys [m,3], n_triangles, n_skipped), m = min(n, capacity),
    after checking that nothing at or beyond the capacity, outside the workspace or behind the counters was written.
    ``stride`` 4: sigma is the last column of a [., 4] array whose other columns are NaN."""
    import torch

    from nerf_sampling_amd import _lib

    lib = _lib.load()
    Gz, Gy, Gx = sigma.shape
    host = torch.from_numpy(np.array(sigma, dtype=np.float32))                           # a writable copy of the shared lattice
    if stride == 1:
        dev = host.cuda()
        sigma_ptr = dev.data_ptr()
    else:
        dev = torch.full((sigma.size, stride), float("nan"), dtype=torch.float32, device="cuda")
        dev[:, stride - 1] = host.reshape(-1).cuda()
        sigma_ptr = dev.data_ptr() + 4 * (stride - 1)
    need = lib.ns_mesh_workspace_bytes(Gx, Gy, Gz)
    groups = ((Gx - 1) * (Gy - 1) * (Gz - 1) + S - 1) // S
    assert need == (16 * groups + 255) // 256 * 256
    byte = lambda n: torch.full((n,), POISON, dtype=torch.uint8, device="cuda")           # noqa: E731
    ws = byte(need + 512)
    counters = byte(16 + 256)
    tri = byte((capacity + PAD) * 36) if capacity > 0 else None
    keys = byte((capacity + PAD) * 24) if capacity > 0 else None
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())                          # noqa: E731
    rc = lib.ns_mesh_extract(C.c_void_p(sigma_ptr), stride, Gx, Gy, Gz, float(iso), *(float(v) for v in lo),
                             *(float(v) for v in h), p(tri), p(keys), capacity, p(counters), C.c_void_p(ws.data_ptr() + 256),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ns_last_error()
    b = ws.cpu().numpy()
    assert (b[:256] == POISON).all() and (b[-256:] == POISON).all(), "written outside the workspace"
    c = counters.cpu().numpy()
    assert (c[16:] == POISON).all()
    n_triangles, n_skipped = (int(v) for v in c[:16].view(np.int64))
    if capacity == 0:
        return np.empty((0, 3, 3), np.int32), np.empty((0, 3), np.int64), n_triangles, n_skipped
    tb, kb = tri.cpu().numpy(), keys.cpu().numpy()
    m = min(n_triangles, capacity)
    assert (tb[m * 36:] == POISON).all() and (kb[m * 24:] == POISON).all(), "written at or beyond the capacity (or the count)"
    return tb[:m * 36].view(np.int32).reshape(m, 3, 3), kb[:m * 24].view(np.int64).reshape(m, 3), n_triangles, n_skipped


def check(name, make, stride=1):
    sigma, iso, lo, h, tri, keys, skipped = reference(name, make)
    n = tri.shape[0]
    got_tri, got_keys, n_triangles, n_skipped = run(sigma, iso, lo, h, n, stride=stride)
    print(f"{name}: lattice {sigma.shape[::-1]}, {n} triangles, {skipped} cells skipped")
    assert (n_triangles, n_skipped) == (n, skipped)
    assert (got_keys == keys).all()
    assert (got_tri == tri.view(np.int32)).all()
    return sigma, iso, lo, h, tri, keys, skipped


def _normal(shape, seed, lo=(-1.0, 0.5, 3.0), h=(0.25, 0.125, 0.75)):
    return lambda: (np.random.default_rng(seed).standard_normal(shape).astype(np.float32), 0.1, lo, h)


def _all_patterns():
    """[2,2,512]: cell 2 m (lattice columns 2 m and 2 m + 1) has the corner with code c inside iff bit c of m is set"""
    rng = np.random.default_rng(11)
    s = np.empty((2, 2, 512), dtype=np.float32)
    for m in range(256):
        for c in range(8):
            magnitude = np.float32(rng.uniform(0.1, 2.0))
            s[c >> 2, (c >> 1) & 1, 2 * m + (c & 1)] = magnitude if (m >> c) & 1 else -magnitude
    return s, 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def test_all_256_patterns_of_a_cell():
    sigma, iso, lo, h, tri, keys, _ = check("patterns", _all_patterns)
    # a key is lin(a) * 8 + d: the triangles that lie in columns 2 m and 2 m + 1 alone are those of cell 2 m
    x_lo, x_hi = keys // 8 % 512, keys // 8 % 512 + (keys & 1)
    per_cell = [int(((x_lo >= 2 * m).all(axis=1) & (x_hi <= 2 * m + 1).all(axis=1) & (x_hi.max(axis=1) == 2 * m + 1)).sum())
                for m in range(256)]
    assert per_cell[0] == 0 and per_cell[255] == 0 and all(2 <= n <= 12 for n in per_cell[1:255]) and max(per_cell) == 12


@pytest.mark.parametrize("dims", [(70, 5, 3), (3, 5, 70), (5, 70, 3)], ids=str)
def test_one_long_axis(dims):
    Gx, Gy, Gz = dims
    check(f"long{dims}", _normal((Gz, Gy, Gx), 3))


@pytest.mark.parametrize("dims", [(S + 2, 2, 2), (2 * S + 2, 2, 2), (19, 17, 13), (2, 3, S + 2)], ids=str)
def test_share_boundaries(dims):
    """S + 1 and 2 S + 1 cells -- the last workgroup owns ONE cell --, and 18 x 16 x 12 = 3456 cells, 3.4 shares and no multiple
    of 256; the fourth has the long axis last, so that consecutive cells of a share change rows"""
    Gx, Gy, Gz = dims
    cells = (Gx - 1) * (Gy - 1) * (Gz - 1)
    assert cells > S and cells % 256 != 0
    check(f"share{dims}", _normal((Gz, Gy, Gx), 5))


def test_sigma_column_of_a_raw_array():
    check("long(70, 5, 3)", _normal((3, 5, 70), 3), stride=4)
    check("share(19, 17, 13)", _normal((13, 17, 19), 5), stride=4)


def test_no_crossing_and_everything_inside():
    for name, value in (("below", -1.0), ("above", 2.0), ("at iso", 0.1)):
        sigma, iso, lo, h, tri, keys, skipped = check(name, lambda v=value: (np.full((6, 7, 40), v, np.float32), 0.1,
                                                                            (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
        assert tri.shape[0] == 0 and skipped == 0


def test_a_corner_exactly_at_iso():
    sigma, iso, lo, h, tri, keys, _ = check("noise", lambda: (MR.noise()[0], 0.0, MR.noise()[1], MR.noise()[2]))
    areas = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert (areas == 0).any()                              # the vertices ON the corner: triangles of zero area
    # many corners at iso, on both sides of others
    check("quantised", lambda: (np.round(np.random.default_rng(9).standard_normal((9, 8, 21)) * 2).astype(np.float32) / 2, 0.5,
                                (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))


def _non_finite():
    rng = np.random.default_rng(13)
    s = rng.standard_normal((9, 10, 37)).astype(np.float32)
    pick = rng.integers(0, 40, size=s.shape)
    s[pick == 0] = np.nan
    s[pick == 1] = np.inf
    s[pick == 2] = -np.inf
    return s, 0.1, (-1.0, 0.5, 3.0), (0.25, 0.125, 0.75)


def test_nan_and_infinite_corners_skip_their_cells():
    sigma, iso, lo, h, tri, keys, skipped = check("non finite", _non_finite)
    finite = np.isfinite(sigma)
    whole = np.ones((8, 9, 36), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                whole &= finite[dz:dz + 8, dy:dy + 9, dx:dx + 36]
    assert skipped == int((~whole).sum()) and 0 < skipped < whole.size and tri.shape[0] > 0
    assert np.isfinite(tri).all()


def test_capacity_zero_counts_and_a_small_capacity_keeps_the_fence():
    sigma, iso, lo, h, tri, keys, skipped = reference("share(19, 17, 13)", _normal((13, 17, 19), 5))
    n = tri.shape[0]
    _t, _k, n_triangles, n_skipped = run(sigma, iso, lo, h, 0)                 # NULL outputs
    assert (n_triangles, n_skipped) == (n, skipped)
    # a capacity inside the first share, at a share's first triangle region, and one short of everything
    for capacity in (1, 7, n // 2, n - 1, n + 5):
        got_tri, got_keys, n_triangles, n_skipped = run(sigma, iso, lo, h, capacity)
        m = min(n, capacity)
        assert (n_triangles, n_skipped) == (n, skipped) and got_tri.shape[0] == m
        assert (got_keys == keys[:m]).all() and (got_tri == tri[:m].view(np.int32)).all()


TILE_LATTICES = {2047: (2048, 33, 33), 2048: (129, 129, 129), 2049: (2050, 33, 33), 4097: (4098, 33, 33)}


def _two_balls(dims):
    """a ball of radius 3.7 cells around lattice point (2, 2, 2) and one around (Gx - 3, Gy - 3, Gz - 3), both cut by the faces
    of the lattice, so that the first and the last cells hold triangles, and nothing between them; the lattice's last point is
    NaN: the last cell, and only it, is skipped"""
    def make():
        Gx, Gy, Gz = dims
        z, y, x = np.meshgrid(np.arange(Gz, dtype=np.float32), np.arange(Gy, dtype=np.float32), np.arange(Gx, dtype=np.float32),
                              indexing="ij", sparse=True)
        near = np.sqrt((x - 2) ** 2 + (y - 2) ** 2 + (z - 2) ** 2)
        far = np.sqrt((x - (Gx - 3)) ** 2 + (y - (Gy - 3)) ** 2 + (z - (Gz - 3)) ** 2)
        sigma = (np.float32(3.7) - np.minimum(near, far)).astype(np.float32)
        sigma[-1, -1, -1] = np.nan
        return sigma, 0.0, (-1.0, 0.5, 3.0), (0.25, 0.125, 0.75)
    return make


def _cell_of(keys, dims):
    """the cell index e of the lattice point a key's edge starts from (that point is a corner of the triangle's cell)"""
    Gx, Gy, Gz = dims
    lin = keys // 8
    i, j, k = lin % Gx, lin // Gx % Gy, lin // (Gx * Gy)
    return (np.minimum(k, Gz - 2) * (Gy - 1) + np.minimum(j, Gy - 2)) * (Gx - 1) + np.minimum(i, Gx - 2)


@pytest.mark.parametrize("shares", sorted(TILE_LATTICES))
def test_the_scan_across_its_tiles(shares):
    """The scan of the per-share counts walks tiles of 2048 entries with a carry and two LDS buffers in turn: lattices of exactly
    2047, 2048, 2049 and 4097 shares, triangles in the first and in the last shares only, and the one skipped cell in the last
    share, so both totals and every index of the second ball cross every tile boundary there is."""
    dims = TILE_LATTICES[shares]
    assert S == 1024 and (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1) == shares * S
    sigma, iso, lo, h, tri, keys, skipped = check(f"tiles{dims}", _two_balls(dims))
    cells = _cell_of(keys, dims)
    first_ball = int((cells.max(axis=1) < shares * S // 2).sum())
    assert skipped == 1 and 0 < first_ball < tri.shape[0]
    assert cells.min() < S and cells.max() >= (shares - 1) * S             # triangles in share 0 and in the last share
    if shares == 2049:
        # fewer records than the first ball has triangles: they are right, the rest is counted, nothing is written behind them
        got_tri, got_keys, n_triangles, n_skipped = run(sigma, iso, lo, h, first_ball - 3)
        assert (n_triangles, n_skipped) == (tri.shape[0], 1) and got_tri.shape[0] == first_ball - 3
        assert (got_keys == keys[:first_ball - 3]).all() and (got_tri == tri[:first_ball - 3].view(np.int32)).all()


def test_two_runs_are_bit_identical():
    sigma, iso, lo, h, tri, keys, _ = reference("non finite", _non_finite)
    a = run(sigma, iso, lo, h, tri.shape[0])
    b = run(sigma, iso, lo, h, tri.shape[0])
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2:] == b[2:]


@pytest.mark.parametrize("name", ["sphere", "torus", "noise"])
def test_the_kernels_own_surface_is_closed_and_oriented(name):
    """through ops.mesh_extract and ops.mesh_weld: every directed edge once and its reverse once, the Euler characteristic of the
    shape, a positive enclosed volume (the surface faces outwards) -- and the ball's within 3.5 % of 4/3 pi r^3 at 12^3, the
    float64 restatement's 3.40 % (tests/test_device_mesh_host.py)"""
    import torch

    from nerf_sampling_amd import ops

    sigma, lo, h = {"sphere": lambda: MR.sphere(12), "torus": lambda: MR.torus(20), "noise": MR.noise}[name]()
    dev = torch.from_numpy(sigma).cuda()
    got = ops.mesh_extract(dev, 0.0, lo, h)
    tri, keys = got["triangles"].cpu().numpy(), got["keys"].cpu().numpy()
    assert got["n_triangles"] == tri.shape[0] > 0 and got["n_skipped"] == 0
    paired, chi, volume = MR.invariants(tri, keys)
    print(f"{name}: {tri.shape[0]} triangles, chi {chi}, volume {volume}")
    assert paired and volume > 0
    if name == "sphere":
        assert chi == 2 and abs(volume / (4.0 / 3.0 * np.pi * 0.7 ** 3) - 1.0) < 0.035
    if name == "torus":
        assert chi == 0
    vertices, faces = ops.mesh_weld(got["triangles"], got["keys"])
    assert faces.dtype == torch.int64 and vertices.shape[0] == np.unique(keys).size
    v, f = vertices.cpu().numpy(), faces.cpu().numpy()
    assert (v[f].view(np.int32) == tri.view(np.int32)).all()
    ref_v, ref_f = MR.weld(tri, keys)
    assert (f == ref_f).all() and (v.view(np.int32) == ref_v.view(np.int32)).all()         # ascending key order
    # a capacity given: one call, cut to what fits, the full count reported
    few = ops.mesh_extract(dev, 0.0, lo, h, capacity=10)
    assert few["n_triangles"] == tri.shape[0] and torch.equal(few["triangles"], got["triangles"][:10])
    assert torch.equal(few["keys"], got["keys"][:10])
    column = torch.full(tuple(dev.shape) + (4,), float("nan"), device="cuda")
    column[..., 3] = dev
    again = ops.mesh_extract(column[..., 3], 0.0, lo, h, capacity=tri.shape[0] + 3)
    assert torch.equal(again["triangles"], got["triangles"]) and torch.equal(again["keys"], got["keys"])
