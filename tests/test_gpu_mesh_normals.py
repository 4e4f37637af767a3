"""ns_mesh_normals / ops.mesh_normals: per-vertex normals of the device mesh from the density lattice.
Yardstick (tests/mesh_normals_reference.py, numpy): the header's definition restated in float32 and float64 in the same order of
operations -- the normals' BITS and the two counts are equal --, and for the kernel's own normals on the kernel's own mesh the
side the triangles face, which neither the kernel nor the restatement defines.

S, the number of keys one workgroup owns, is the header's NS_MESH_NORMALS_SHARE.  Every call of ``run`` goes through the C ABI with
a workspace of exactly ns_mesh_normals_workspace_bytes, poisoned with 0xA5 and fenced by guard bytes, normals poisoned the same way
with PAD vertices behind them, and counters that hold garbage before the call."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_normals_reference as NR
import mesh_reference as MR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
PAD = 8                                                   # poisoned vertices behind normal_out
S = int(re.search(r"#define NS_MESH_NORMALS_SHARE (\d+)",
                  open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()).group(1))
H = (0.25, 0.125, 0.75)                                   # anisotropic, exact in fp32
DIMS = (7, 6, 9)
_reference = {}


def reference(name, make):
    """(sigma, iso, h, keys, normals, n_degenerate, n_invalid) of a named case: built and restated once, shared, never modified"""
    if name not in _reference:
        sigma, iso, h, keys = make()
        sigma = np.ascontiguousarray(sigma, dtype=np.float32)
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        normals, n_degenerate, n_invalid, _ = NR.normals(sigma, iso, h, keys)
        for a in (sigma, keys, normals):
            a.setflags(write=False)
        _reference[name] = (sigma, np.float32(iso), np.asarray(h, np.float32), keys, normals, n_degenerate, n_invalid)
    return _reference[name]


def run(sigma, iso, h, keys, stride=1):
    """One call through the C ABI -> (normal bits [V,3] int32, n_degenerate, n_invalid), after checking that nothing behind the
    normals, outside the workspace or behind the counters was written.  ``stride`` 4: sigma is the last column of a [., 4] array
    whose other columns are NaN."""
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
    V = int(keys.size)
    need = lib.ns_mesh_normals_workspace_bytes(V)
    assert need == (16 * ((V + S - 1) // S) + 255) // 256 * 256
    byte = lambda n: torch.full((n,), POISON, dtype=torch.uint8, device="cuda")           # noqa: E731
    ws = byte(need + 512)
    counters = byte(16 + 256)
    out = byte((V + PAD) * 12)
    key_dev = torch.from_numpy(np.array(keys, dtype=np.int64).reshape(-1)).cuda()
    p = lambda x: C.c_void_p(x.data_ptr())                                                # noqa: E731
    rc = lib.ns_mesh_normals(C.c_void_p(sigma_ptr), stride, Gx, Gy, Gz, float(iso), *(float(v) for v in h),
                             p(key_dev) if V else None, V, p(out), p(counters), C.c_void_p(ws.data_ptr() + 256),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ns_last_error()
    b = ws.cpu().numpy()
    assert (b[:256] == POISON).all() and (b[256 + need:] == POISON).all(), "written outside the workspace"
    c = counters.cpu().numpy()
    assert (c[16:] == POISON).all()
    n_degenerate, n_invalid = (int(v) for v in c[:16].view(np.int64))
    nb = out.cpu().numpy()
    assert (nb[V * 12:] == POISON).all(), "written behind normal_out"
    return nb[:V * 12].view(np.int32).reshape(V, 3), n_degenerate, n_invalid


def check(name, make, stride=1):
    sigma, iso, h, keys, normals, n_degenerate, n_invalid = reference(name, make)
    bits, got_degenerate, got_invalid = run(sigma, iso, h, keys, stride=stride)
    differ = (bits != normals.reshape(-1, 3).view(np.int32)).any(axis=1)
    print(f"{name}: lattice {sigma.shape[::-1]}, {keys.size} keys, {n_degenerate} degenerate, {n_invalid} invalid, "
          f"{int(differ.sum())} normals differ from the restatement")
    assert (got_degenerate, got_invalid) == (n_degenerate, n_invalid)
    assert not differ.any()
    return sigma, iso, h, keys, normals, n_degenerate, n_invalid


def _noise(dims, seed=3):
    Gx, Gy, Gz = dims
    return np.random.default_rng(seed).standard_normal((Gz, Gy, Gx)).astype(np.float32)


def _every_edge(dims=DIMS, seed=3):
    """normal noise without a border, every lattice edge there is: every boundary and every one-sided stencil occurs"""
    return lambda: (_noise(dims, seed), 0.1, H, NR.all_edge_keys(dims))


def test_every_edge_of_a_lattice_without_a_border():
    sigma, iso, h, keys, normals, n_degenerate, _ = check("every edge", _every_edge())
    assert keys.size == 2053 and n_degenerate == 0
    length = np.linalg.norm(normals.astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() < 2 * np.finfo(np.float32).eps
    _, a, b = NR.decode(keys, DIMS)
    far = np.array(DIMS) - 1
    assert ((a == 0).any(axis=1) & (b == far).any(axis=1)).any()                          # one-sided at both ends of one edge


def test_sigma_column_of_a_raw_array():
    check("every edge", _every_edge(), stride=4)


def test_a_lattice_two_points_wide():
    """Gx = 2: every x stencil is one-sided, xm = 0 and xp = 1 at both points"""
    sigma, iso, h, keys, *_ = check("Gx = 2", _every_edge((2, 5, 3), seed=5))
    assert keys.size > 100


def test_keys_shuffled_and_duplicated():
    def make():
        rng = np.random.default_rng(17)
        keys = NR.all_edge_keys(DIMS)
        keys = np.concatenate([keys, keys[::3], keys[:40], keys[:40]])
        return _noise(DIMS), 0.1, H, rng.permutation(keys)

    sigma, iso, h, keys, normals, *_ = check("shuffled", make)
    order = np.argsort(keys, kind="stable")
    same = keys[order][1:] == keys[order][:-1]
    bits = normals.view(np.int32)[order]
    assert same.sum() > 700 and (bits[1:][same] == bits[:-1][same]).all()                 # a function of the key alone


@pytest.mark.parametrize("V", [S - 1, S, S + 1, 2 * S + 1])
def test_share_boundaries(V):
    """the last workgroup owns a whole share, one key short of it, and ONE key"""
    check(f"tiled {V}", lambda: (_noise(DIMS), 0.1, H, np.resize(NR.all_edge_keys(DIMS)[::-1], V)))


def test_invalid_keys_among_valid_ones():
    bad = NR.invalid_keys(DIMS)

    def make():
        good = NR.all_edge_keys(DIMS)
        at = np.arange(bad.size) * 97 + 5                                                 # spread over three shares' steps
        return _noise(DIMS), 0.1, H, np.insert(good, at, bad)

    sigma, iso, h, keys, normals, n_degenerate, n_invalid = check("invalid", make)
    assert n_invalid == bad.size == 21 and n_degenerate == 0
    is_bad = ~NR.decode(keys, DIMS)[0]
    assert is_bad.sum() == bad.size and (normals[is_bad] == 0).all()
    # the neighbours of an invalid key keep the normals they have without it
    alone = reference("every edge", _every_edge())[4]
    assert (normals[~is_bad].view(np.int32) == alone.view(np.int32)).all()
    # nothing but invalid keys: no address is formed, every normal is zero
    bits, got_degenerate, got_invalid = run(sigma, iso, h, bad)
    assert (bits == 0).all() and (got_degenerate, got_invalid) == (0, bad.size)


def _poisoned():
    sigma = _noise(DIMS)
    sigma[4, 3, 3] = np.nan
    sigma[1, 1, 5] = np.inf
    sigma[7, 4, 1] = -np.inf
    return sigma, 0.1, H, NR.all_edge_keys(DIMS)


def test_nan_and_inf_in_a_stencil_neighbour():
    sigma, iso, h, keys, normals, n_degenerate, _ = check("non finite", _poisoned)
    _, a, b = NR.decode(keys, DIMS)
    ends_finite = np.isfinite(sigma[a[:, 2], a[:, 1], a[:, 0]]) & np.isfinite(sigma[b[:, 2], b[:, 1], b[:, 0]])
    zero = (normals == 0).all(axis=1)
    neighbour_only = zero & ends_finite                    # degenerate through a stencil neighbour that is no endpoint
    print(f"{int(zero.sum())} degenerate, {int(neighbour_only.sum())} of them with finite endpoints")
    assert n_degenerate == zero.sum() and neighbour_only.sum() >= 30 and (~ends_finite).sum() >= 30
    assert np.isfinite(normals).all() and (zero | (np.abs(normals).max(axis=1) > 0.5)).all()


def test_equal_endpoints_and_a_zero_gradient():
    def quantised():
        sigma = np.round(_noise(DIMS, seed=9) * 2).astype(np.float32) / 2
        return sigma, 0.25, H, NR.all_edge_keys(DIMS)

    sigma, iso, h, keys, normals, n_degenerate, _ = check("quantised", quantised)
    _, a, b = NR.decode(keys, DIMS)
    equal = sigma[a[:, 2], a[:, 1], a[:, 0]] == sigma[b[:, 2], b[:, 1], b[:, 0]]
    assert equal.sum() > 100 and (normals[equal] == 0).all() and n_degenerate >= equal.sum()

    def isolated():
        sigma = np.zeros((5, 5, 5), dtype=np.float32)
        sigma[2, 2, 2] = 3.0                                                              # s_a = iso among zeros: tt = -0, g_a = 0
        return sigma, 3.0, H, NR.all_edge_keys((5, 5, 5))

    sigma, iso, h, keys, normals, n_degenerate, _ = check("isolated", isolated)
    from_peak = keys // 8 == NR.lin(2, 2, 2, (5, 5, 5))
    assert from_peak.sum() == 7 and (normals[from_peak] == 0).all()
    assert n_degenerate == keys.size                       # everywhere else s_a == s_b == 0 or tt = 3 / 3 lands on a zero gradient


def test_no_keys_and_one_key():
    sigma = _noise(DIMS)
    bits, n_degenerate, n_invalid = run(sigma, 0.1, H, np.empty((0,), np.int64))
    assert bits.shape == (0, 3) and (n_degenerate, n_invalid) == (0, 0)
    check("one key", lambda: (_noise(DIMS), 0.1, H, NR.all_edge_keys(DIMS)[1000:1001]))


def test_two_runs_are_bit_identical_and_the_counters_are_overwritten():
    """run() poisons the counters before every call: equal counts twice means overwritten, not accumulated"""
    sigma, iso, h, keys, normals, n_degenerate, n_invalid = reference("non finite", _poisoned)
    a = run(sigma, iso, h, keys)
    b = run(sigma, iso, h, keys)
    assert (a[0] == b[0]).all() and a[1:] == b[1:] == (n_degenerate, n_invalid) and n_degenerate > 0


def test_the_kernels_normals_face_the_way_its_triangles_do():
    """through ops.mesh_extract, ops.mesh_weld and ops.mesh_normals on MR.sphere(24): the kernel's own normals against the
    area-weighted normals of the kernel's own triangles -- positive at every vertex (the restatement stands at 0.994) --, equal
    to the restatement's bits, in mesh_weld's vertex order; [n,3] keys keep their shape; a caller's workspace changes nothing"""
    import torch

    from nerf_sampling_amd import ops

    sigma, lo, h = MR.sphere(24)
    dev = torch.from_numpy(sigma).cuda()
    got = ops.mesh_extract(dev, 0.0, lo, h)
    vertices, faces = ops.mesh_weld(got["triangles"], got["keys"])
    unique = torch.unique(got["keys"])
    shaded = ops.mesh_normals(dev, 0.0, h, unique)
    normals = shaded["normals"].cpu().numpy()
    assert normals.shape == (vertices.shape[0], 3) and (shaded["n_degenerate"], shaded["n_invalid"]) == (0, 0)
    geometric = NR.geometric_normals(vertices.cpu().numpy(), faces.cpu().numpy())
    dots = np.einsum("ij,ij->i", normals.astype(np.float64), geometric)
    print(f"sphere: {normals.shape[0]} vertices, smallest dot {dots.min():.4f}")
    assert dots.min() > 0
    want = NR.normals(sigma, 0.0, h, unique.cpu().numpy())[0]
    assert (normals.view(np.int32) == want.view(np.int32)).all()
    per_corner = ops.mesh_normals(dev, 0.0, h, got["keys"])["normals"]
    assert per_corner.shape == tuple(got["keys"].shape) + (3,) and torch.equal(per_corner, shaded["normals"][faces])
    ws = torch.full((ops.mesh_normals_workspace_bytes(unique.numel()),), 0xFF, dtype=torch.uint8, device="cuda")
    again = ops.mesh_normals(dev, 0.0, h, unique, workspace=ws)
    assert torch.equal(again["normals"], shaded["normals"]) and again["n_degenerate"] == 0
    column = torch.full(tuple(dev.shape) + (4,), float("nan"), device="cuda")
    column[..., 3] = dev
    assert torch.equal(ops.mesh_normals(column[..., 3], 0.0, h, unique)["normals"], shaded["normals"])
    with pytest.raises(ValueError):
        ops.mesh_normals(dev, 0.0, h, unique.int())
    with pytest.raises(ValueError):
        ops.mesh_normals(dev, 0.0, (h[0], 0.0, h[2]), unique)
    with pytest.raises(ValueError):
        ops.mesh_normals(dev, 0.0, h, unique, workspace=ws[1:])
