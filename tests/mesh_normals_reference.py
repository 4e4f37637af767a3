"""The numpy statement of ns_mesh_normals (include/nerf_sampling_hip.h: the lattice's finite-difference gradient interpolated
along a vertex's own lattice edge), shared by tests/test_mesh_normals_host.py (the definition's properties, without a GPU),
tests/test_gpu_mesh_normals.py (the kernel) and tests/test_gpu_device_mesh_normals.py (the layers above it).

``normals(sigma, iso, h, keys)`` restates the header's definition with every operation in the header's format and order: float32
up to the gradient at the vertex, float64 for the length and the division, one rounding to float32 at the end -- the kernel's
bits and counts.  ``geometric_normals(vertices, faces)`` is what the definition does not use: the area-weighted normals of the
triangles around a vertex, in float64, for orientation checks only."""

import numpy as np


def decode(keys, dims):
    """-> (valid bool [n], a int64 [n,3], b int64 [n,3]) of the keys on a lattice of dims = (Gx, Gy, Gz); a and b are (i, j, k)
    and mean nothing where the key is not valid"""
    Gx, Gy, Gz = (int(g) for g in dims)
    keys = np.asarray(keys, dtype=np.int64).reshape(-1)
    lin, code = keys >> 3, keys & 7
    valid = (keys >= 0) & (lin < Gx * Gy * Gz) & (code != 0)
    lin = np.where(valid, lin, 0)
    a = np.stack([lin % Gx, lin // Gx % Gy, lin // (Gx * Gy)], axis=1)
    b = a + np.stack([code & 1, (code >> 1) & 1, code >> 2], axis=1)
    valid = valid & (b < np.array([Gx, Gy, Gz])).all(axis=1)
    return valid, a, b


def lin(i, j, k, dims):
    return (k * dims[1] + j) * dims[0] + i


def invalid_keys(dims):
    """the keys the header refuses on a lattice of dims = (Gx, Gy, Gz), each for one reason: code 0 at an interior point, b one
    past each far face (from the far corner's neighbours and from the far corner itself), lin equal to and beyond the lattice
    size, negative keys"""
    Gx, Gy, Gz = dims
    far = (Gx - 1, Gy - 1, Gz - 1)
    keys = [lin(1, 1, 1, dims) * 8 + 0,
            lin(far[0], 1, 1, dims) * 8 + 1, lin(1, far[1], 1, dims) * 8 + 2, lin(1, 1, far[2], dims) * 8 + 4,
            lin(far[0], 1, 1, dims) * 8 + 7, lin(1, far[1], 1, dims) * 8 + 3, lin(1, 1, far[2], dims) * 8 + 6,
            lin(*far, dims) * 8 + 1, lin(*far, dims) * 8 + 2, lin(*far, dims) * 8 + 4, lin(*far, dims) * 8 + 7,
            Gx * Gy * Gz * 8 + 1, Gx * Gy * Gz * 8 + 7, (Gx * Gy * Gz + 5) * 8 + 2, 2 ** 34 + 1, 2 ** 62 + 3, 2 ** 63 - 1,
            -1, -8, -7, -2 ** 63]
    return np.array(keys, dtype=np.int64)


def all_edge_keys(dims):
    """every valid key of the lattice, ascending: all seven codes at every point whose far end lies inside"""
    Gx, Gy, Gz = dims
    keys = np.arange(Gx * Gy * Gz * 8, dtype=np.int64)
    return keys[decode(keys, dims)[0]]


def nodal_gradient(s, q, h):
    """the float32 gradient [n,3] of the lattice ``s`` [Gz,Gy,Gx] float32 at the lattice points q [n,3] = (i, j, k): central where
    both neighbours exist, one-sided on the boundary"""
    G = (s.shape[2], s.shape[1], s.shape[0])
    g = np.empty((q.shape[0], 3), dtype=np.float32)
    for x in range(3):
        xm, xp = np.maximum(q[:, x] - 1, 0), np.minimum(q[:, x] + 1, G[x] - 1)
        lo, hi = q.copy(), q.copy()
        lo[:, x], hi[:, x] = xm, xp
        with np.errstate(all="ignore"):
            diff = s[hi[:, 2], hi[:, 1], hi[:, 0]] - s[lo[:, 2], lo[:, 1], lo[:, 0]]
            g[:, x] = diff / ((xp - xm).astype(np.float32) * np.float32(h[x]))
    return g


def normals(sigma, iso, h, keys):
    """-> (normals float32 keys.shape + (3,), n_degenerate, n_invalid, length float64 keys.shape) of the lattice ``sigma``
    [Gz,Gy,Gx]; ``length`` is the fp64 length of the gradient at the vertex (0 where the key is invalid)"""
    s = np.asarray(sigma, dtype=np.float32)
    assert s.ndim == 3 and min(s.shape) >= 2
    shape = np.asarray(keys).shape
    valid, a, b = decode(keys, (s.shape[2], s.shape[1], s.shape[0]))
    a, b = np.where(valid[:, None], a, 0), np.where(valid[:, None], b, 0)
    iso = np.float32(iso)
    h = np.asarray(h, dtype=np.float32)
    sa, sb = s[a[:, 2], a[:, 1], a[:, 0]], s[b[:, 2], b[:, 1], b[:, 0]]
    ga, gb = nodal_gradient(s, a, h), nodal_gradient(s, b, h)
    with np.errstate(all="ignore"):
        tt = (iso - sa) / (sb - sa)
        g = ga + tt[:, None] * (gb - ga)
        assert g.dtype == np.float32 and tt.dtype == np.float32
        G = g.astype(np.float64)
        length = np.sqrt(G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1] + G[:, 2] * G[:, 2])
        degenerate = ~(np.isfinite(sa) & np.isfinite(sb) & np.isfinite(tt) & np.isfinite(g).all(axis=1)) | (length == 0)
        n = (-G / length[:, None]).astype(np.float32)
    degenerate &= valid
    n[degenerate | ~valid] = 0.0
    length = np.where(valid, length, 0.0)
    return n.reshape(shape + (3,)), int(degenerate.sum()), int((~valid).sum()), length.reshape(shape)


def geometric_normals(vertices, faces):
    """-> unit normals float64 [V,3]: the sum of (p1 - p0) x (p2 - p0) over the faces around a vertex (twice their area each),
    normalised; a vertex whose sum is zero keeps zeros"""
    p = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    cross = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    total = np.zeros_like(p)
    for v in range(3):
        np.add.at(total, f[:, v], cross)
    length = np.linalg.norm(total, axis=1, keepdims=True)
    return np.divide(total, length, out=np.zeros_like(total), where=length > 0)
