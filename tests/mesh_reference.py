"""The numpy statement of ns_mesh_extract (include/nerf_sampling_hip.h: marching tetrahedra on the Kuhn split), shared by
tests/test_gpu_mesh_extract.py (the kernel), tests/test_gpu_device_mesh.py (the layers above it) and
tests/test_device_mesh_host.py (hand cases and the surface's invariants, without a GPU).

``march(sigma, iso, lo, h, dtype)`` restates the header's definition with every operation in ``dtype`` and in the header's
order: float32 gives the kernel's triangle count, order, keys and position bits; float64 is the same surface without fp32's
rounding.  The case table is derived here from the geometric rule in floating point, not copied from the library's.
``invariants(triangles, keys)`` judges a surface by what neither the kernel nor this restatement defines: every directed edge once
and its reverse once, the Euler characteristic and the enclosed volume."""

import itertools

import numpy as np

PERMS = list(itertools.permutations(range(3)))           # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx


def tet_codes(t):
    """corner codes dx + 2 dy + 4 dz of w0 .. w3 of tetrahedron t"""
    p = PERMS[t]
    return [0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7]


def _corner(code):
    return np.array([code & 1, (code >> 1) & 1, code >> 2], dtype=np.float64)


def tet_case(t, mask):
    """the triangles of tetrahedron t whose inside corners are the set bits of ``mask``: a list of triangles, each three lattice
    edges (inside corner, outside corner) as corner numbers 0 .. 3, wound from inside to outside"""
    inside = [q for q in range(4) if (mask >> q) & 1]
    outside = [q for q in range(4) if not (mask >> q) & 1]
    if len(inside) in (0, 4):
        return []
    if len(inside) == 1:
        tris = [[(inside[0], b) for b in outside]]
    elif len(inside) == 3:
        tris = [[(a, outside[0]) for a in inside]]
    else:
        (a0, a1), (b0, b1) = inside, outside
        quad = [(a0, b0), (a0, b1), (a1, b1), (a1, b0)]
        tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    w = [_corner(c) for c in tet_codes(t)]
    outward = np.mean([w[q] for q in outside], axis=0) - np.mean([w[q] for q in inside], axis=0)
    out = []
    for tri in tris:
        m = [0.5 * (w[a] + w[b]) for a, b in tri]
        d = float(np.dot(np.cross(m[1] - m[0], m[2] - m[0]), outward))
        assert abs(d) > 1e-6                                # never degenerate: the midpoints span a plane across the tetrahedron
        out.append(tri if d > 0 else [tri[0], tri[2], tri[1]])
    return out


def march(sigma, iso, lo, h, dtype=np.float32):
    """-> (triangles [n,3,3] ``dtype``, keys [n,3] int64, n_skipped) of the lattice ``sigma`` [Gz,Gy,Gx]"""
    s = np.asarray(sigma, dtype=dtype)
    Gz, Gy, Gx = s.shape
    assert min(Gx, Gy, Gz) >= 2
    iso = dtype(iso)
    lo, h = np.asarray(lo, dtype=dtype), np.asarray(h, dtype=dtype)
    k, j, i = (a.reshape(-1) for a in np.meshgrid(np.arange(Gz - 1), np.arange(Gy - 1), np.arange(Gx - 1), indexing="ij"))
    idx = (i, j, k)                                         # the flat order of the cells is e
    val = [s[k + (c >> 2), j + ((c >> 1) & 1), i + (c & 1)] for c in range(8)]
    finite = np.all([np.isfinite(v) for v in val], axis=0)
    with np.errstate(invalid="ignore"):
        inside = [(v >= iso) & finite for v in val]
    lin0 = (k.astype(np.int64) * Gy + j) * Gx + i
    off = [(c & 1) + ((c >> 1) & 1) * Gx + (c >> 2) * Gx * Gy for c in range(8)]
    rec_e, rec_t, rec_n, rec_p, rec_k = [], [], [], [], []
    for t in range(6):
        codes = tet_codes(t)
        mask = sum(inside[codes[q]].astype(np.int64) << q for q in range(4))
        for m in range(1, 15):
            cells = np.nonzero(mask == m)[0]
            if cells.size == 0:
                continue
            for n, tri in enumerate(tet_case(t, m)):
                P = np.empty((cells.size, 3, 3), dtype=dtype)
                K = np.empty((cells.size, 3), dtype=np.int64)
                for v, (qa, qb) in enumerate(tri):
                    ca, cb = sorted((codes[qa], codes[qb]))             # the codes grow with the lattice index
                    sa, sb = val[ca][cells], val[cb][cells]
                    with np.errstate(all="ignore"):
                        tt = (iso - sa) / (sb - sa)
                        for a in range(3):
                            pa = lo[a] + (idx[a][cells] + ((ca >> a) & 1)).astype(dtype) * h[a]
                            pb = lo[a] + (idx[a][cells] + ((cb >> a) & 1)).astype(dtype) * h[a]
                            P[:, v, a] = pa + tt * (pb - pa)
                    K[:, v] = (lin0[cells] + off[ca]) * 8 + (cb ^ ca)
                rec_e.append(cells), rec_t.append(np.full(cells.size, t)), rec_n.append(np.full(cells.size, n))
                rec_p.append(P), rec_k.append(K)
    n_skipped = int((~finite).sum())
    if not rec_e:
        return np.empty((0, 3, 3), dtype=dtype), np.empty((0, 3), dtype=np.int64), n_skipped
    e, t, n = np.concatenate(rec_e), np.concatenate(rec_t), np.concatenate(rec_n)
    order = np.lexsort((n, t, e))
    return np.concatenate(rec_p)[order], np.concatenate(rec_k)[order], n_skipped


def weld(triangles, keys):
    """-> (vertices [V,3] in ascending key order, faces [F,3] int64): ops.mesh_weld on the host"""
    u, first, inv = np.unique(np.asarray(keys).reshape(-1), return_index=True, return_inverse=True)
    return np.asarray(triangles).reshape(-1, 3)[first], inv.reshape(-1, 3).astype(np.int64)


def invariants(triangles, keys):
    """-> (paired, chi, volume): whether every directed edge (by key) occurs once and its reverse once, V - E + F with E the
    number of undirected edges, and the signed volume 1/6 sum p0 . (p1 x p2) in float64"""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    u, inv = np.unique(keys.reshape(-1), return_inverse=True)
    F = inv.reshape(-1, 3).astype(np.int64)
    V = int(u.size)
    a = np.concatenate([F[:, 0], F[:, 1], F[:, 2]])
    b = np.concatenate([F[:, 1], F[:, 2], F[:, 0]])
    directed, counts = np.unique(a * V + b, return_counts=True)
    reverse = np.unique(b * V + a)
    paired = bool((counts == 1).all() and directed.size == reverse.size and (directed == reverse).all() and (a != b).all())
    p = np.asarray(triangles, dtype=np.float64).reshape(-1, 3, 3)
    volume = float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
    return paired, V - directed.size // 2 + F.shape[0], volume


# ---- the lattices the tests share -------------------------------------------------------------------------------------------
def axes(G, bound=1.0):
    """(lo [3], h [3]) in float32 of a G^3 lattice on [-bound, bound]^3, and the float64 coordinates of its points per axis"""
    lo = np.full(3, -bound, dtype=np.float32)
    h = np.full(3, np.float32(2.0 * bound / (G - 1)), dtype=np.float32)
    return lo, h, lo[0].astype(np.float64) + np.arange(G) * h[0].astype(np.float64)


def sphere(G, radius=0.7):
    """sigma = radius - |p|, iso 0: inside the ball"""
    lo, h, ax = axes(G)
    Z, Y, X = np.meshgrid(ax, ax, ax, indexing="ij")
    return (radius - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32), lo, h


def torus(G=20, R=0.6, r=0.25):
    lo, h, ax = axes(G)
    Z, Y, X = np.meshgrid(ax, ax, ax, indexing="ij")
    return (r - np.sqrt((np.sqrt(X * X + Y * Y) - R) ** 2 + Z * Z)).astype(np.float32), lo, h


def noise(shape=(7, 6, 9), seed=0):
    """normal values, a border of -1 and one interior corner exactly at the iso value 0"""
    s = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    s[0] = s[-1] = -1
    s[:, 0] = s[:, -1] = -1
    s[:, :, 0] = s[:, :, -1] = -1
    s[shape[0] // 2, shape[1] // 2, shape[2] // 2] = 0.0
    return s, np.zeros(3, np.float32), np.ones(3, np.float32)
