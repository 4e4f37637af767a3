"""ns_mesh_simplify and ops.mesh_simplify restated in numpy, from the header's definitions: the yardstick of
tests/test_mesh_simplify_host.py and tests/test_gpu_mesh_simplify.py, never a fallback.  float64 throughout, every operation its
own numpy call (numpy contracts nothing), integers in int64: the tests compare bits.

The clamp is written as the definition has it -- round first, clamp afterwards, in float64 so that nothing overflows -- not as
csrc/ns_mesh_cluster.h has it (clamp first): the two must agree."""

import numpy as np

FRAC = 16
ONE = 65536.0
MAX_DIM = 1 << 15
MAX_CELLS = 1 << 24


def lattice(lo, cell, dims):
    lo, cell = np.asarray(lo, dtype=np.float32), np.asarray(cell, dtype=np.float32)
    dims = np.asarray(dims, dtype=np.int64)
    assert lo.shape == cell.shape == dims.shape == (3,)
    assert np.isfinite(lo).all() and np.isfinite(cell).all() and (cell > 0).all()
    assert (dims >= 1).all() and (dims <= MAX_DIM).all() and int(dims.prod()) <= MAX_CELLS
    return lo, cell, dims


def coords(vertices, lo, cell, dims):
    """-> (u int64 [V,3], cell index int64 [V] (-1 for a non-finite vertex), finite bool [V])"""
    lo, cell, dims = lattice(lo, cell, dims)
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    finite = np.isfinite(v).all(axis=1)
    with np.errstate(all="ignore"):
        diff = v.astype(np.float64) - lo.astype(np.float64)[None, :]
        quot = diff / cell.astype(np.float64)[None, :]
        t = quot * ONE
        r = np.rint(t)                                                       # round half to even, as llrint
        top = (dims * 65536 - 1).astype(np.float64)[None, :]
        r = np.minimum(np.maximum(r, 0.0), top)
    u = np.where(finite[:, None], np.where(np.isnan(r), 0.0, r), 0.0).astype(np.int64)
    c = u >> FRAC
    lin = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    return u, np.where(finite, lin, -1), finite


def distance2(u, S, n):
    """d32 float32 [...] of members with coordinates u [...,3] in clusters with sums S [...,3] and counts n [...]"""
    mean = np.asarray(S, dtype=np.int64).astype(np.float64) / np.asarray(n, dtype=np.int64).astype(np.float64)[..., None]
    diff = np.asarray(u, dtype=np.int64).astype(np.float64) - mean
    sq = diff * diff
    return ((sq[..., 0] + sq[..., 1]) + sq[..., 2]).astype(np.float32)


def clusters(vertices, lo, cell, dims):
    """-> dict(u, lin, finite, S int64 [cells,3], n int32 [cells], d32 float32 [V], word uint64 [V], rep int32 [V],
    n_nonfinite, n_clusters)"""
    u, lin, finite = coords(vertices, lo, cell, dims)
    V, cells = u.shape[0], int(np.prod(np.asarray(dims, dtype=np.int64)))
    S, n = np.zeros((cells, 3), dtype=np.int64), np.zeros((cells,), dtype=np.int64)
    members = np.flatnonzero(finite)
    np.add.at(S, lin[members], u[members])
    np.add.at(n, lin[members], 1)
    d32 = np.zeros((V,), dtype=np.float32)
    d32[members] = distance2(u[members], S[lin[members]], n[lin[members]])
    word = (d32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(V, dtype=np.uint64)
    best = np.full((cells,), np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(best, lin[members], word[members])
    rep = np.full((V,), -1, dtype=np.int32)
    rep[members] = (best[lin[members]] & np.uint64(0xFFFFFFFF)).astype(np.int64).astype(np.int32)
    return dict(u=u, lin=lin, finite=finite, S=S, n=n.astype(np.int32), d32=d32, word=word, rep=rep,
                n_nonfinite=int(V - members.size), n_clusters=int((n > 0).sum()))


def map_faces(faces, rep, capacity=None):
    """-> (faces_out int64 [min(kept, capacity),3] in the input numbering, counters): the header's order of judgement"""
    faces = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    V = rep.shape[0]
    valid = ((faces >= 0) & (faces < V)).all(axis=1)
    r = np.zeros(faces.shape, dtype=np.int64)                                # V == 0: no face is valid
    if V:
        r = np.where(valid[:, None], rep[np.clip(faces, 0, V - 1)], 0).astype(np.int64)
    on_nonfinite = valid & (r < 0).any(axis=1)
    rest = valid & ~on_nonfinite
    collapsed = rest & ((r[:, 0] == r[:, 1]) | (r[:, 0] == r[:, 2]) | (r[:, 1] == r[:, 2]))
    kept = rest & ~collapsed
    out = r[kept]
    counters = dict(n_kept=int(kept.sum()), n_collapsed=int(collapsed.sum()), n_invalid=int((~valid).sum()),
                    n_nonfinite_faces=int(on_nonfinite.sum()))
    return (out if capacity is None else out[:capacity]), counters


def entry(vertices, faces, lo, cell, dims, capacity=None):
    """what ns_mesh_simplify writes: (rep int32 [V], faces_out int64, count int64 [6])"""
    c = clusters(vertices, lo, cell, dims)
    out, k = map_faces(faces, c["rep"], capacity)
    count = np.array([k["n_kept"], k["n_collapsed"], k["n_invalid"], c["n_nonfinite"], k["n_nonfinite_faces"], c["n_clusters"]],
                     dtype=np.int64)
    return c["rep"], out, count


def renumber(rep, faces_out):
    """-> (kept bool [V], index int64 [V], faces renumbered): the representatives in ascending input index"""
    V = rep.shape[0]
    kept = rep.astype(np.int64) == np.arange(V)
    index = np.where(kept, np.cumsum(kept) - 1, -1).astype(np.int64)
    return kept, index, index[faces_out].reshape(-1, 3)


def dedupe(faces):
    """-> (faces without those whose vertex set occurred earlier, n_duplicate): the first occurrence stays, with its winding"""
    seen, keep = set(), []
    for f in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        key = tuple(sorted(f))
        keep.append(key not in seen)
        seen.add(key)
    keep = np.array(keep, dtype=bool)
    return np.asarray(faces, dtype=np.int64).reshape(-1, 3)[keep], int((~keep).sum())


def simplify(vertices, faces, lo, cell, dims, dedupe_faces=True):
    """ops.mesh_simplify on the host -> dict(vertices, faces, index, rep, counters ...)"""
    vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    rep, out, count = entry(vertices, faces, lo, cell, dims)
    kept, index, new_faces = renumber(rep, out)
    n_duplicate = 0
    if dedupe_faces:
        new_faces, n_duplicate = dedupe(new_faces)
    return dict(vertices=vertices[kept], faces=new_faces, index=index, rep=rep, n_collapsed=int(count[1]), n_invalid=int(count[2]),
                n_nonfinite=int(count[3]), n_nonfinite_faces=int(count[4]), n_duplicate=n_duplicate, n_clusters=int(count[5]))


def signed_volume(vertices, faces):
    """1/6 sum p0 . (p1 x p2) in float64"""
    p = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def surface_area(vertices, faces):
    p = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    return float(np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum() / 2.0)


# ---- cases worked out by hand ------------------------------------------------------------------------------------------------
# name -> (vertices, faces, lo, cell, dims, rep, faces_out (input numbering), count [6], then ops.mesh_simplify's: index,
# faces renumbered and deduped, n_duplicate)
_A = 1.0 - 2.0 ** -17                                     # t = 65535.5: half way, rounds to the even 65536 -> cell 1
_B = 1.0 - 3.0 * 2.0 ** -17                               # t = 65534.5: rounds to the even 65534 -> cell 0
HAND_CASES = [
    # two members at 0.25 and 0.75 of the one cell: S_x = 16384 + 49152, the mean 32768, both d = 16384^2 = 2^28 -> index 0;
    # the face on them collapses to a point
    ("tie", [(0.25, 0.5, 0.5), (0.75, 0.5, 0.5)], [(0, 1, 0)], (0, 0, 0), (1, 1, 1), (1, 1, 1),
     [0, 0], [], [0, 1, 0, 0, 0, 1], [0, -1], [], 0),
    # u_x = 8192, 32768, 40960: the mean is 27306.67 and the middle one, index 1, is 5461.33 from it
    ("nearest the centroid", [(0.125, 0.5, 0.5), (0.5, 0.5, 0.5), (0.625, 0.5, 0.5)], [(0, 1, 2), (2, 1, 0)], (0, 0, 0),
     (1, 1, 1), (1, 1, 1), [1, 1, 1], [], [0, 2, 0, 0, 0, 1], [-1, 0, -1], [], 0),
    # a 2 x 2 x 1 lattice of unit cells.  x = 1 exactly: u = 65536, cell 1; _A rounds up into cell 1, _B down into cell 0;
    # x = -3 clamps to u = 0 (cell 0), x = 7 to u = 131071 (cell 1); a NaN and an infinite vertex; (0.5, 1.5) alone in cell 2.
    # cell 1 = {0, 1, 4}: u_x = 65536, 65536, 131071, the mean 87381, d = 21845^2 twice -> index 0.
    # cell 0 = {2, 3}: u_x = 65534, 0, the mean 32767, d = 32767^2 twice -> index 2.
    ("boundary, clamp, non-finite, bad faces",
     [(1.0, 0.5, 0.5), (_A, 0.5, 0.5), (_B, 0.5, 0.5), (-3.0, 0.5, 0.5), (7.0, 0.5, 0.5), (np.nan, 0.5, 0.5),
      (0.5, np.inf, 0.5), (0.5, 1.5, 0.5)],
     [(0, 2, 5),            # on the NaN vertex
      (0, 1, 2),            # (0, 0, 2): collapses to an edge
      (0, 1, 4),            # (0, 0, 0): collapses to a point
      (-1, 0, 2), (0, 2, 8),   # indices -1 and V
      (0, 2, 7),            # kept as it is
      (6, 6, -1),           # invalid comes first: not counted as on a non-finite vertex
      (4, 3, 7),            # kept: (0, 2, 7) again
      (7, 3, 1),            # kept: (7, 2, 0), the same set with the other winding
      (6, 0, 7)],           # on the infinite vertex
     (0, 0, 0), (1, 1, 1), (2, 2, 1),
     [0, 0, 2, 2, 0, -1, -1, 7], [(0, 2, 7), (0, 2, 7), (7, 2, 0)], [3, 2, 3, 2, 2, 3],
     [0, -1, 1, -1, -1, -1, -1, 2], [(0, 1, 2)], 2),
    ("no vertices", [], [(0, 1, 2), (0, 0, 0)], (0, 0, 0), (1, 1, 1), (2, 2, 2), [], [], [0, 0, 2, 0, 0, 0], [], [], 0),
    ("no faces", [(0.5, 0.5, 0.5)], [], (0, 0, 0), (1, 1, 1), (1, 1, 1), [0], [], [0, 0, 0, 0, 0, 1], [0], [], 0),
    ("nothing", [], [], (0, 0, 0), (1, 1, 1), (1, 1, 1), [], [], [0, 0, 0, 0, 0, 0], [], [], 0),
]


def hand_case(case):
    name, vertices, faces, lo, cell, dims, rep, faces_out, count, index, new_faces, n_duplicate = case
    return (np.array(vertices, dtype=np.float32).reshape(-1, 3), np.array(faces, dtype=np.int64).reshape(-1, 3), lo, cell, dims,
            np.array(rep, dtype=np.int32), np.array(faces_out, dtype=np.int64).reshape(-1, 3), np.array(count, dtype=np.int64),
            np.array(index, dtype=np.int64), np.array(new_faces, dtype=np.int64).reshape(-1, 3), n_duplicate)


def soup(V=5000, F=10000, seed=0, bad=7, nonfinite=5, box=(-0.3, 8.3)):
    """a random soup on an 8^3 lattice of unit cells from 0: some vertices outside it, a few non-finite, a few faces out of range"""
    rng = np.random.default_rng(seed)
    vertices = rng.uniform(box[0], box[1], size=(V, 3)).astype(np.float32)
    c = np.floor(vertices)
    vertices = vertices[np.lexsort((c[:, 0], c[:, 1], c[:, 2]))]              # neighbouring indices mostly share a cell
    rows = rng.choice(V, size=nonfinite, replace=False)
    vertices[rows, rng.integers(0, 3, size=nonfinite)] = rng.choice([np.nan, np.inf, -np.inf], size=nonfinite)
    faces = rng.integers(0, V, size=(F, 3), dtype=np.int64)
    near = rng.choice(F, size=F // 2, replace=False)                          # half the faces on neighbouring indices
    faces[near, 1] = (faces[near, 0] + rng.integers(1, 6, size=near.size)) % V
    rows = rng.choice(F, size=bad, replace=False)
    faces[rows, rng.integers(0, 3, size=bad)] = rng.choice([-1, V, V + 1, -2 ** 40, 2 ** 40, 2 ** 31, 2 ** 32 + 7], size=bad)
    return vertices, faces
