"""The contract of ns_mesh_components (include/nerf_sampling_hip.h) restated as a plain union-find on the host, and the small
meshes the component tests share.  Integers only: every comparison with it is exact."""

import numpy as np


def components(faces, n_vertices):
    """(labels [V] int32, tri_count [V] int32, vert_count [V] int32, n_components, n_ignored): a face with an index outside
    [0, V) joins nothing and is counted; label[v] is the smallest vertex of v's component; the counts stand at the roots"""
    V = int(n_vertices)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    valid = ((faces >= 0) & (faces < V)).all(axis=1)
    for a, b, c in faces[valid].tolist():
        for u, w in ((a, b), (a, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)                  # the smaller index stays the root
    labels = np.fromiter((find(v) for v in range(V)), dtype=np.int32, count=V)
    vert_count = np.bincount(labels, minlength=V).astype(np.int32)
    tri_count = np.bincount(labels[faces[valid][:, 0]], minlength=V).astype(np.int32)
    n_components = int((labels == np.arange(V)).sum())
    return labels, tri_count, vert_count, n_components, int((~valid).sum())


def strip(n_faces):
    """a triangle strip: face f = (f, f + 1, f + 2) on n_faces + 2 vertices"""
    f = np.arange(n_faces, dtype=np.int64)
    return np.stack([f, f + 1, f + 2], axis=1)


# (name, faces, V, labels, triangles at the roots, vertices at the roots, n_components, n_ignored), worked out by hand
HAND_CASES = [
    ("two disjoint triangles", [(0, 1, 2), (3, 4, 5)], 6, [0, 0, 0, 3, 3, 3], {0: 1, 3: 1}, {0: 3, 3: 3}, 2, 0),
    ("two triangles sharing one vertex", [(0, 1, 2), (2, 3, 4)], 5, [0, 0, 0, 0, 0], {0: 2}, {0: 5}, 1, 0),
    ("two triangles sharing an edge", [(3, 1, 2), (2, 1, 0)], 4, [0, 0, 0, 0], {0: 2}, {0: 4}, 1, 0),
    ("a vertex in no face", [(0, 2, 3)], 5, [0, 1, 0, 0, 4], {0: 1}, {0: 3, 1: 1, 4: 1}, 3, 0),
    ("a face (a, a, b)", [(1, 1, 3), (2, 2, 2)], 4, [0, 1, 2, 1], {1: 1, 2: 1}, {0: 1, 1: 2, 2: 1}, 3, 0),
    ("faces with index V and -1", [(0, 1, 5), (2, -1, 3), (3, 4, 4)], 5, [0, 1, 2, 3, 3], {3: 1}, {0: 1, 1: 1, 2: 1, 3: 2}, 4, 2),
]


def hand_case(case):
    """(faces [F,3] int64, V, labels, tri_count, vert_count, n_components, n_ignored) of one HAND_CASES entry as arrays"""
    _, faces, V, labels, tri, vert, n_components, n_ignored = case
    tri_count, vert_count = np.zeros(V, np.int32), np.zeros(V, np.int32)
    for r, n in tri.items():
        tri_count[r] = n
    for r, n in vert.items():
        vert_count[r] = n
    return np.asarray(faces, np.int64).reshape(-1, 3), V, np.asarray(labels, np.int32), tri_count, vert_count, n_components, n_ignored
