"""The numpy statement of ns_mesh_raster (include/nerf_sampling_hip.h: the device mesh rasterised from a pinhole camera), shared by
tests/test_mesh_raster_host.py (the definition's properties, without a GPU), tests/test_gpu_mesh_raster.py (the kernel, bit for
bit) and tests/test_gpu_device_mesh_eval.py (the layers above it).

Everything is written from the header, not from the kernel: the projection in float32 operation by operation, np.rint for the
snapping, the edge functions in int64 as the header spells them (the kernel evaluates an expanded form), float64 depth and
colour, and a lexicographic minimum over (depth bits, face index)."""

import numpy as np

SUB = 256                       # sub-pixel steps per pixel
BAND = 2.0 ** 20                # |x|, |y| of a usable vertex, in pixels
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def project(vertices, c2w, fx, fy, cx, cy, dtype=np.float32):
    """-> (x, y, z) of every vertex in ``dtype``, each operation rounded on its own: e = p - t, q = R^T e added left to right,
    z = -q_2, x = cx + fx (q_0 / z), y = cy - fy (q_1 / z).  float64: the same expression for the analytic checks."""
    p = np.asarray(vertices, dtype=dtype).reshape(-1, 3)
    c2w = np.asarray(c2w, dtype=dtype).reshape(3, 4)
    fx, fy, cx, cy = (dtype(v) for v in (fx, fy, cx, cy))
    r, t = c2w[:, :3], c2w[:, 3]
    with np.errstate(all="ignore"):
        e = [p[:, c] - t[c] for c in range(3)]
        q = [(e[0] * r[0, k] + e[1] * r[1, k]) + e[2] * r[2, k] for k in range(3)]
        z = -q[2]
        x = cx + fx * (q[0] / z)
        y = cy - fy * (q[1] / z)
    return x, y, z


def snap(x, y, z, near):
    """-> (X, Y int64, usable bool): eight sub-pixel bits, round half to even; unusable vertices get X = Y = 0"""
    with np.errstate(all="ignore"):
        usable = (np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~(z < np.float32(near))
                  & ~(np.abs(x) > np.float32(BAND)) & ~(np.abs(y) > np.float32(BAND)))
        X = np.where(usable, np.rint(x * np.float32(SUB)), 0).astype(np.int64)
        Y = np.where(usable, np.rint(y * np.float32(SUB)), 0).astype(np.int64)
    return X, Y, usable


def edge(ax, ay, bx, by, px, py):
    """E_AB(P) in int64 (python ints and int64 arrays: no overflow below 2^63)"""
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def tie_owned(dx, dy):
    """the top-left rule for the edge direction d = sign(area2) * (B - A): a centre exactly on the edge is covered iff ..."""
    return dy < 0 or (dy == 0 and dx > 0)


def face_coverage(P, area2, px, py):
    """-> (covered bool, [w_0, w_1, w_2]) of the snapped triangle P = [(X, Y)] * 3 at the points (px, py) (int64 arrays)"""
    sg = 1 if area2 > 0 else -1
    w, cov = [], np.ones(np.broadcast(px, py).shape, dtype=bool)
    for k in range(3):
        (ax, ay), (bx, by) = P[(k + 1) % 3], P[(k + 2) % 3]
        wk = edge(ax, ay, bx, by, px, py)
        w.append(wk)
        v = sg * wk
        cov &= (v > 0) | ((v == 0) & tie_owned(sg * (bx - ax), sg * (by - ay)))
    return cov, w


def _depth(w, z, area2):
    """-> (zpix float32, s float64, [w_k / z_k])"""
    with np.errstate(all="ignore"):
        q = [np.asarray(w[k]).astype(np.float64) / np.float64(z[k]) for k in range(3)]
        s = (q[0] + q[1]) + q[2]
        return (np.float64(area2) / s).astype(np.float32), s, q


def rasterize(vertices, faces, c2w, fx, fy, cx, cy, H, W, near, attr=None, background=0.0, cull=0):
    """-> dict(depth float32 [H*W], tri int32 [H*W], rgb float32 [H*W,3] or None, counts int64 [4]: clipped, degenerate, invalid,
    covered; n_cover, n_front int32 [H*W]: how many of the faces that passed ``cull`` cover each pixel, and how many of those
    face the camera (area2 < 0); z, X, Y, usable: the projection)"""
    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = vertices.shape[0]
    x, y, z = project(vertices, c2w, fx, fy, cx, cy)
    X, Y, usable = snap(x, y, z, near)
    zbuf = np.full((H, W), EMPTY, dtype=np.uint64)
    n_cover, n_front = np.zeros((H, W), dtype=np.int32), np.zeros((H, W), dtype=np.int32)
    clipped = degenerate = invalid = 0
    for f, idx in enumerate(faces):
        if ((idx < 0) | (idx >= V)).any():
            invalid += 1
            continue
        if not usable[idx].all():
            clipped += 1
            continue
        P = [(int(X[i]), int(Y[i])) for i in idx]
        area2 = edge(*P[0], *P[1], *P[2])
        if area2 == 0:
            degenerate += 1
            continue
        if (cull == 1 and area2 > 0) or (cull == 2 and area2 < 0):
            continue
        i0, i1 = max(-(-min(p[0] for p in P) // SUB), 0), min(max(p[0] for p in P) // SUB, W - 1)
        j0, j1 = max(-(-min(p[1] for p in P) // SUB), 0), min(max(p[1] for p in P) // SUB, H - 1)
        if i0 > i1 or j0 > j1:
            continue
        py, px = np.meshgrid(np.arange(j0, j1 + 1, dtype=np.int64) * SUB, np.arange(i0, i1 + 1, dtype=np.int64) * SUB,
                             indexing="ij")
        cov, w = face_coverage(P, area2, px, py)
        zpix, _, _ = _depth(w, z[idx], area2)
        frag = (zpix.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        sub = zbuf[j0:j1 + 1, i0:i1 + 1]
        sub[cov] = np.minimum(sub[cov], frag[cov])
        n_cover[j0:j1 + 1, i0:i1 + 1] += cov
        if area2 < 0:
            n_front[j0:j1 + 1, i0:i1 + 1] += cov
    zbuf = zbuf.reshape(-1)
    hit = zbuf != EMPTY
    depth = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0.0)).astype(np.float32)
    tri = np.where(hit, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    rgb = None
    if attr is not None:
        attr = np.asarray(attr, dtype=np.float32).reshape(-1, 3)
        rgb = np.full((H * W, 3), np.float32(background), dtype=np.float32)
        at = np.nonzero(hit)[0]
        if at.size:
            idx = faces[tri[at]]                                                         # [n,3]
            px, py = (at % W).astype(np.int64) * SUB, (at // W).astype(np.int64) * SUB
            w = [edge(X[idx[:, (k + 1) % 3]], Y[idx[:, (k + 1) % 3]], X[idx[:, (k + 2) % 3]], Y[idx[:, (k + 2) % 3]], px, py)
                 for k in range(3)]
            with np.errstate(all="ignore"):
                q = [w[k].astype(np.float64) / z[idx[:, k]].astype(np.float64) for k in range(3)]
                s = (q[0] + q[1]) + q[2]
                for c in range(3):
                    a = [attr[idx[:, k], c].astype(np.float64) for k in range(3)]
                    rgb[at, c] = (((q[0] * a[0] + q[1] * a[1]) + q[2] * a[2]) / s).astype(np.float32)
    counts = np.array([clipped, degenerate, invalid, int(hit.sum())], dtype=np.int64)
    return dict(depth=depth, tri=tri, rgb=rgb, counts=counts, n_cover=n_cover.reshape(-1), n_front=n_front.reshape(-1), z=z,
                X=X, Y=Y, usable=usable)


def cover_counts(vertices, faces, c2w, fx, fy, cx, cy, H, W, near, cull=0):
    """-> (faces covering each pixel [H,W], those of them that face the camera [H,W])"""
    got = rasterize(vertices, faces, c2w, fx, fy, cx, cy, H, W, near, cull=cull)
    return got["n_cover"].reshape(H, W), got["n_front"].reshape(H, W)


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """a c2w [3,4] float32 in the project's convention: the camera looks along its -z, x to the right, y up"""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    return np.concatenate([np.stack([right, np.cross(back, right), back], axis=1), eye[:, None]], axis=1).astype(np.float32)


IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32)


def screen_vertices(xy, z=2.0, fx=1.0, fy=1.0, cx=0.0, cy=0.0):
    """world points that the IDENTITY camera with (fx, fy, cx, cy) = (1, 1, 0, 0) projects onto the screen points ``xy`` at
    depth ``z`` EXACTLY when xy * z and the quotient are exact in float32 (small integers or dyadic fractions, z a power of
    two): p = ((x - cx) z / fx, -(y - cy) z / fy, -z)"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), xy.shape[:1])
    return np.stack([(xy[:, 0] - cx) * z / fx, -(xy[:, 1] - cy) * z / fy, -z], axis=1).astype(np.float32)
