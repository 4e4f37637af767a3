"""The numpy statement of ns_cloud_append, shared by tests/test_gpu_cloud.py (the kernel) and tests/test_device_cloud_host.py (a
hand-written case).  Nothing here calls the library."""

import numpy as np


def keep_mask(w, t):
    """w >= t per sample; a NaN weight (or a NaN threshold) compares false, -0.0 >= 0.0 true"""
    with np.errstate(invalid="ignore"):
        return np.asarray(w, dtype=np.float32) >= np.float32(t)


def select(pts, w, rgb, t):
    """The records one batch contributes: pts [R,N,3], w [R,N], rgb [R,3] or None -> (pts[mask] [M,3], w[mask] [M], the kept
    samples' RAY colours [M,3] or None), ray-major and sample-minor."""
    pts, w = np.asarray(pts), np.asarray(w, dtype=np.float32)
    R, N = w.shape
    mask = keep_mask(w, t)
    ray_of = np.nonzero(mask)[0]                       # row-major order: rays, then samples
    return pts.reshape(R, N, 3)[mask], w[mask], (None if rgb is None else np.asarray(rgb)[ray_of])


def select_batches(batches, t):
    """the concatenation of ``select`` over the batches (pts, w, rgb), in order: what appending them one by one must give"""
    parts = [select(p, w, c, t) for p, w, c in batches]
    colours = None if parts[0][2] is None else np.concatenate([p[2] for p in parts]).reshape(-1, 3)
    return np.concatenate([p[0] for p in parts]).reshape(-1, 3), np.concatenate([p[1] for p in parts]), colours
