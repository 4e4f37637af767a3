"""The host restatement of the ray-batch generator (ray_batches.permute_index / draw_indices) and the C ABI of the two
ray-batch entries: argument refusals happen before any HIP call, so they are checked here without a GPU."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from nerf_sampling_amd import _lib
from nerf_sampling_amd import ray_batches as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 15, 16, 17, 660, 4097])
def test_permute_index_is_a_bijection(n):
    perms = set()
    for seed in (0, 1, 0xDEADBEEFCAFE, (1 << 64) - 1):
        for counter in (0, 1, 2, 1 << 40):
            p = RB.permute_index(n, seed, counter, np.arange(n))
            assert np.array_equal(np.sort(p), np.arange(n)), (n, seed, counter)
            perms.add(tuple(p))
    if n >= 15:                                   # 16 (seed, counter) pairs: no two share a permutation
        assert len(perms) == 16


def test_permute_index_at_a_full_frame():
    n = 640000                                    # 800 x 800
    a = RB.permute_index(n, 7, 0, np.arange(n))
    b = RB.permute_index(n, 7, 1, np.arange(n))
    assert np.array_equal(np.sort(a), np.arange(n)) and np.array_equal(np.sort(b), np.arange(n))
    assert (a != b).mean() > 0.99 and (a != np.arange(n)).mean() > 0.99
    # single indices and any array shape agree with the vectorised call
    assert int(RB.permute_index(n, 7, 0, 12345)) == a[12345]
    assert np.array_equal(RB.permute_index(n, 7, 1, np.arange(12).reshape(3, 4)), b[:12].reshape(3, 4))


def test_permute_index_refuses_bad_arguments():
    for n, i in ((0, []), (1 << 31, [0]), (5, [5]), (5, [-1])):
        with pytest.raises(ValueError):
            RB.permute_index(n, 0, 0, i)


def test_all_images_scope_covers_each_epoch_once():
    H, W, train = 5, 7, [2, 0, 1]                 # N = 105 rays, B = 64: steps 0..4 hold three epochs and five rays
    N, B = 105, 64
    img, pix = zip(*(RB.draw_indices(B, s, 9, "all_images", H, W, train) for s in range(5)))
    g = np.concatenate(img).astype(np.int64) * (H * W) + np.concatenate(pix)
    assert g.size == 320
    for e in range(3):
        assert np.array_equal(np.sort(g[e * N:(e + 1) * N]), np.arange(N)), e
    assert len(set(g[3 * N:])) == 5
    assert not np.array_equal(g[:N], g[N:2 * N])


def test_per_image_scope_draws_a_window_without_repeats():
    H, W, train = 33, 20, [4, 1, 3]
    win = (10, 13, 6, 11)
    images = set()
    for step in range(12):
        img, pix = RB.draw_indices(15, step, 3, "per_image", H, W, train, window=win)
        assert img.dtype == pix.dtype == np.int32 and len(set(img)) == 1 and int(img[0]) in train
        images.add(int(img[0]))
        rows, cols = pix // W, pix % W
        assert rows.min() >= 10 and rows.max() < 13 and cols.min() >= 6 and cols.max() < 11
        assert len(set(pix)) == 15                # the whole 3 x 5 window: a permutation of it
    assert images == set(train)
    whole, _ = RB.draw_indices(660, 0, 3, "per_image", H, W, train)[1], None
    assert np.array_equal(np.sort(whole), np.arange(660))
    for bad in ((0, 0, 0, 5), (0, 34, 0, 5), (3, 2, 0, 5), (0, 3, -1, 5)):
        with pytest.raises(ValueError):
            RB.draw_indices(1, 0, 3, "per_image", H, W, train, window=bad)
    with pytest.raises(ValueError):
        RB.draw_indices(16, 0, 3, "per_image", H, W, train, window=win)
    with pytest.raises(ValueError):
        RB.draw_indices(1, 0, 3, "some_images", H, W, train)


def test_precrop_window_is_the_reference_crop():
    assert RB.precrop_window(800, 800, 0.5) == (200, 600, 200, 600)
    assert RB.precrop_window(33, 20, 0.5) == (8, 24, 5, 15)


def test_header_exports_match_the_bindings():
    text = open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(ns_[a-z0-9_]+)\s*\(", text))
    assert {"ns_ray_batch_gather", "ns_ray_batch_draw"} <= names
    assert names == set(_lib.SIGNATURES)
    lib = _lib.load()
    assert hasattr(lib, "ns_ray_batch_gather") and hasattr(lib, "ns_ray_batch_draw")
    for macro, value in (("NS_RAY_SCOPE_PER_IMAGE", _lib.RAY_SCOPE_PER_IMAGE), ("NS_RAY_SCOPE_ALL_IMAGES", _lib.RAY_SCOPE_ALL_IMAGES),
                         ("NS_RAY_DRAW_ROUNDS", RB.ROUNDS)):
        assert int(re.search(r"#define " + macro + r" (\d+)", text).group(1)) == value
    assert RB.SCOPES.index("per_image") == _lib.RAY_SCOPE_PER_IMAGE and RB.SCOPES.index("all_images") == _lib.RAY_SCOPE_ALL_IMAGES


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_ray_struct_mirrors_match_the_header_layout(tmp_path):
    pairs = {"ns_ray_dataset": _lib.RayDataset, "ns_ray_draw_params": _lib.RayDrawParams}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nerf_sampling_hip.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read(), flags=re.S)
    for cname, cls in pairs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", text, flags=re.S).group(1)
        assert sum(len(decl.split(",")) for decl in body.split(";") if decl.strip()) == len(cls._fields_), cname


def _dataset(**over):
    d = dict(images_dev=1, poses_dev=1, n_images=3, H=5, W=7, C=3, pose_stride=12, white_bkgd=0, fx=1.0, fy=1.0, cx=0.0, cy=0.0)
    d.update(over)
    return _lib.RayDataset(**d)


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every refusal returns NS_E_INVALID from the argument checks, which run before the first HIP call: no GPU needed (the
    pointers below are never dereferenced)."""
    lib = _lib.load()
    one = ctypes.c_void_p(1)

    def gather(ds, B=4, img=0):
        return lib.ns_ray_batch_gather(ctypes.byref(ds), None, img, one, B, one, one, one, one, None)

    def draw(ds, B=4, scope=0, n_train=2, host=(0, 0, 5, 0, 7), dev=None):
        hp = None if host is None else ctypes.byref(_lib.RayDrawParams(*host))
        return lib.ns_ray_batch_draw(ctypes.byref(ds), one, n_train, scope, dev, hp, 0, B, None, None, one, one, one, one, None)

    for call in (gather, draw):
        assert call(_dataset(), B=-1) == -1 and b"batch size" in lib.ns_last_error()
        assert call(_dataset(n_images=1 << 11, H=1 << 10, W=1 << 10)) == -1 and b"2^31" in lib.ns_last_error()
        for ch in (1, 2, 5):
            assert call(_dataset(C=ch)) == -1 and b"channels" in lib.ns_last_error()
        assert call(_dataset(pose_stride=9)) == -1
        assert call(_dataset(poses_dev=None)) == -1
        assert call(_dataset(images_dev=None)) == -1
        assert call(_dataset(), B=0) == 0                                        # nothing to do, nothing launched
    assert gather(_dataset(), img=3) == -1 and b"image index" in lib.ns_last_error()
    assert gather(_dataset(), img=-1) == -1
    assert draw(_dataset(), host=(0, 2, 2, 0, 7)) == -1 and b"empty window" in lib.ns_last_error()
    assert draw(_dataset(), host=(0, 0, 5, 4, 3)) == -1 and b"empty window" in lib.ns_last_error()
    assert draw(_dataset(), host=(0, 0, 6, 0, 7)) == -1 and b"outside" in lib.ns_last_error()
    assert draw(_dataset(), B=36) == -1 and b"exceeds the window" in lib.ns_last_error()
    assert draw(_dataset(), host=(-1, 0, 5, 0, 7)) == -1
    assert draw(_dataset(), scope=2) == -1
    assert draw(_dataset(), n_train=0) == -1
    assert draw(_dataset(), host=None) == -1                                     # neither device nor host params
    assert draw(_dataset(), dev=one) == -1                                       # both
    assert draw(_dataset(n_images=1 << 10, H=1 << 10, W=1 << 10), n_train=1 << 11) == -1
