"""The host side of the device point cloud (not gpu): the new switches and their defaults, the PLY writer, the reference's two
plot.py helpers, and the numpy reference tests/test_gpu_cloud.py measures ns_cloud_append against."""

import inspect
import random

import numpy as np
import pytest
import torch

import cloud_reference as CR


def test_new_parameters_default_off_and_the_pinned_ones_stay():
    from nerf_sampling_amd import nerf_utils, ops
    from nerf_sampling_amd.trainers import Trainer

    p = inspect.signature(Trainer.__init__).parameters
    assert p["device_cloud"].default is False and p["cloud_min_weight"].default == 0.0 and p["cloud_points"].default is None
    assert isinstance(p["cloud_min_weight"].default, float)
    for name in ("device_eval", "device_ssim", "device_depth", "device_batches", "save_scene_data"):
        assert p[name].default is False, name
    assert p["hip_graph"].default is True and p["batch_seed"].default == 0
    s = inspect.signature(nerf_utils.scene_cloud).parameters
    assert list(s) == ["render_poses", "hwf", "K", "render_kwargs", "min_weight", "max_points", "capacity", "colours", "savedir",
                       "seed"]
    assert (s["min_weight"].default, s["max_points"].default, s["capacity"].default, s["colours"].default, s["savedir"].default,
            s["seed"].default) == (0.0, None, None, True, None, 0)
    a = inspect.signature(ops.cloud_append).parameters
    assert list(a) == ["cloud", "o", "d", "z", "w", "rgb", "min_weight"] and a["rgb"].default is None and a["min_weight"].default == 0.0
    c = inspect.signature(ops.PointCloud.__init__).parameters
    assert c["colours"].default is False and c["device"].default == "cuda"
    with pytest.raises(ValueError):
        Trainer(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="", device_cloud=True,
                cloud_points=-1)


def test_render_cli_has_the_three_flags():
    from nerf_sampling_amd.experiments.render import main

    opts = {o.name: o for o in main.params}
    assert opts["device_cloud"].is_flag and opts["device_cloud"].default is False
    assert opts["cloud_min_weight"].default == 0.0 and opts["cloud_points"].default is None
    assert "--device-cloud" in opts["device_cloud"].opts and "raise it" in opts["cloud_min_weight"].help


def test_ply_writer(tmp_path):
    from nerf_sampling_amd.nerf_utils import write_ply

    pts = np.array([[0.0, 1.0, -2.0], [3.5, np.nan, 1e-3], [7.0, 8.0, 9.0]], dtype=np.float32)
    rgb = np.array([[0.0, 0.5, 1.0], [-0.25, 1.5, 0.999], [0.1, 0.2, 0.8]], dtype=np.float32)    # below 0 and above 1: clipped
    w = np.array([0.25, 0.5, 1.0], dtype=np.float32)
    path = str(tmp_path / "c.ply")
    write_ply(path, pts, rgb, w)
    raw = open(path, "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty float weight\nend_header\n").encode("ascii")
    assert raw.startswith(header) and len(raw) == len(header) + 3 * 19
    body = raw[len(header):]
    for i in range(3):
        rec = body[19 * i:19 * (i + 1)]
        assert rec[:12] == pts[i].astype("<f4").tobytes() and rec[15:] == w[i:i + 1].astype("<f4").tobytes()
    assert list(body[12:15]) == [0, 127, 255] and list(body[19 + 12:19 + 15]) == [0, 255, 254] and list(body[38 + 12:38 + 15]) == [25, 51, 204]
    write_ply(path, pts, None, w)                                                   # no colours: white
    assert list(open(path, "rb").read()[len(header) + 12:len(header) + 15]) == [255, 255, 255]
    write_ply(path, pts[:0], rgb[:0], w[:0])
    assert open(path, "rb").read() == header.replace(b"vertex 3", b"vertex 0")
    with pytest.raises(ValueError):
        write_ply(path, pts, rgb, w[:2])


def test_compat_helpers_behave_as_the_reference_ones():
    from nerf_sampling_amd import utils

    d = torch.tensor([[0.5, float("nan"), -0.0], [0.0, 1e-9, float("inf")]])
    mask = utils.get_min_indices(d, 0.0)
    assert mask.dtype == torch.bool and mask.tolist() == [[True, False, True], [True, True, True]]
    assert utils.get_min_indices(d, torch.tensor(0.5)).tolist() == [[True, False, False], [False, False, True]]
    random.seed(5)
    got = utils.get_random_indices(100, 7)
    random.seed(5)
    assert got == random.sample(range(100), k=7) and len(set(got)) == 7 and all(0 <= i < 100 for i in got)
    assert utils.get_random_indices(4, 4) != [] and sorted(utils.get_random_indices(4, 4)) == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        utils.get_random_indices(3, 4)
    # through the compat alias, where a plot.py-style script looks for them
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat"))
    try:
        from nerf_sampling.nerf_pytorch import utils as aliased
    finally:
        sys.path.pop(0)
    assert aliased.get_min_indices is utils.get_min_indices and aliased.get_random_indices is utils.get_random_indices


def test_numpy_reference_on_a_hand_written_case():
    """two rays of four samples: element e = 4 r + k, kept where w >= 0.5"""
    w = np.array([[0.5, 0.49999997, np.nan, 0.75], [np.inf, -np.inf, 0.5, 0.0]], dtype=np.float32)
    pts = np.arange(24, dtype=np.float32).reshape(2, 4, 3)
    rgb = np.array([[0.1, 0.2, 0.3], [0.7, 0.8, 0.9]], dtype=np.float32)
    assert CR.keep_mask(w, 0.5).tolist() == [[True, False, False, True], [True, False, True, False]]
    p, ww, c = CR.select(pts, w, rgb, 0.5)
    assert p.tolist() == [[0, 1, 2], [9, 10, 11], [12, 13, 14], [18, 19, 20]]
    assert ww.tolist() == [0.5, 0.75, np.inf, 0.5]
    assert c.tolist() == rgb[[0, 0, 1, 1]].tolist()
    # -0.0 passes a threshold of 0.0, NaN passes none, and a NaN threshold keeps nothing
    z = np.array([[-0.0, 0.0, np.nan, -1e-30]], dtype=np.float32)
    assert CR.keep_mask(z, 0.0).tolist() == [[True, True, False, False]]
    assert not CR.keep_mask(z, np.nan).any()
    assert CR.select(pts[:1], z, None, 0.0)[2] is None
    # batches are concatenated in order, each with its own N
    both = CR.select_batches([(pts, w, rgb), (pts[:1, :1], np.array([[1.0]], np.float32), rgb[1:])], 0.5)
    assert both[0].shape == (5, 3) and both[0][-1].tolist() == [0, 1, 2] and both[1][-1] == 1.0 and both[2][-1].tolist() == rgb[1].tolist()
    none = CR.select_batches([(pts, w, rgb)], 2.0 ** 100)
    assert none[0].shape == (1, 3) and none[1].tolist() == [np.inf]
