"""Host side of the depth report of the device evaluation (no GPU): the options are off by default, device_depth needs
device_eval, depth.txt has its exact text, the MSE of a sum is numpy's, and the two symbols are bound."""

import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trainer(**over):
    from nerf_sampling_amd.trainers import DepthNetTrainer

    kw = dict(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="", half_res=True, white_bkgd=True)
    kw.update(over)
    return DepthNetTrainer(**kw)


def test_options_default_to_off():
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.experiments import render, run
    from nerf_sampling_amd.trainers import Trainer

    assert inspect.signature(Trainer.__init__).parameters["device_depth"].default is False
    assert _trainer().device_depth is False and _trainer(device_eval=True).device_depth is False
    assert _trainer(device_eval=True, device_depth=True).device_depth is True
    for fn in (nerf_utils.score_views, nerf_utils.evaluate_views):
        p = inspect.signature(fn).parameters
        assert p["depth"].default is False and p["field_depths"].default is None and p["return_depths"].default is False
    for cli in (render.main, run.main):
        opt = {p.name: p for p in cli.params}["device_depth"]
        assert opt.is_flag and opt.default is False and opt.opts == ["--device-depth"]


def test_device_depth_needs_device_eval():
    with pytest.raises(ValueError, match="device_eval"):
        _trainer(device_depth=True)
    # the reports render_path keeps stay refused under the device evaluation, with or without the new option
    with pytest.raises(ValueError, match="device_eval reports a PSNR only"):
        _trainer(device_eval=True, device_depth=True, compare_nerf=True)


def test_evaluate_views_refusals_that_need_no_device():
    from nerf_sampling_amd import nerf_utils

    with pytest.raises(ValueError, match="compare_nerf / use_nerf_max_pts go through render_path"):
        nerf_utils.evaluate_views(None, [0], [None], [4, 4, 1.0], None, dict(trainer=_trainer(compare_nerf=True)), depth=True)
    with pytest.raises(ValueError, match="use_full_nerf"):
        nerf_utils.evaluate_views(None, [0], [None], [4, 4, 1.0], None, dict(trainer=_trainer(use_full_nerf=True)), depth=True)
    for extra in (dict(return_depths=True), dict(field_depths=[None])):
        with pytest.raises(ValueError, match="depth=True"):
            nerf_utils.evaluate_views(None, [0], [None], [4, 4, 1.0], None, dict(trainer=_trainer()), **extra)


def test_depth_txt_text(tmp_path):
    from nerf_sampling_amd import nerf_utils

    sample = np.array([0.015625, 2.5, 1e-3])
    mean = np.array([0.0078125, 1.25, 0.1 + 0.2])
    avg_s, avg_m = float(np.mean(sample)), float(np.mean(mean))
    want = ("000.png, MSE: 0.015625, mean MSE: 0.0078125\n001.png, MSE: 2.5, mean MSE: 1.25\n"
            "002.png, MSE: 0.001, mean MSE: 0.30000000000000004\n"
            f"Avg of 3 images:\nMSE: {avg_s}\nmean MSE: {avg_m}\n")
    assert nerf_utils.format_depth_txt(sample, avg_s, mean, avg_m) == want
    assert float(want.splitlines()[4][len("MSE: "):]) == avg_s and float(want.splitlines()[5][len("mean MSE: "):]) == avg_m
    out = tmp_path / "testset_000002"
    nerf_utils._write_depth_txt(str(out), sample, avg_s, mean, avg_m)
    assert (out / "depth.txt").read_text() == want
    assert [p.name for p in out.iterdir()] == ["depth.txt"]
    nan = nerf_utils.format_depth_txt(np.array([np.nan]), float("nan"), np.array([1.0]), 1.0)
    assert nan == "000.png, MSE: nan, mean MSE: 1.0\nAvg of 1 images:\nMSE: nan\nmean MSE: 1.0\n"


def test_mse_from_sqerr_is_numpys():
    import torch

    from nerf_sampling_amd import ops

    rng = np.random.default_rng(0)
    d = (rng.random((3, 7 * 13)) - 0.5).astype(np.float32).astype(np.float64)
    sums, n = np.sum(d * d, axis=1), d.shape[1]
    got = ops.mse_from_sqerr(sums, n)
    assert got.dtype == np.float64 and got.shape == (3,)
    assert np.array_equal(got, sums / n)
    assert np.array_equal(ops.mse_from_sqerr(torch.from_numpy(sums), n), got)          # a device-less tensor is read as it is
    assert float(ops.mse_from_sqerr(sums[0], n)) == got[0]
    assert float(ops.mse_from_sqerr(float(sums[0]), n)) == got[0]
    with_nan = ops.mse_from_sqerr(np.array([np.nan, 4.0]), 8)
    assert np.isnan(with_nan[0]) and with_nan[1] == 0.5
    assert ops.mse_from_sqerr(np.array([0.0]), n)[0] == 0.0


def test_symbols_are_bound_and_the_share_is_the_headers():
    import ctypes as C

    from nerf_sampling_amd import _lib

    for name, n_args in (("ns_depth_sqerr_workspace_bytes", 2), ("ns_depth_sqerr", 8)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    assert _lib.SIGNATURES["ns_depth_sqerr"][1][1] is C.c_int64 and _lib.SIGNATURES["ns_depth_sqerr"][1][3] is C.c_int64
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()
    S = int(re.search(r"#define NS_DEPTH_SQERR_SHARE (\d+)", text).group(1))
    # one double per workgroup share, rounded up to 256 bytes: 32 shares fill the first 256
    assert lib.ns_depth_sqerr_workspace_bytes(1, 1) == 256
    assert lib.ns_depth_sqerr_workspace_bytes(32 * S, 1) == 256 and lib.ns_depth_sqerr_workspace_bytes(32 * S + 1, 1) == 512
    assert lib.ns_depth_sqerr_workspace_bytes(S, 64) == 512 and lib.ns_depth_sqerr_workspace_bytes(S, 65) == 768
    for R, N in ((0, 4), (4, 0), (-1, 1), (2 ** 31, 1), (2 ** 25, 64)):           # shapes ns_depth_sqerr refuses
        assert lib.ns_depth_sqerr_workspace_bytes(R, N) == 0
    assert lib.ns_depth_sqerr_workspace_bytes(2 ** 31 - 1, 1) > 0
    # refused before any HIP call, so also without a GPU
    assert lib.ns_depth_sqerr(None, 0, None, 4, 4, None, None, None) == -1
    assert b"ns_depth_sqerr" in lib.ns_last_error()
