"""Host side of the device evaluation (no GPU): the options are off by default, what cannot be evaluated is refused at
construction, psnr.txt has render_path's text, and the PSNR of a sum is numpy's."""

import inspect

import numpy as np
import pytest


def _trainer(cls=None, **over):
    from nerf_sampling_amd.trainers import DepthNetTrainer

    kw = dict(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="", half_res=True, white_bkgd=True)
    kw.update(over)
    return (cls or DepthNetTrainer)(**kw)


def test_options_default_to_off():
    from nerf_sampling_amd.experiments import render, run
    from nerf_sampling_amd.trainers import BlenderTrainer, FieldFitter, Trainer

    assert inspect.signature(Trainer.__init__).parameters["device_eval"].default is False
    assert _trainer().device_eval is False and _trainer(BlenderTrainer).device_eval is False
    assert _trainer(device_eval=True).device_eval is True and _trainer(BlenderTrainer, device_eval=True).device_eval is True
    assert _trainer().i_testset == 100                                    # the reference's default, unused while the option is off
    fit = inspect.signature(FieldFitter.fit).parameters
    assert fit["i_testset"].default == 0 and fit["test_ids"].default is None
    for cli, flag in ((render.main, "device_psnr"), (run.main, "device_eval")):
        opt = {p.name: p for p in cli.params}[flag]
        assert opt.is_flag and opt.default is False


@pytest.mark.parametrize("bad", [dict(compare_nerf=True), dict(use_nerf_max_pts=True)])
def test_reports_beyond_a_psnr_are_refused_at_construction(bad):
    with pytest.raises(ValueError, match="device_eval"):
        _trainer(device_eval=True, **bad)
    assert _trainer(**bad).device_eval is False                            # and stay available without the option
    assert _trainer(device_eval=True, use_full_nerf=True).use_full_nerf


def test_evaluate_views_refuses_those_reports_too():
    from nerf_sampling_amd import nerf_utils

    tr = _trainer(compare_nerf=True)
    with pytest.raises(ValueError, match="compare_nerf"):
        nerf_utils.evaluate_views(None, [0], [None], [4, 4, 1.0], None, dict(trainer=tr))


def test_psnr_txt_text(tmp_path):
    """render_path's format (nerf_utils.py:318-336): one line per view, then the average over n images"""
    from nerf_sampling_amd import nerf_utils

    psnrs = np.array([23.5, 7.0625, 31.25])
    avg = float(np.mean(psnrs))
    want = ("000.png, PSNR: 23.5\n001.png, PSNR: 7.0625\n002.png, PSNR: 31.25\n"
            f"Avg of 3 images:\nPSNR: {avg}\n")
    assert nerf_utils.format_psnr_txt(psnrs, avg) == want
    out = tmp_path / "testset_000003"
    nerf_utils._write_psnr_txt(str(out), psnrs, avg)
    assert (out / "psnr.txt").read_text() == want
    assert [p.name for p in out.iterdir()] == ["psnr.txt"]                # no PNG
    # the view lines are render_path's own expression
    i, psnr = 1, psnrs[1]
    assert want.splitlines()[1] == f"{i:03d}.png, PSNR: {psnr}"


def test_psnr_from_sqerr_is_numpys():
    import torch

    from nerf_sampling_amd.ray_batches import DeviceRayDataset

    rng = np.random.default_rng(0)
    d = (rng.random((3, 11 * 13 * 3)) - 0.5).astype(np.float32).astype(np.float64)
    sums = np.sum(d * d, axis=1)
    n = d.shape[1]
    want = -10.0 * np.log10(np.mean(d * d, axis=1))
    got = DeviceRayDataset.psnr_from_sqerr(sums, n)
    assert got.dtype == np.float64 and got.shape == (3,)
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
    assert np.array_equal(got, -10.0 * np.log10(sums / n))
    assert np.array_equal(DeviceRayDataset.psnr_from_sqerr(torch.from_numpy(sums), n), got)      # a tensor is read back
    assert float(DeviceRayDataset.psnr_from_sqerr(sums[0], n)) == got[0]
    assert np.isnan(DeviceRayDataset.psnr_from_sqerr(np.array([np.nan]), n)[0])
    assert DeviceRayDataset.psnr_from_sqerr(np.array([0.0]), n)[0] == np.inf


def test_a_callable_ray_source_has_no_held_out_views():
    """checked before anything touches the device"""
    from nerf_sampling_amd.trainers import FieldFitter

    fitter = FieldFitter.__new__(FieldFitter)
    with pytest.raises(ValueError, match="i_testset"):
        fitter.fit(lambda: None, 1, i_testset=2)
