"""Host side of the device frames (no GPU): every new option is off by default, what cannot work is refused before anything
touches the device, and ns_frame_to8b is bound and exported."""

import ctypes
import inspect
import os

import pytest


def _trainer(cls=None, **over):
    from nerf_sampling_amd.trainers import DepthNetTrainer

    kw = dict(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="", half_res=True, white_bkgd=True)
    kw.update(over)
    return (cls or DepthNetTrainer)(**kw)


def test_new_options_default_to_off():
    from nerf_sampling_amd import nerf_utils, ops
    from nerf_sampling_amd.trainers import BlenderTrainer, FieldFitter, Trainer

    assert inspect.signature(Trainer.__init__).parameters["device_frames"].default is False
    assert _trainer().device_frames is False and _trainer(BlenderTrainer).device_frames is False
    assert _trainer(device_eval=True, device_frames=True).device_frames is True
    assert inspect.signature(FieldFitter.fit).parameters["test_frames"].default is False
    assert inspect.signature(FieldFitter.evaluate_views).parameters["frames"].default is False
    for fn in (nerf_utils.score_views, nerf_utils.evaluate_views):
        p = inspect.signature(fn).parameters
        assert p["frames"].default is False and p["return_frames"].default is False and p["savedir"].default is None
    w = inspect.signature(nerf_utils.write_views).parameters
    assert list(w)[:5] == ["poses", "hwf", "K", "render_kwargs", "savedir"] and w["savedir"].default is inspect.Parameter.empty
    f = inspect.signature(nerf_utils.FrameWriter.__init__).parameters
    assert list(f)[1:8] == ["savedir", "H", "W", "channels", "n_buffers", "workers", "compress_level"]
    assert (f["channels"].default, f["n_buffers"].default, f["workers"].default, f["compress_level"].default) == (3, 4, 4, None)
    assert nerf_utils.FrameWriter.MAX_WORKERS == 8
    o = inspect.signature(ops.frame_to8b).parameters
    assert list(o) == ["rgb", "alpha", "out", "channels"]
    assert (o["alpha"].default, o["out"].default, o["channels"].default) == (None, None, 3)


def test_both_clis_have_the_flag():
    from nerf_sampling_amd.experiments import render, run

    for cli in (render.main, run.main):
        opt = {p.name: p for p in cli.params}["device_frames"]
        assert opt.is_flag and opt.default is False and "--device-frames" in opt.opts


def test_device_frames_needs_device_eval():
    from nerf_sampling_amd.trainers import BlenderTrainer

    for cls in (None, BlenderTrainer):
        with pytest.raises(ValueError, match="device_eval"):
            _trainer(cls, device_frames=True)


def test_frames_without_savedir_is_refused_before_the_device():
    """the dataset, the poses and the renderer are never looked at"""
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.trainers import FieldFitter

    with pytest.raises(ValueError, match="savedir"):
        nerf_utils.score_views(None, [0], [None], None, savedir=None, frames=True)
    with pytest.raises(ValueError, match="savedir"):
        nerf_utils.evaluate_views(None, [0], [None], [4, 4, 1.0], None, dict(trainer=_trainer()), frames=True)
    with pytest.raises(ValueError, match="savedir"):
        nerf_utils.write_views([None], [4, 4, 1.0], None, dict(trainer=_trainer()), None)
    with pytest.raises(ValueError, match="n_buffers"):
        nerf_utils.score_views(None, [0], [None], None, savedir="/tmp/x", frames={"threads": 2})
    fitter = FieldFitter.__new__(FieldFitter)
    with pytest.raises(ValueError, match="basedir"):
        fitter.fit(lambda: None, 1, i_testset=2, test_frames=True)


def test_frame_to8b_refuses_host_tensors():
    """as ops._dev does: no CPU fallback"""
    import torch

    from nerf_sampling_amd import nerf_utils, ops

    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_to8b(torch.zeros(4, 3))
    with pytest.raises(TypeError):
        ops.frame_to8b([[0.0, 0.0, 0.0]])
    with pytest.raises(RuntimeError, match="GPU"):
        nerf_utils.FrameWriter("/tmp/never_made_frames_dir", 4, 4, device="cpu")
    assert not os.path.exists("/tmp/never_made_frames_dir")


def test_the_binding_and_the_export():
    from nerf_sampling_amd import _lib

    restype, argtypes = _lib.SIGNATURES["ns_frame_to8b"]
    assert restype is ctypes.c_int and len(argtypes) == 7
    assert argtypes[1] is ctypes.c_int64 and argtypes[3] is ctypes.c_int64 and argtypes[5] is ctypes.c_int
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ns_frame_to8b")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include",
                               "nerf_sampling_hip.h")).read()
    assert "int ns_frame_to8b(const float* rgb_dev, int64_t rgb_stride, const float* alpha_dev, int64_t n_pixels" in header
    assert "run_nerf_helpers.py:11" in header and "nerf_utils.py:322-325" in header


def test_argument_checks_return_before_anything_touches_the_device():
    """every refusal, and the empty frame, return from the host code ahead of the launch, so they run without a GPU (the
    pointers are never dereferenced; tests/test_gpu_frame_to8b.py repeats the refusals on real buffers and checks the output)."""
    from nerf_sampling_amd import _lib

    fn = _lib.load().ns_frame_to8b
    rgb, out = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)
    assert fn(rgb, 0, None, 0, out, 3, None) == 0 and fn(None, 4, None, 0, None, 4, None) == 0          # n_pixels == 0
    bad = [(None, 0, None, 5, out, 3), (rgb, 0, None, 5, None, 3), (rgb, 0, None, -1, out, 3),
           (rgb, 0, None, 2 ** 29, out, 3), (rgb, 3, None, 2 ** 40, out, 4)]
    bad += [(rgb, s, None, 5, out, 3) for s in (-1, 1, 2, 5, 6)] + [(rgb, 0, None, 5, out, c) for c in (-3, 0, 1, 2, 5)]
    for args in bad:
        assert fn(*args, None) == -1, args
        assert b"ns_frame_to8b" in _lib.load().ns_last_error()
