"""ns_map_max / ops.map_max against np.nanmax on the host copy of the same fp32 map: state[0] is the maximum over the values that
are not NaN (-inf when there are none; compared with ==, the sign of a zero is not specified), state[1] the NaN flag.  The counts
and layouts of tests/test_gpu_map_to8b.py; accumulated calls against the concatenation; the maximum in the first, the last and
a middle position and in the last, partial group of a second workgroup; and nothing but the two floats and the workspace is
written."""

import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import test_gpu_map_to8b as T

pytestmark = pytest.mark.gpu

COUNTS = T.COUNTS
SHARE = 2048                                 # values per workgroup (the header's statement of the partition)
POISON = 0xA5


def _nanmax(x):
    """(np.nanmax with -inf for nothing to take a maximum of, whether a NaN is there)"""
    nan = np.isnan(x)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return (np.float32(np.nanmax(x)) if not nan.all() else np.float32(-np.inf)), bool(nan.any())


def _maps():
    """fp32 [max count] in [-0.3, 0.7], a NaN every 97 values from the 11th on (the five smallest counts see none)"""
    x = np.random.default_rng(43).random(max(COUNTS), dtype=np.float32) - np.float32(0.3)
    x[10::97] = np.nan
    return x


def _check(state, x, where=None):
    got = state.cpu().numpy()
    want_max, want_nan = _nanmax(x)
    assert got.dtype == np.float32 and got.shape == (2,)
    assert got[0] == want_max and got[1] == (1.0 if want_nan else 0.0), (where, got.tolist(), float(want_max), want_nan)


@pytest.mark.parametrize("layout", ["packed", "column"])
def test_every_count_and_layout_is_nanmax_and_the_flag(layout):
    from nerf_sampling_amd import ops

    x = _maps()
    flags = set()
    for n in COUNTS:
        for in_off in range(4):
            m = T._device_map(x[:n], layout, in_off)
            state = ops.map_max(m)
            _check(state, x[:n], (layout, n, in_off))
            flags.add(float(state.cpu()[1]))
    assert flags == {0.0, 1.0}


def test_all_nan_no_nan_infinities_and_zeros():
    from nerf_sampling_amd import ops

    for layout in ("packed", "column"):
        for n in (1, 5, 257, 4099):
            nan = np.full(n, np.nan, np.float32)
            got = ops.map_max(T._device_map(nan, layout, 1)).cpu().numpy()
            assert got[0] == -np.inf and got[1] == 1.0, (layout, n, got.tolist())
            neg = -np.random.default_rng(n).random(n, dtype=np.float32) - np.float32(1)      # all below the initial 0 of a lazy fold
            _check(ops.map_max(T._device_map(neg, layout, 0)), neg)
        special = np.array([-np.inf, np.nan, -0.0, 0.0, -1e-40, -3.0], np.float32)
        _check(ops.map_max(T._device_map(special, layout, 0)), special)
        assert ops.map_max(T._device_map(special, layout, 0)).cpu()[0] == 0.0
        _check(ops.map_max(T._device_map(np.array([1.0, np.inf, 2.0], np.float32), layout, 0)),
               np.array([np.inf], np.float32))
        _check(ops.map_max(T._device_map(np.array([-np.inf, -np.inf], np.float32), layout, 0)), np.array([-np.inf], np.float32))


@pytest.mark.parametrize("layout", ["packed", "column"])
def test_three_accumulated_calls_are_the_concatenation(layout):
    from nerf_sampling_amd import ops

    rng = np.random.default_rng(47)
    for trial, (where_max, where_nan) in enumerate([(0, None), (1, 2), (2, 0), (1, None), (0, 1)]):
        parts = [rng.random(n, dtype=np.float32) for n in (1025, 4099, 63)]
        parts[where_max][rng.integers(0, parts[where_max].size)] = 1.5
        if where_nan is not None:
            parts[where_nan][3 % parts[where_nan].size] = np.nan
        state = torch.full((2,), 123.0, device="cuda")
        ws = torch.empty((ops.map_max_workspace_bytes(4099),), dtype=torch.uint8, device="cuda")
        for k, p in enumerate(parts):
            assert ops.map_max(T._device_map(p, layout, k), state=state, accumulate=k > 0, workspace=ws) is state
            _check(state, np.concatenate(parts[:k + 1]), (trial, k))
        assert float(state.cpu()[0]) == 1.5
        # a fresh call on the same state forgets what was there, the flag included
        ops.map_max(T._device_map(parts[2], layout, 0), state=state, accumulate=False, workspace=ws)
        _check(state, parts[2], trial)


@pytest.mark.parametrize("layout", ["packed", "column"])
def test_the_maximum_is_found_wherever_it_lies(layout):
    """first, last and middle positions; the last, partial group of four of a second workgroup (a packed map on a 16-byte
    boundary is read as float4s, its tail one float at a time) and the last value of a first, full one"""
    from nerf_sampling_amd import ops

    base = np.random.default_rng(53).random(3 * SHARE, dtype=np.float32) * np.float32(0.5)
    cases = [(n, pos) for n in (SHARE + 5, SHARE + 6, SHARE + 7, 2 * SHARE, 2 * SHARE + 1, 4099)
             for pos in (0, n // 2, SHARE - 1, SHARE, n - 3, n - 2, n - 1)]
    cases += [(n, pos) for n in (1, 2, 3, 5, 255, 257) for pos in (0, n // 2, n - 1)]
    for n, pos in cases:
        x = base[:n].copy()
        x[pos] = 0.75
        for in_off in (0, 1):
            got = ops.map_max(T._device_map(x, layout, in_off)).cpu().numpy()
            assert got[0] == np.float32(0.75) and got[1] == 0.0, (layout, n, pos, in_off, got.tolist())


@pytest.mark.parametrize("layout", ["packed", "column"])
def test_only_the_state_and_the_workspace_are_written(layout):
    from nerf_sampling_amd import ops

    x = _maps()[:4099]
    m = T._device_map(x, layout, 0)
    before = m.cpu().numpy().tobytes()
    need = ops.map_max_workspace_bytes(x.size)
    assert need == 256 and ops.map_max_workspace_bytes(32 * SHARE + 1) == 512 and ops.map_max_workspace_bytes(0) == 0
    ws_buf = torch.full((8 + need + 64,), POISON, dtype=torch.uint8, device="cuda")
    fenced = torch.full((6,), 77.0, dtype=torch.float32, device="cuda")
    for lo in (1, 2):                                                  # a state that is 4-byte and one that is 8-byte aligned
        fenced.fill_(77.0)
        ws_buf.fill_(POISON)
        state = fenced[lo:lo + 2]
        ops.map_max(m, state=state, workspace=ws_buf[8:8 + need])
        _check(state, x)
        host = fenced.cpu().numpy()
        assert (host[:lo] == 77.0).all() and (host[lo + 2:] == 77.0).all()
        ws = ws_buf.cpu().numpy()
        assert (ws[:8] == POISON).all() and (ws[8 + need:] == POISON).all()
        assert (ws[8 + 8 * 3:8 + need] == POISON).all()                # three workgroups leave three (max, flag) pairs
    assert m.cpu().numpy().tobytes() == before


def test_an_empty_map_and_the_refusals():
    from nerf_sampling_amd import _lib, ops

    x = torch.rand(16, device="cuda")
    state = torch.tensor([3.0, 1.0], device="cuda")
    assert ops.map_max(x[:0], state=state, accumulate=True).cpu().tolist() == [3.0, 1.0]      # left as it is
    got = ops.map_max(x[:0], state=state).cpu().numpy()
    assert got[0] == -np.inf and got[1] == 0.0                                               # initialised from nothing
    got = ops.map_max(x[:0]).cpu().numpy()
    assert got[0] == -np.inf and got[1] == 0.0
    lib = _lib.load()
    state.copy_(torch.tensor([3.0, 1.0]))
    ws = torch.empty((256,), dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp, sp, wp = C.c_void_p(x.data_ptr()), C.c_void_p(state.data_ptr()), C.c_void_p(ws.data_ptr())
    bad = [(None, 1, 16, 0, sp, wp), (xp, 1, 16, 0, None, wp), (xp, 1, 16, 0, sp, None), (xp, 1, -1, 0, sp, wp),
           (xp, 1, 2 ** 31, 0, sp, wp), (xp, 1, 16, 0, C.c_void_p(state.data_ptr() + 2), wp),
           (xp, 1, 16, 0, sp, C.c_void_p(ws.data_ptr() + 4))]
    bad += [(xp, st, 16, 0, sp, wp) for st in (-1, 0, 2, 3, 5)]
    for args in bad:
        assert lib.ns_map_max(*args, s) == -1, args
        assert b"ns_map_max" in lib.ns_last_error()
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [3.0, 1.0]
    for kwargs in (dict(accumulate=True), dict(state=torch.zeros(3, device="cuda")), dict(state=torch.zeros(2)),
                   dict(state=torch.zeros(2, device="cuda", dtype=torch.float64)), dict(workspace=ws[:255]),
                   dict(workspace=ws[1:]), dict(workspace=torch.empty(256, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            ops.map_max(x, **kwargs)
    for bad_map in (torch.rand(16, 2, device="cuda"), torch.rand(48, device="cuda")[::3], x.double()):
        with pytest.raises(ValueError):
            ops.map_max(bad_map)
    with pytest.raises(RuntimeError):
        ops.map_max(x.cpu())
