"""The tall GEMM's host side: declaration, binding, argument checks of the C entry and of the Python wrappers (not gpu)."""

import ctypes as C
import os
import re

import pytest
import torch

from nerf_sampling_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_and_the_binding_matches():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read(), flags=re.S)
    m = re.search(r"\bns_gemm_tall\s*\(([^)]*)\)\s*;", text)
    assert m, "ns_gemm_tall is not declared in the header"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert n_args == 17
    assert len(_lib.SIGNATURES["ns_gemm_tall"][1]) == n_args
    assert hasattr(_lib.load(), "ns_gemm_tall")


def _call(**over):
    """ns_gemm_tall on made-up (never dereferenced) addresses: every case below fails a check, and no launch follows one"""
    a = dict(A=C.c_void_p(0x10000), lda=256, B=C.c_void_p(0x20000), sb0=256, sb1=1, bias=None, Cp=C.c_void_p(0x30000), ldc=256,
             rows=1000, N=256, K=256, acc=0, act=0, dact=0, ref=None, ld_ref=0)
    a.update(over)
    return _lib.load().ns_gemm_tall(a["A"], a["lda"], a["B"], a["sb0"], a["sb1"], a["bias"], a["Cp"], a["ldc"], a["rows"], a["N"],
                                    a["K"], a["acc"], a["act"], a["dact"], a["ref"], a["ld_ref"], None)


@pytest.mark.parametrize("over", [dict(N=513), dict(K=513), dict(N=513, K=513, lda=600, ldc=600)])
def test_larger_shapes_are_unsupported(over):
    assert _call(**over) == -2
    assert b"ns_gemm_tall" in _lib.load().ns_last_error()


@pytest.mark.parametrize("over", [
    dict(rows=0), dict(rows=-1), dict(rows=1 << 31), dict(N=0), dict(K=0), dict(A=None), dict(B=None), dict(Cp=None),
    dict(A=C.c_void_p(0x10002)), dict(B=C.c_void_p(0x20001)), dict(Cp=C.c_void_p(0x30003)), dict(bias=C.c_void_p(0x40002)),
    dict(lda=255), dict(ldc=255), dict(sb0=-1), dict(acc=2), dict(act=4), dict(dact=4), dict(dact=1),
    dict(dact=1, ref=C.c_void_p(0x50000), ld_ref=255), dict(dact=1, ref=C.c_void_p(0x50002), ld_ref=256),
])
def test_bad_arguments_are_invalid(over):
    assert _call(**over) == -1
    assert b"ns_gemm_tall" in _lib.load().ns_last_error()


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from nerf_sampling_amd import autograd as ag

    x, W, b = torch.zeros(5, 8), torch.zeros(4, 8), torch.zeros(4)
    with pytest.raises(RuntimeError, match="GPU"):
        ag.linear_forward_tall(x, W, b, ag.RELU)
    with pytest.raises(RuntimeError, match="GPU"):
        ag.linear_backward_input_tall(torch.zeros(5, 4), W)
    with pytest.raises(TypeError):
        ag.linear_forward_tall(None, W, b)


@pytest.mark.parametrize("bad", ["bogus", "", "Tall", None])
def test_unknown_engine_raises(bad):
    from nerf_sampling_amd import autograd as ag
    from nerf_sampling_amd.run_nerf_helpers import NeRF
    from nerf_sampling_amd.trainers import FieldFitter

    net = NeRF(D=2, W=32, input_ch=63, input_ch_views=27, output_ch=5, skips=[], use_viewdirs=True)
    with pytest.raises(ValueError, match="engine"):
        FieldFitter(net, None, gemm_engine=bad)
    with pytest.raises(ValueError, match="engine"):
        ag.nerf_forward_train(net, torch.zeros(2, 2, 3), torch.zeros(2, 3), engine=bad)


def test_default_engine_is_tile():
    import inspect

    from nerf_sampling_amd import autograd as ag
    from nerf_sampling_amd.trainers import FieldFitter

    assert inspect.signature(FieldFitter.__init__).parameters["gemm_engine"].default == "tile"
    assert inspect.signature(ag.nerf_forward_train).parameters["engine"].default == "tile"
    assert inspect.signature(ag._nerf_layers_forward).parameters["engine"].default == "tile"
    assert inspect.signature(ag._nerf_layers_backward).parameters["engine"].default == "tile"
