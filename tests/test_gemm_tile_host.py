"""The tile GEMM's host side (not gpu): the kernel's K slicing restated and proved on the index arithmetic, the reference of
tests/gemm_tile_reference.py against an independent product, the exactness bound of the integer cases, the argument checks of
ns_gemm_fused / ns_gemm_fused_batched, and the binding (argument counts, struct layout)."""

import ctypes as C
import functools
import os
import re

import pytest
import torch

import gemm_tile_reference as G
from nerf_sampling_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerf_sampling_hip.h")
SOURCE = os.path.join(ROOT, "nerf_sampling_amd", "csrc", "ns_train.hip")


@functools.lru_cache(maxsize=None)
def _visits(K, KT):
    return G.slice_visits(K, KT)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- the K slicing -----------------------------------------------------------------------------------------------------

def test_every_k_is_visited_exactly_once():
    for KT in (32, 64):
        for K in range(0, 1101):
            seen = [k for wave in _visits(K, KT) for pair in wave for k in pair if k is not None]
            assert sorted(seen) == list(range(K)), (K, KT)


def _order(K, KT):
    """Per wave, the MFMAs that feed anything, in issue order.  One whose two lane halves are both masked multiplies zeros:
    it adds +0 to accumulators that are never -0 (they start at +0, and x + y is -0 only if both are), so it changes no bit."""
    return [[pair for pair in wave if pair != (None, None)] for wave in _visits(K, KT)]


def test_mfma_order_per_accumulator_is_the_same_for_both_trip_lengths():
    for K in range(0, 1101):
        assert _order(K, 32) == _order(K, 64), K


def test_each_lane_half_feeds_increasing_k_within_its_wave_slice():
    """The row sums add a lane's registers in issue order: the order of k per lane half is the same for both trip lengths and
    every k stays inside its wave's slice."""
    for KT in (32, 64):
        for K in (1, 7, 8, 9, 100, 255, 256, 257, 300, 1020, 1024):
            kq = (((K + 3) // 4) + 7) & ~7
            for w, wave in enumerate(G.slice_visits(K, KT)):
                for h in (0, 1):
                    ks = [pair[h] for pair in wave if pair[h] is not None]
                    assert ks == sorted(ks) and all(w * kq <= k < min(K, (w + 1) * kq) for k in ks), (K, KT, w, h)


def test_wide_switch_sits_at_256():
    src = open(SOURCE).read()
    assert re.findall(r"const bool wide = (\w+) >= (\d+);", src) == [("K", str(G.WIDE_K)), ("kmax", str(G.WIDE_K))]
    assert re.search(r"if \(wide\) gemm_strided_kernel<AK, BK, 64>", src) and re.search(r"else gemm_strided_kernel<AK, BK, 32>", src)
    assert re.search(r"if \(wide\) gemm_batched_kernel<AK, BK, 64>", src) and re.search(r"else gemm_batched_kernel<AK, BK, 32>", src)
    assert G.WIDE_K == 256 and G.trip_length(255) == 32 and G.trip_length(256) == 64
    assert 255 in G.K_SWEEP and 256 in G.K_SWEEP and 257 in G.K_SWEEP


# ---- the reference -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(100, 257, 319), (256, 64, 1024), (5, 3, 0)])
def test_expected_matches_an_independent_float64_einsum(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    A, B, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    c64 = torch.einsum("ik,jk->ij", A.double(), B.double()) + bias.double()
    bound = (K + 2) * G.U * (torch.einsum("ik,jk->ij", A.double().abs(), B.double().abs()) + bias.double().abs())
    assert bool(((G.expected(A, B, bias).double() - c64).abs() <= bound).all())
    assert bool(((G.rowsum(A).double() - A.double().sum(1)).abs() <= (K + 2) * G.U * A.double().abs().sum(1)).all())


def test_expected_applies_bias_accumulate_act_dact_in_the_documented_order():
    A = torch.tensor([[1.0, 2.0], [-3.0, 1.0]])
    B = torch.tensor([[1.0, 1.0], [2.0, -1.0]])                     # products [[3, 0], [-2, -7]]
    bias, c0 = torch.tensor([1.0, -1.0]), torch.tensor([[0.0, 2.0], [-1.0, 3.0]])
    ref = torch.tensor([[0.5, 0.0], [0.25, 1.0]])
    pre = torch.tensor([[4.0, 1.0], [-2.0, -5.0]])
    assert torch.equal(G.expected(A, B, bias, c0, accumulate=1), pre)
    assert torch.equal(G.expected(A, B, bias, c0, act=1, accumulate=1), pre.clamp(min=0))
    leaky = G.expected(A, B, bias, c0, act=2, accumulate=1)
    c = torch.tensor(0.01, dtype=torch.float32)                     # fp32(0.01) * v, one rounding
    assert torch.equal(leaky, torch.stack([pre[0], torch.stack([c * pre[1, 0], c * pre[1, 1]])]))
    assert float(leaky[1, 1]) == float(torch.tensor(float(c) * -5.0, dtype=torch.float32))   # the double product, rounded once
    assert torch.equal(G.expected(A, B, bias, c0, ref, act=1, dact=1, accumulate=1), torch.tensor([[4.0, 0.0], [0.0, 0.0]]))
    assert torch.equal(G.expected(A, B, bias, c0, ref, dact=3, accumulate=1), pre * torch.tensor([[0.25, 0.0], [0.1875, 0.0]]))
    # act before dact: sigmoid(v) * y (1 - y), not sigmoid(v * y (1 - y))
    s = G.expected(A, B, bias, c0, ref, act=3, dact=3, accumulate=1)
    assert torch.allclose(s.double(), torch.sigmoid(pre.double()) * (ref * (1 - ref)).double(), rtol=1e-6, atol=0)
    assert torch.equal(G.rowsum(A), torch.tensor([3.0, -2.0]))


def test_integer_partial_sums_stay_exact():
    """Every partial sum of the exact cases is an integer below 2^24: any summation order gives the same bits."""
    for K in G.K_SWEEP + G.K_PRODUCT + (1024,):                    # 1024: the batched grad-weight launch; colsum: 1000 rows
        assert G.max_partial_sum(K, G.INT_RANGE) < 2 ** 24, K
    assert G.max_partial_sum(max(G.K_SWEEP), G.INT_RANGE) == 16 * 1024 + 8
    assert G.max_partial_sum(256, 1) < 2 ** 24                      # the sigmoid cases' pre-activation
    assert G.INT_RANGE * 1024 < 2 ** 24 and G.INT_RANGE * 1000 < 2 ** 24      # row sums, column sums
    # the worst case is reached, not only bounded: all-4 inputs at the largest K, in float32, in the kernel's slice order
    K = max(G.K_SWEEP)
    acc = torch.zeros((), dtype=torch.float32)
    for wave in G.slice_visits(K, G.trip_length(K)):
        part = torch.zeros((), dtype=torch.float32)
        for pair in wave:
            for k in pair:
                if k is not None:
                    part = part + torch.tensor(16.0)
                    assert float(part) < 2 ** 24
        acc = acc + part
    assert float(acc + 8.0) == G.max_partial_sum(K)
    for y in G.DYADIC:                                              # y (1 - y) is exact in fp32
        t = torch.tensor(y, dtype=torch.float32)
        assert float(t * (1 - t)) == y * (1 - y)


# ---- argument checks: made-up addresses that are never dereferenced; every case fails a check and no launch follows one ------

def _fused(**over):
    a = dict(A=C.c_void_p(0x10000), sa0=64, sa1=1, B=C.c_void_p(0x20000), sb0=64, sb1=1, bias=None, Cp=C.c_void_p(0x30000),
             ldc=64, M=32, N=32, K=64, acc=0, act=0, dact=0, ref=None, ld_ref=0, rowsum=None)
    a.update(over)
    return _lib.load().ns_gemm_fused(a["A"], a["sa0"], a["sa1"], a["B"], a["sb0"], a["sb1"], a["bias"], a["Cp"], a["ldc"], a["M"],
                                     a["N"], a["K"], a["acc"], a["act"], a["dact"], a["ref"], a["ld_ref"], a["rowsum"], None)


@pytest.mark.parametrize("over", [
    dict(M=-1), dict(N=-1), dict(K=-1), dict(act=4), dict(act=-1), dict(dact=4), dict(dact=-1), dict(dact=1),
    dict(dact=1, M=0), dict(A=None), dict(B=None), dict(Cp=None),
])
def test_fused_bad_arguments_are_invalid(over):
    assert _fused(**over) == -1
    assert b"ns_gemm_fused:" in _lib.load().ns_last_error()


@pytest.mark.parametrize("over", [dict(M=0), dict(N=0), dict(M=0, N=0, A=None, B=None, Cp=None)])
def test_fused_empty_output_returns_ok_without_a_launch(over):
    assert _fused(**over) == 0


def _problem(**over):
    q = _lib.GemmProblem()
    q.A_dev, q.sa0, q.sa1 = 0x10000, 64, 1
    q.B_dev, q.sb0, q.sb1 = 0x20000, 64, 1
    q.bias_dev = None
    q.C_dev, q.ldc = 0x30000, 64
    q.M, q.N, q.K = 32, 32, 64
    q.accumulate, q.act, q.dact = 0, 0, 0
    q.dact_ref_dev, q.ld_ref = None, 0
    q.a_rowsum_dev = None
    for k, v in over.items():
        setattr(q, k, v)
    return q


def _batched(problems, count=None):
    arr = (_lib.GemmProblem * max(len(problems), 1))(*problems)
    return _lib.load().ns_gemm_fused_batched(arr, len(problems) if count is None else count, None)


@pytest.mark.parametrize("problems,count", [
    ([_problem()], 0),
    ([_problem()] * 5, 5),
    ([_problem()], -1),
    ([_problem(M=0)], None),
    ([_problem(), _problem(N=0)], None),
    ([_problem(K=-1)], None),
    ([_problem(A_dev=None)], None),
    ([_problem(act=4)], None),
    ([_problem(dact=2)], None),
    ([_problem(), _problem(sa0=1, sa1=64)], None),                 # sa1 == 1 differs
    ([_problem(), _problem(sb0=1, sb1=64)], None),                 # sb1 == 1 differs
    ([_problem(sa0=1, sa1=64, sb0=1, sb1=64), _problem(sa0=1, sa1=64, sb0=1, sb1=64), _problem()], None),
])
def test_batched_bad_arguments_are_invalid(problems, count):
    assert _batched(problems, count) == -1
    assert b"ns_gemm_fused_batched:" in _lib.load().ns_last_error()


def test_batched_null_table_is_invalid():
    assert _lib.load().ns_gemm_fused_batched(None, 1, None) == -1
    assert b"ns_gemm_fused_batched:" in _lib.load().ns_last_error()


# ---- the binding -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ns_gemm_fused", "ns_gemm_fused_batched", "ns_colsum", "ns_adam_step_multi_dev"])
def test_header_argument_counts_match_the_binding(name):
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, f"{name} is not declared in the header"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert len(_lib.SIGNATURES[name][1]) == n_args
    assert hasattr(_lib.load(), name)


def _c_struct_layout(name):
    """[(field, offset)], size of `typedef struct name {...}` in the header: pointers and int64_t 8 bytes, int and float 4,
    every field at its natural alignment, the size rounded up to the widest one."""
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), _header(), flags=re.S)
    assert m, f"struct {name} is not declared in the header"
    fields, off, widest = [], 0, 1
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if "*" in decl:
            size, names = 8, decl.rsplit("*", 1)[1]
        else:
            ctype, names = re.match(r"(?:const\s+)?(\w+)\s+(.*)", decl).groups()
            size = {"int64_t": 8, "int": 4, "float": 4}[ctype]
        for field in names.split(","):
            off = (off + size - 1) // size * size
            fields.append((field.strip(), off))
            off += size
            widest = max(widest, size)
    return fields, (off + widest - 1) // widest * widest


def test_gemm_problem_struct_layout_matches_the_header():
    fields, size = _c_struct_layout("ns_gemm_problem")
    assert C.sizeof(_lib.GemmProblem) == size
    assert [f for f, _ in fields] == [f for f, _ in _lib.GemmProblem._fields_]
    for field, off in fields:
        assert getattr(_lib.GemmProblem, field).offset == off, field


def test_adam_table_row_is_five_words():
    """tests/test_gpu_gemm_tile.py builds the ns_adam_tensor table as an int64 tensor of five columns."""
    fields, size = _c_struct_layout("ns_adam_tensor")
    assert [f for f, _ in fields] == ["p", "g", "m", "v", "n"] and [o for _, o in fields] == [0, 8, 16, 24, 32] and size == 40
