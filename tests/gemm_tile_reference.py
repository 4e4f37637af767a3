"""The tile GEMM (ns_gemm_fused, csrc/ns_train.hip) restated plainly: the expected result, the row sums and the kernel's index
arithmetic.

Shared by tests/test_gemm_tile_host.py (the index arithmetic and the argument checks, on the CPU) and
tests/test_gpu_gemm_tile.py (the HIP kernels).  Nothing here calls the library.

The operation, in the kernel's documented order:

    acc      = sum_k A[i, k] B[j, k]                     (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 sums)
    v        = acc (+ bias[j]) (+ C[i, j] if accumulate)
    v        = act(v)             act 0 none, 1 v < 0 ? 0 : v, 2 v > 0 ? v : float32(0.01) * v, 3 1 / (1 + expf(-v))
                                  (a NaN stays NaN under every one of them, as under torch.relu: row NAN_ROW of the NaN case)
    C[i, j]  = v * act'(dact)     evaluated from the activation OUTPUT y = dact_ref[i, j]:
                                  dact 1: y > 0 ? 1 : 0,  2: y > 0 ? 1 : float32(0.01),  3: y * (1 - y)
    a_rowsum[i] = sum_k A[i, k]

Exact cases.  With integer inputs in [-R, R] every product is an integer of at most R^2 and every partial sum of any order is
an integer of at most R^2 K + 2 R (bias and accumulate seed included): below 2^24 it is held exactly, so the summation order
does not matter and `expected` -- the product in float64, converted to float32 -- is the only correct result.  What follows the
sum is one IEEE operation per step on both sides (the library is built with -ffp-contract=off: the leaky multiply and the
multiply by act' are never fused with anything), so the comparison is bit for bit.  `max_partial_sum` is that bound;
tests/test_gemm_tile_host.py asserts it for every range and K the GPU tests use.

The sigmoid (act 3) is the one step that is not exact: `expected` evaluates it in float32 on the CPU as the kernel writes it,
which the GPU's expf need not match in the last bits; the GPU tests compare that case with float64 under `sigmoid_bound`.
"""

import torch

U = 2.0 ** -24
LEAKY = torch.tensor(0.01, dtype=torch.float32)

# the integer range of the exact cases, the values of an activation output that keep y (1 - y) exact, and the K of the sweep
INT_RANGE = 4
DYADIC = (0.0, 0.25, 0.5, 0.75, 1.0)
K_SWEEP = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 129, 255, 256, 257, 319, 1020, 1024)
K_PRODUCT = (7, 64, 300)
SIZES = ((1, 1), (31, 33), (32, 32), (33, 31), (65, 100), (100, 257), (64, 1))
NAN_ROW = 37          # the row of A that holds a NaN in the relu-keeps-NaN cases (not the first row of a 32-row tile)
WIDE_K = 256        # ns_gemm_fused: K >= WIDE_K runs trips of 64 k per wave, below it trips of 32


def trip_length(K):
    """KT of the launch for a (largest) K."""
    return 64 if K >= WIDE_K else 32


def max_partial_sum(K, rng=INT_RANGE):
    """Largest magnitude any partial sum of the GEMM (bias and accumulate seed included) can reach on integers in [-rng, rng]."""
    return rng * rng * K + 2 * rng


def _f32(x):
    return None if x is None else x.detach().cpu().to(torch.float32)


def act_apply(v, act):
    """The forward activation as float32 torch operations on the CPU."""
    if act == 0:
        return v
    if act == 1:
        return torch.clamp(v, min=0.0)
    if act == 2:
        return torch.where(v > 0, v, LEAKY * v)
    if act == 3:
        return 1.0 / (1.0 + torch.exp(-v))
    raise ValueError(act)


def dact_factor(y, dact):
    """act'(.) of activation `dact` from its output y (float32)."""
    one = torch.ones_like(y)
    if dact == 1:
        return torch.where(y > 0, one, torch.zeros_like(y))
    if dact == 2:
        return torch.where(y > 0, one, LEAKY * one)
    if dact == 3:
        return y * (1.0 - y)
    raise ValueError(dact)


def product(A, B):
    """A B^T for A [M, K], B [N, K]: taken in float64, converted to float32 (exact for the integer cases)."""
    return (_f32(A).double() @ _f32(B).double().t()).to(torch.float32)


def epilogue(prod, bias=None, c0=None, ref=None, act=0, dact=0, accumulate=0):
    """What ns_gemm_fused does with the finished sum, as float32 operations on the CPU: bias, accumulate (the seed c0), act, dact."""
    v = prod
    if bias is not None:
        v = v + _f32(bias)
    if accumulate:
        v = v + _f32(c0)
    v = act_apply(v, act)
    if dact:
        v = v * dact_factor(_f32(ref), dact)
    return v


def expected(A, B, bias=None, c0=None, ref=None, act=0, dact=0, accumulate=0):
    """C [M, N] of ns_gemm_fused for A [M, K], B [N, K] (float32, any device): `product`, then `epilogue`."""
    return epilogue(product(A, B), bias, c0, ref, act, dact, accumulate)


def rowsum(A):
    """a_rowsum [M] for A [M, K]: exact on the integers."""
    return _f32(A).double().sum(1).to(torch.float32)


def sigmoid_bound(v64):
    """|sigmoid32 - sigmoid64| for the exact pre-activation v: 8 * 2^-24 * sigma + 2^-126.  With e = expf(-v) within 2 ulp
    (4u relative) the quotient 1 / (1 + e) moves by sigma (1 - sigma) 4u <= 4u sigma; the add and the IEEE divide round once
    each (2u sigma): 6u sigma, taken as 8u.  The absolute term covers results in the denormal range."""
    return 8 * U * torch.sigmoid(v64) + 2.0 ** -126


def slice_visits(K, KT):
    """The index arithmetic of gemm_tile, restated: for each of the four waves the list of its MFMAs in issue order, each one
    the pair (k fed by lane half h = 0, k fed by lane half h = 1), None where the `k < kend` mask feeds a zero.

    Wave w owns k in [w kq, min(K, (w + 1) kq)) with kq = (((K + 3) / 4) + 7) & ~7; a trip starts at k0 and covers KT values of
    k; register e = 4 c + m of lane half h holds k = k0 + 8 c + 4 h + m; the MFMAs are issued in the order of e."""
    kq = (((K + 3) // 4) + 7) & ~7
    waves = []
    for wave in range(4):
        kbeg = wave * kq
        kend = min(K, kbeg + kq)
        issued = []
        k0 = kbeg
        while k0 < kend:
            reg = {}
            for c in range(KT // 8):
                for m in range(4):
                    for h in (0, 1):
                        k = k0 + 8 * c + 4 * h + m
                        reg[4 * c + m, h] = k if k < kend else None
            for e in range(KT // 2):
                issued.append((reg[e, 0], reg[e, 1]))
            k0 += KT
        waves.append(issued)
    return waves
