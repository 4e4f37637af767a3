"""raw2outputs at every sample count and lane layout against float64, ns_raw2outputs_strided through ctypes, and inverse-CDF
sampling / importance_z at every kernel size (run with -m gpu on an MI355X).

The compositing bounds are the error model of tests/composite_bounds.py (formulas in N stated there); tests/test_composite_bounds.py
shows on the CPU that they reject float32 mutants of the oracle.  Measured on the MI355X, worst |err| / bound per layout (every
bound is within 8x of the worst value measured for it: the sweep's maxima are 1.00, 0.71, 0.22, 0.37, 0.48, 0.16):
                     alphas  weights  acc    depth  rgb    disp
    single (N = 1)   -       -        exact  exact  0.478  1e10
    sw2              0.500   0.500    0.138  0.147  0.245  0.069
    sw4              0.500   0.500    0.169  0.174  0.311  0.115
    sw8              0.500   0.500    0.101  0.237  0.163  0.115
    sw16             0.593   0.500    0.111  0.200  0.281  0.078
    sw32             0.500   0.500    0.100  0.186  0.152  0.132
    sw64             0.501   0.500    0.104  0.146  0.154  0.087
    chunks (N > 64)  0.876   0.500    0.077  0.126  0.129  0.049
    grid stride      0.998   0.713    0.223  0.374  0.346  0.164    (N = 2, 3, 9, 17, 33, 65; ~1e6 samples each)
"""

import ctypes as C

import numpy as np
import pytest
import torch

import composite_bounds as CB
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from nerf_sampling_amd import ops as _ops

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    """Bit for bit where the values are numbers, NaN at the same entries (a NaN's sign and payload carry no meaning)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(_bits(torch.where(na, 0.0, a)), _bits(torch.where(nb, 0.0, b)))


def _run_and_check(ops, N, R, seed, worst):
    for with_noise in (False, True):
        raw, z, d, noise = CB.make_inputs(R, N, seed, with_noise)
        rd, zd, dd = raw.cuda(), z.cuda(), d.cuda()
        nd = None if noise is None else noise.cuda()
        outs = {}
        for white in (False, True):
            got = ops.raw2outputs(rd, zd, dd, nd, white)
            lean = ops.raw2outputs(rd, zd, dd, nd, white, want_per_sample=False)
            for a, b in zip(got[:4], lean[:4]):           # the per-sample outputs change nothing else
                assert torch.equal(_bits(a), _bits(b)), (N, R, white, with_noise)
            assert lean[4] is None and lean[5] is None
            stats = CB.check(got, raw, z, d, noise, white)
            for k, v in stats.items():
                w = worst.setdefault(k, [0.0, 0.0])
                w[0], w[1] = max(w[0], v[0]), max(w[1], v[1])
            outs[white] = got
        # white background = black background + (1 - acc), bit for bit in fp32 on the device (N = 1: no background at all)
        rgb_b, acc = outs[False][0], outs[False][2]
        exp_white = rgb_b if N == 1 else rgb_b + (1.0 - acc)[:, None]
        assert _same_bits(outs[True][0], exp_white), (N, R, with_noise, int((outs[True][0] != exp_white).sum()),
                                                      int(torch.isnan(exp_white).sum()))
        for k in (1, 2, 3, 4, 5):
            assert _same_bits(outs[True][k], outs[False][k]), (N, R, with_noise, k)


LAYOUTS = {}
for _n in CB.SWEEP:
    LAYOUTS.setdefault(CB.layout_name(_n), []).append(_n)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_raw2outputs_against_float64(ops, layout):
    """Every N of the layout, R = 3 (256 / SW) + 1 rays (a partial last block), both backgrounds, with and without noise."""
    worst = {}
    for N in LAYOUTS[layout]:
        _run_and_check(ops, N, CB.rays_for(N), seed=1000 + N, worst=worst)
    print(f"\nraw2outputs {layout} (N = {LAYOUTS[layout][0]}..{LAYOUTS[layout][-1]}): worst |err| / bound, max |err|: "
          + ", ".join(f"{k} {v[0]:.3f} {v[1]:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("N", [2, 3, 9, 17, 33, 65])
def test_raw2outputs_grid_stride(ops, N):
    """The smallest N of each layout with 2 * 4096 * (256 / SW) + 5 rays: every thread runs at least two grid-stride passes
    (the software-pipelined prefetch of the next ray's inputs)."""
    sw = CB.lane_width(N)
    worst = {}
    _run_and_check(ops, N, 2 * 4096 * (256 // sw) + 5, seed=2000 + N, worst=worst)
    print(f"\nraw2outputs grid stride N = {N}: " + ", ".join(f"{k} {v[0]:.3f} {v[1]:.2e}" for k, v in worst.items()))


# ---- ns_raw2outputs_strided through the C ABI ------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("N", [1, 8, 130])
def test_raw2outputs_strided_writes_only_its_columns(ops, N):
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    R = 301
    raw, z, d, _ = CB.make_inputs(R, N, seed=N, with_noise=False)
    raw, z, d = raw.cuda(), z.cuda(), d.cuda()
    ref = ops.raw2outputs(raw, z, d, None, True)
    n_out = 0 if N == 1 else N
    for rgb_stride in (4, 7):
        for disp_stride in (1, 4):
            for per_sample in (True, False):
                rgb = torch.full((R, rgb_stride), -7.0, device="cuda")
                disp = torch.full((R, disp_stride), -7.0, device="cuda")
                acc, depth = torch.full((R,), -7.0, device="cuda"), torch.full((R,), -7.0, device="cuda")
                alphas, weights = torch.full((R, n_out), -7.0, device="cuda"), torch.full((R, n_out), -7.0, device="cuda")
                extra = (_p(acc), _p(depth), _p(alphas), _p(weights)) if per_sample else (None, None, None, None)
                rc = lib.ns_raw2outputs_strided(_p(raw), _p(z), _p(d), None, R, N, 1, _p(rgb), rgb_stride, _p(disp), disp_stride,
                                                *extra, None)
                torch.cuda.synchronize()
                tag = (N, rgb_stride, disp_stride, per_sample)
                assert rc == 0, (tag, lib.ns_last_error())
                assert torch.equal(_bits(rgb[:, :3]), _bits(ref[0])), tag
                assert bool((rgb[:, 3:] == -7.0).all()), tag
                assert torch.equal(_bits(disp[:, 0]), _bits(ref[1])), tag
                assert bool((disp[:, 1:] == -7.0).all()), tag
                if per_sample:
                    for got, exp in ((acc, ref[2]), (depth, ref[3]), (alphas, ref[4]), (weights, ref[5])):
                        assert torch.equal(_bits(got), _bits(exp)), tag
                else:
                    for t in (acc, depth, alphas, weights):
                        assert bool((t == -7.0).all()), tag


def test_raw2outputs_strided_refuses_before_any_launch(ops):
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    R, N = 64, 8
    raw, z, d, _ = CB.make_inputs(R, N, seed=3, with_noise=False)
    base = torch.zeros(R * N * 4 + 4, device="cuda")
    base[4:] = raw.reshape(-1).cuda()
    raw_off = base[1:]                                         # 4 bytes off the 16-byte alignment of the allocation
    raw, z, d = raw.cuda(), z.cuda(), d.cuda()
    rgb = torch.full((R, 4), -7.0, device="cuda")
    disp = torch.full((R, 4), -7.0, device="cuda")
    acc = torch.full((R,), -7.0, device="cuda")

    def call(raw_t, n, rgb_stride, disp_stride, r=R):
        return lib.ns_raw2outputs_strided(_p(raw_t), _p(z), _p(d), None, r, n, 0, _p(rgb), rgb_stride, _p(disp), disp_stride,
                                          _p(acc), None, None, None, None)

    assert raw_off.data_ptr() % 16 == 4
    for args in ((raw, N, 2, 1), (raw, N, 4, 0), (raw, 0, 4, 1), (raw_off, N, 4, 1)):
        assert call(*args) == -1, args                          # NS_E_INVALID
        assert b"ns_raw2outputs_strided" in lib.ns_last_error()
    assert call(raw, N, 4, 4, r=0) == 0                          # nothing to do
    torch.cuda.synchronize()
    assert bool((rgb == -7.0).all()) and bool((disp == -7.0).all()) and bool((acc == -7.0).all())


# ---- inverse-CDF sampling -----------------------------------------------------------------------------------------------
def _statistical(mine, exp, frac=2e-3):
    """The inverse CDF is continuous in u except where a bin's mass is below the reference's 1e-5 floor: a few samples may land
    in the neighbouring bin (the allowance of test_gpu_kernels.py::test_sample_pdf)."""
    err = (mine.cpu().double() - exp.double()).abs().numpy()
    assert np.mean(err > 2e-5) < frac, float(np.mean(err > 2e-5))
    assert np.median(err) < 1e-6, float(np.median(err))


def _weights(R, Nb, gen):
    w = torch.rand(R, Nb - 1, generator=gen) ** 3
    w[0] = 0.0                                                   # all mass from the 1e-5 floor
    w[1] = 0.0
    w[1, (Nb - 1) // 2] = 1.0                                    # one-hot
    w[2] = 10.0 ** (-8.0 * torch.rand(Nb - 1, generator=gen))     # a 1e8 dynamic range
    return w


def _bins(R, Nb, gen):
    b = torch.sort(2.0 + 4.0 * torch.rand(R, Nb, generator=gen), -1).values
    if Nb >= 3:
        b[3, 1] = b[3, 0]                                        # duplicate edges
        b[3, -1] = b[3, -2]
    return b


@pytest.mark.parametrize("Nb", [2, 3, 64, 65, 66, 129, 512])
def test_sample_pdf_shapes(ops, Nb):
    gen = torch.Generator().manual_seed(Nb)
    R = 1024
    bins, w = _bins(R, Nb, gen), _weights(R, Nb, gen)
    for Nf in (0, 1, 64, 65, 300):
        for random_u in (False, True):
            u = torch.rand(R, Nf, generator=gen) if random_u else None
            mine = ops.sample_pdf(bins.cuda(), w.cuda(), Nf, None if u is None else u.cuda()).cpu()
            exp = O.sample_pdf(bins, w, Nf, det=True, u=u)
            assert mine.shape == (R, Nf)
            if Nf == 0:
                continue
            tag = (Nb, Nf, random_u)
            assert bool(((mine >= bins[:, :1]) & (mine <= bins[:, -1:])).all()), tag
            if not random_u:
                assert bool((mine[:, 1:] >= mine[:, :-1]).all()), tag
            _statistical(mine, exp)


def test_sample_pdf_edge_draws(ops):
    """u = 0, u = 1 and u equal to a CDF value of the oracle (searchsorted right=True: the boundary belongs to the next bin)."""
    gen = torch.Generator().manual_seed(11)
    R, Nb = 1024, 33
    bins, w = _bins(R, Nb, gen), _weights(R, Nb, gen)
    wf = w + 1e-5
    cdf = torch.cat([torch.zeros(R, 1), torch.cumsum(wf / wf.sum(-1, keepdim=True), -1)], -1)
    u = torch.cat([torch.zeros(R, 1), torch.ones(R, 1), cdf[:, 1:-1]], -1).contiguous()
    mine = ops.sample_pdf(bins.cuda(), w.cuda(), u.shape[1], u.cuda()).cpu()
    assert bool(((mine >= bins[:, :1]) & (mine <= bins[:, -1:])).all())
    assert torch.equal(mine[:, 0], bins[:, 0])                    # u = 0: the first edge, exactly (t = 0)
    # every draw sits on a bin boundary, where the inverse CDF jumps if the bin's mass is below the 1e-5 floor.  The kernel's CDF
    # is normalised by a sum in another order, so its boundaries lie within 32 ulps of 1 of the oracle's (the normalised terms
    # round once each, the sums in double): the inverse CDF is non-decreasing in u, so each sample lies between the oracle's
    # values at u -+ 32 * 2^-24
    du = 32 * 2.0 ** -24
    lo = O.sample_pdf(bins, w, u.shape[1], u=(u - du).clamp(0.0, 1.0).contiguous())
    hi = O.sample_pdf(bins, w, u.shape[1], u=(u + du).clamp(0.0, 1.0).contiguous())
    hi = torch.where(u + du >= 1.0, bins[:, -1:].expand_as(hi), hi)   # whether u lies past the last CDF value (the clamp to
    ok = (mine >= lo - 2e-5) & (mine <= hi + 2e-5)                      # the last edge) turns on how that value rounds
    # a bin whose mass lies within du of the 1e-5 floor may take either side of `denom < 1e-5` (interpolate, or stay at the
    # lower edge): a draw on its boundaries may land anywhere in the two bins around that boundary
    mass = cdf[:, 1:] - cdf[:, :-1]
    near_floor = ((mass - 1e-5).abs() <= du).float()
    j = torch.arange(2, u.shape[1])                                     # column c holds u = cdf[c - 1] (c >= 2)
    amb = torch.zeros_like(ok)
    amb[:, 2:] = (near_floor[:, j - 2] + near_floor[:, (j - 1).clamp(max=Nb - 2)]) > 0
    lo2 = torch.cat([bins[:, :2], bins[:, 0:Nb - 2]], -1)               # bins[c - 2] for column c
    hi2 = torch.cat([bins[:, :2], bins[:, 2:Nb].clone()], -1)           # bins[c] for column c (the last edge at the top)
    ok |= amb & (mine >= lo2) & (mine <= hi2)
    if not bool(ok.all()):
        r, c = [int(v) for v in (~ok).nonzero()[0]]
        raise AssertionError(f"{int((~ok).sum())} draws outside; row {r} col {c}: u {float(u[r, c])!r} mine {float(mine[r, c])!r} "
                             f"lo {float(lo[r, c])!r} hi {float(hi[r, c])!r} at-u {float(O.sample_pdf(bins, w, u.shape[1], u=u)[r, c])!r} "
                             f"bins {bins[r, max(c - 3, 0):c + 2].tolist()} w {w[r, max(c - 3, 0):c + 2].tolist()} cdf {cdf[r, max(c - 3, 0):c + 2].tolist()}")
    # ... and away from the jumps, where the inverse CDF is continuous, they agree with the oracle at u itself
    _statistical(mine, O.sample_pdf(bins, w, u.shape[1], u=u), 0.05)


@pytest.mark.parametrize("Nc,Nf", [(65, 10), (100, 150), (200, 700), (513, 1535)])
def test_importance_z_lds_kernel_sizes(ops, Nc, Nf):
    """The LDS kernel at P = 128, 256, 1024 and 2048 (512 bins, 2048 samples: both limits)."""
    gen = torch.Generator().manual_seed(Nc + Nf)
    R = 67
    zc = torch.sort(2.0 + 4.0 * torch.rand(R, Nc, generator=gen), -1).values
    w = torch.cat([torch.rand(R, 1, generator=gen), _weights(R, Nc - 1, gen), torch.rand(R, 1, generator=gen)], -1)[:, :Nc]
    z_mid = 0.5 * (zc[..., 1:] + zc[..., :-1])
    for random_u in (False, True):
        u = torch.rand(R, Nf, generator=gen) if random_u else None
        mine = ops.importance_z(zc.cuda(), w.contiguous().cuda(), Nf, None if u is None else u.cuda()).cpu()
        samples = O.sample_pdf(z_mid, w[..., 1:-1], Nf, det=True, u=u)
        ref = torch.sort(torch.cat([zc, samples], -1), -1).values
        assert mine.shape == (R, Nc + Nf) and torch.isfinite(mine).all()
        assert bool((mine[:, 1:] >= mine[:, :-1]).all())
        # every coarse depth is in its row, bit for bit (multiset inclusion)
        for r in range(R):
            vals, counts = torch.unique(_bits(mine[r]), return_counts=True)
            have = dict(zip(vals.tolist(), counts.tolist()))
            cv, cc = torch.unique(_bits(zc[r]), return_counts=True)
            assert all(have.get(v, 0) >= c for v, c in zip(cv.tolist(), cc.tolist())), (Nc, Nf, r)
        assert bool(((mine >= zc[:, :1]) & (mine <= zc[:, -1:])).all())
        _statistical(mine, ref, 5e-3)          # (the allowance of test_gpu_kernels.py::test_importance_z_shapes)


def test_importance_z_limits(ops):
    for Nc, Nf in ((514, 0), (64, 1985)):
        with pytest.raises(ValueError):
            ops.importance_z(torch.rand(4, Nc).sort(-1).values.cuda(), torch.rand(4, Nc).cuda(), Nf)
