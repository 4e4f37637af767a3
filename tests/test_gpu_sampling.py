"""Hierarchical sampling sample by sample (run with -m gpu on an MI355X): ops.sample_pdf against the float64 reference and error
model of tests/sampling_bounds.py at every draw; ops.importance_z bit for bit against sort(cat[z, ops.sample_pdf(z_mid, ...)]) for
every sort implementation (the wave kernel's one-merge shortcut and full register network at NR = 1, 2, 4, the LDS network), which
with the bound on ops.sample_pdf at bins = z_mid places every fine sample; ns_sort_rows exactly against torch.sort, in place too.

No share of the entries is forgiven: tests/test_sampling_bounds_host.py shows on the CPU that this comparison accepts the fp32
oracle everywhere and rejects a kernel that gets a single draw of a single ray wrong."""

import ctypes as C

import pytest
import torch

import sampling_bounds as SB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from nerf_sampling_amd import ops as _ops

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def _bits(x):
    return x.contiguous().view(torch.int32)


def _assert_same_bits(a, b, tag):
    """Bit for bit where the values are numbers, NaN at the same entries (a NaN's sign and payload carry no meaning)."""
    assert a.shape == b.shape, (tag, tuple(a.shape), tuple(b.shape))
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        r, s = (int(v) for v in (na ^ nb).nonzero()[0])
        raise AssertionError(f"{tag}: NaN pattern differs in {int((na ^ nb).sum())} entries; row {r} entry {s}: "
                             f"{float(a[r, s])!r} against {float(b[r, s])!r} ({int(na[r].sum())} / {int(nb[r].sum())} NaNs in that row)")
    diff = _bits(torch.where(na, 0.0, a)) != _bits(torch.where(nb, 0.0, b))
    if bool(diff.any()):
        r, s = (int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{tag}: {int(diff.sum())} entries differ; row {r} entry {s}: {float(a[r, s])!r} != {float(b[r, s])!r}")


def _dev(t):
    return None if t is None else t.cuda()


def _check_bound(samples, c, tag):
    got = samples.cpu()
    rej, worst = SB.compare(got, c.ref, c.planted)
    print(f"\n{tag}: worst |err| / e = {worst:.3f} over {int((~c.ref.loose | c.planted).sum())} strict draws, "
          f"{int((c.ref.loose & ~c.planted).sum())} loose")
    assert rej.shape[0] == 0, (tag, SB.describe(rej, got, c.ref, c.u_eff))


# ---- ops.sample_pdf against ref64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("explicit", [False, True], ids=["linspace", "explicit"])
@pytest.mark.parametrize("R,Nb,Nf", SB.CASES_PDF)
def test_sample_pdf_every_sample(ops, R, Nb, Nf, explicit):
    """Regimes A, C and D stacked in one call; R = 8195 walks sample_pdf_kernel's ray loop twice (the grid stops at 8192)."""
    c = SB.make_case(R, Nb, Nf, explicit)
    got = ops.sample_pdf(_dev(c.bins), _dev(c.w), Nf, _dev(c.u))
    assert got.shape == (R, Nf)
    _check_bound(got, c, f"sample_pdf_kernel R={R} Nb={Nb} Nf={Nf} {'explicit' if explicit else 'linspace'}")


# ---- ops.importance_z = sort(cat[z, ops.sample_pdf(z_mid, w[:, 1:-1])]), bit for bit ------------------------------------------
def _relation(ops, z, w, Nf, u, tag):
    got = ops.importance_z(z, w, Nf, u)
    z_mid = (0.5 * (z[:, 1:] + z[:, :-1])).contiguous()
    samples = ops.sample_pdf(z_mid, w[:, 1:-1].contiguous(), Nf, u)
    # sorted on the host, NaN last: torch.sort on the device put the NaN samples of a row of 64 entries or more first
    exp = torch.sort(torch.cat([z, samples], -1).cpu(), -1).values
    _assert_same_bits(got.cpu(), exp, tag)
    return got, z_mid, samples


@pytest.mark.parametrize("explicit", [False, True], ids=["linspace", "explicit"])
@pytest.mark.parametrize("R,Nc,Nf", SB.CASES_IMPORTANCE)
def test_importance_z_every_sample(ops, R, Nc, Nf, explicit):
    """R = 32773 at (4, 4): the wave grid stops at 8192 workgroups of four rays; R = 8195 at (65, 3): the LDS kernel's at 8192 rays."""
    c = SB.make_case(R, Nc - 1, Nf, explicit, True)
    kernel = SB.kernel_of(Nc, Nf)
    tag = f"importance_z {kernel} R={R} Nc={Nc} Nf={Nf} {'explicit' if explicit else 'linspace'}"
    z, w, u = _dev(c.z), _dev(c.w_full), _dev(c.u)
    got, z_mid, samples = _relation(ops, z, w, Nf, u, tag)
    assert got.shape == (R, Nc + Nf)
    assert torch.equal(z_mid.cpu(), c.bins)
    # the ray with a NaN weight: its sorted coarse depths, then Nf NaNs
    for r in SB.special_rows(c, SB.ROW_NAN):
        row = got[r].cpu()
        assert torch.equal(_bits(row[:Nc]), _bits(c.z[r])) and bool(row[Nc:].isnan().all()), (tag, r)
    if Nf > 0:
        _check_bound(samples, c, tag + " (ops.sample_pdf on z_mid)")
    if not explicit:
        # descending coarse depths: the wave kernel finds its coarse run out of order and sorts with the full network
        _relation(ops, z.flip(-1).contiguous(), w, Nf, None, tag + " descending z")


# ---- ns_sort_rows -----------------------------------------------------------------------------------------------------------
def _sort_input(R, N):
    g = torch.Generator().manual_seed(7 * N + R)
    x = torch.randn(R, N, generator=g)
    x[::2] = torch.round(x[::2] * 4.0) / 4.0 + 0.0               # every other row: few distinct values, many duplicates (no -0)
    x[torch.rand(R, N, generator=g) < 0.05] = float("nan")
    x[0] = float("nan")
    x[1] = 1.5
    x[2] = torch.arange(N, 0, -1, dtype=torch.float32)           # descending
    return x


@pytest.mark.parametrize("R,N", [(67, 513), (67, 1024), (67, 1025), (67, 2048), (8195, 3)])
def test_sort_rows_exact(ops, R, N):
    x = _sort_input(R, N)
    got = ops.sort_rows(x.cuda()).cpu()
    _assert_same_bits(got, torch.sort(x, -1).values, f"sort_rows R={R} N={N}")


@pytest.mark.parametrize("N", [65, 2048])
def test_sort_rows_in_place(ops, N):
    """out aliasing x, as the gaussian mode of ns_place_samples calls it."""
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    R = 67
    x = _sort_input(R, N)
    xd = x.cuda()
    torch.cuda.synchronize()
    p = C.c_void_p(xd.data_ptr())
    rc = lib.ns_sort_rows(p, R, N, p, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.ns_last_error()
    _assert_same_bits(xd.cpu(), torch.sort(x, -1).values, f"sort_rows in place N={N}")
