"""tests/sampling_bounds.py on the CPU, at every (R, Nb, Nf) the GPU tests use, with deterministic and explicit draws: the
generators meet their conditions, the fp32 oracle is accepted on every sample, and every fp32 mutant is rejected in every regime
it is listed for -- so a kernel that passes tests/test_gpu_sampling.py has placed every sample."""

import pytest
import torch

import sampling_bounds as SB

# (R, Nb, Nf, coarse): sample_pdf's cases on free bin edges, importance_z's on z_mid of coarse depths
CASES = sorted({(R, Nb, Nf, False) for R, Nb, Nf in SB.CASES_PDF} | {(R, Nc - 1, Nf, True) for R, Nc, Nf in SB.CASES_IMPORTANCE})
DRAWN = [c for c in CASES if c[2] > 0]
_worst = {}


def _ids(c):
    return f"R{c[0]}-Nb{c[1]}-Nf{c[2]}-{'zmid' if c[3] else 'bins'}"


@pytest.mark.parametrize("explicit", [False, True], ids=["linspace", "explicit"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_generators_meet_their_conditions(case, explicit):
    R, Nb, Nf, coarse = case
    c = SB.make_case(R, Nb, Nf, explicit, coarse)
    assert c.bins.shape == (R, Nb) and c.w.shape == (R, Nb - 1) and c.planted.shape == (R, Nf)
    assert c.bins.dtype == c.w.dtype == torch.float32 and c.sizes == [R - 2 * (R // 3), R // 3, R // 3]
    assert bool((c.bins[:, 1:] >= c.bins[:, :-1]).all()) and float(c.bins.min()) >= 2.0 and float(c.bins.max()) <= 6.0
    if coarse:
        assert torch.equal(c.bins, 0.5 * (c.z[:, 1:] + c.z[:, :-1])) and torch.equal(c.w_full[:, 1:-1].isnan(), c.w.isnan())
        assert bool((c.w_full[:, 1:-1][~c.w.isnan()] == c.w[~c.w.isnan()]).all())
    # the dynamic range behind the wave kernel's exact double scan
    v = c.ref.v[~c.ref.nan_row]
    assert float((v.max(-1).values / v.min(-1).values).max()) < 2.0 ** 28
    # the special rows are there
    assert c.ref.nan_row.nonzero().flatten().tolist() == SB.special_rows(c, SB.ROW_NAN)
    for r in SB.special_rows(c, SB.ROW_ZERO):
        assert bool((c.w[r] == 0).all())
    for r in SB.special_rows(c, SB.ROW_ONEHOT):
        assert int((c.w[r] != 0).sum()) == 1
    if Nb >= 3:
        for r in SB.special_rows(c, SB.ROW_DUP):
            assert float(c.bins[r, 1]) == float(c.bins[r, 0]) and float(c.bins[r, -1]) == float(c.bins[r, -2])
    if Nf == 0:
        return
    assert bool(((c.u_eff >= 0) & (c.u_eff <= 1)).all())
    loose = c.ref.loose & ~c.planted
    for reg, name in enumerate(SB.REGIMES):
        rows = c.regime == reg
        if name in ("A", "C"):
            assert int(loose[rows].sum()) == 0, (name, int(loose[rows].sum()))
        else:
            share = float(loose[rows].double().mean())
            assert share <= 0.02, share
    # planted draws: regime C, explicit draws, inside bins of both kinds, 40 U or more from the knots
    in_c = c.regime == 1
    assert not bool(c.planted[~in_c].any())
    if explicit and Nb >= 4:
        rows = in_c.clone()
        rows[[s[1] for s in (SB.special_rows(c, x) for x in (SB.ROW_ZERO, SB.ROW_ONEHOT, SB.ROW_NAN)) if len(s) > 1]] = False
        pl = c.planted[rows]
        assert bool(pl.any(-1).all())
        k, u = c.ref.k[rows], c.u_eff[rows].double()
        cl, ch = c.ref.c[rows].gather(-1, k), c.ref.c[rows].gather(-1, k + 1)
        assert bool((torch.minimum(u - cl, ch - u)[pl] >= 40 * SB.U).all())
        thr_hit = (c.ref.thr[rows].gather(-1, k) & pl).any(-1)
        assert bool(thr_hit.all())
        if Nb >= 5 and Nf >= 2:
            m = c.ref.m[rows].gather(-1, k)
            assert bool((((m > 2e-5) & (m < 4e-5)) & pl).any(-1).all())


@pytest.mark.parametrize("explicit", [False, True], ids=["linspace", "explicit"])
@pytest.mark.parametrize("case", DRAWN, ids=_ids)
def test_oracle_accepted_and_mutants_rejected(case, explicit):
    R, Nb, Nf, coarse = case
    c = SB.make_case(R, Nb, Nf, explicit, coarse)
    got = SB.oracle(c)
    assert torch.equal(got.isnan(), SB.oracle32(c.bins, c.w, c.u_eff).isnan())
    assert torch.equal(got.nan_to_num(0.0), SB.oracle32(c.bins, c.w, c.u_eff).nan_to_num(0.0))     # the mutants' base is the oracle
    rej, worst = SB.compare(got, c.ref, c.planted)
    assert rej.shape[0] == 0, SB.describe(rej, got, c.ref, c.u_eff)
    _worst[case + (explicit,)] = worst
    print(f"\noracle fp32 {_ids(case)} {'explicit' if explicit else 'linspace'}: worst |err| / e = {worst:.3f}  "
          f"(so far {max(_worst.values()):.3f})")
    for name, (fn, regimes, applies) in SB.MUTANTS.items():
        if not applies(c):
            continue
        rej, _ = SB.compare(fn(c), c.ref, c.planted)
        hit = set(c.regime[rej[:, 0]].tolist())
        for reg in regimes:
            assert "ACD".index(reg) in hit, (name, reg, rej.shape[0])
    # the copied draw is rejected as exactly that entry
    if Nf >= 2:
        rej, _ = SB.compare(SB.MUTANTS["one_draw_copied"][0](c), c.ref, c.planted)
        assert sorted(map(tuple, rej.tolist())) == sorted(SB.copied_draw(c))


def test_comparator_rejects_a_misplaced_nan_and_an_escaped_loose_draw():
    c = SB.make_case(SB.R_CASE, 64, 63, False)
    good = SB.oracle(c)
    nan_row = SB.special_rows(c, SB.ROW_NAN)[0]
    g = good.clone()
    g[nan_row, 5] = 3.0                                       # a number where the reference has NaN
    g[nan_row - 1, 7] = float("nan")                          # NaN where the reference has a number
    rej, _ = SB.compare(g, c.ref)
    assert sorted(map(tuple, rej.tolist())) == [(nan_row - 1, 7), (nan_row, 5)]
    loose = c.ref.loose.nonzero()
    assert loose.shape[0] > 0                                 # (regime D)
    r, s = (int(x) for x in loose[0])
    g = good.clone()
    g[r, s] = float(c.ref.hi[r, s]) + 1e-3
    rej, _ = SB.compare(g, c.ref)
    assert rej.tolist() == [[r, s]]
