"""Inverse-CDF sampling (sample_pdf, importance_z) sample by sample against float64: the inputs, the reference, the error model
with its comparator, and float32 mutants of the oracle.

Shared by tests/test_gpu_sampling.py (the HIP kernels) and tests/test_sampling_bounds_host.py (on the CPU: the generators meet
their conditions, the fp32 oracle is accepted on every sample and every mutant below is rejected, so the bound is tight enough to
mean something).  Nothing here calls the library.

The reference, ref64(bins, w, u), in float64 on the fp32 inputs (nb bin edges b, nb - 1 weights w, draws u):
    v_j = fp32(w_j + 1e-5f) widened      S = sum_j v_j      p_j = v_j / S      c_0 = 0, c_k = sum_{j<k} p_j      m_k = c_{k+1} - c_k
    bin k is THRESHOLDED when m_k < 1e-5: den_k = 1, otherwise den_k = m_k
    k(u) = the last index with c_k <= u, clamped to nb - 2
    F(u) = b_k + (u - c_k) / den_k * (b_{k+1} - b_k),      F(u) = b_{nb-1} when u >= c_{nb-1}
    deterministic draws: torch.linspace(0, 1, Nf), widened.  A row with a NaN weight is NaN in every sample.

The error model.  U = 2^-24, slope_k = |b_{k+1} - b_k| / den_k:
    e(u) = C U max(slope_{k-1}, slope_k, slope_{k+1}) + 4 U |F(u)|
  The neighbouring slopes: a cdf off by a few U may put u into the next bin, and F is continuous across a knot unless a jump
  bin (below) touches it.  C = 24 is derived, not measured:
    - the kernels' normalising sum is a strided partial per lane plus a 6-step xor butterfly: at most 8 + 6 = 14 roundings on
      the path of any term for 511 terms, relative error |d| <= 14 U.  d scales the whole cdf, and because
      c_k + t m_k <= 1 that moves a sample by at most |d| slope;
    - the independent roundings -- one per division v_j / S (the cumulative sum itself runs in double), the conversion of each
      of the two knots to fp32, u - c, the quotient, the product -- add at most 7.5 U slope;
    - the final add and the rounding of the bin edges (z_mid = 0.5f * (z_k + z_{k+1}) rounds once) are the second term.
  (the wave kernel's double prefix scan is exact, whatever its order, while max v / min v < 2^28 in a row: the generators keep
  that, and the host test checks it.)

Jump bins and loose draws.  The inverse CDF jumps where a bin's mass crosses the reference's `denom < 1e-5` switch:
    bin k is a JUMP bin if it is thresholded or |m_k - 1e-5| <= 64 U;
    a draw is LOOSE if c_k - 64 U <= u <= c_{k+1} + 64 U for some jump bin k: it must lie in the hull of the edges of bins
    k - 1 .. k + 1 (over every such k), widened by e(u);
    every other draw is STRICT: |got - F(u)| <= e(u).
  NaN sits in the same entries as in the reference.  compare() returns the rejected entries; no share of them is forgiven.

Input regimes (make_case stacks a third of the rays from each; bin edges sorted in [2, 6], everything seeded):
    A  floor: w = rand^3 + 0.02, every mass far above the switch.
    C  small bins on both sides of the switch: the row sums to about 2; a quarter of the interior bins have w = 0 (mass about
       5e-6: thresholded), another eighth w = 5e-5 (mass about 3e-5: interpolated); never the first or the last bin.  With
       explicit draws the first columns of u are PLANTED at the midpoints of up to four bins of each kind per ray (42 U or more
       from their knots: they count as strict, and they are what catches a wrong threshold -- no random draw lands there).
       The zeroed bins are capped at max(4, 24576 / Nf) per ray: every one of them takes a 212 U stretch of [0, 1] away from the
       draws, and beyond that cap no redraw (next line) ends with all Nf draws clear of them.
       A and C hold NO loose draw: a ray whose draws (linspace counts) come within 64 U of a jump bin is redrawn, at most 8 times.
    D  compositing weights: alpha = rand^4 with half of them zero, w = alpha * T, interior slice.  Rows sum to about 1, so empty
       bins sit exactly at the switch, as the renderer's do (under linspace with Nf < 200, where the draws u = 0 and u = 1 are
       more than 1 % of a row, the first and the last bin hold at least 0.02).  A ray with more than 1 % of loose draws is redrawn
       (at most 8 times); the loose share of a case stays below 2 % (host test), and every strict draw is held to e(u).
    special rows in every regime: 1 all weights zero; 2 one-hot (0.5 in A and C, where the other bins then hold 2e-5 and
       interpolate; 1.0 in D, where they sit at the switch: that row is loose outside its hot bin and is not redrawn);
       3 duplicate edges at both ends (zero width); 5 one NaN weight (rows 4 and 6 around it are ordinary strict rows).

Mutants (fp32 variants of the oracle; the comparator rejects each in every regime named -- tests/test_sampling_bounds_host.py):
    no `+ 1e-5` (A, C, D); the normalising sum with one term counted twice (A, C, D; not under linspace with Nf <= 2, whose
    draws u = 0 and u = 1 give the first and the last edge whatever the sum); u = s / Nf instead of s / (Nf - 1)
    (deterministic draws; A, C, D); the threshold never taken, and a threshold of 1e-4 (C with planted draws); the last draw of
    every row equal to the one before it (A, C, D); one draw of one ray copied from its neighbour (A, C; the draw of that ray that differs most from
    its neighbour: the comparator rejects exactly that entry).
  searchsorted with right=False returns the same values (at u == c_k the two bins meet in the same point, or t = 0 against t = 1
  of a zero-mass step that cannot exist with v > 0), so it cannot be told apart and is no mutant.

Worst |err| / e over the strict draws, C = 24, at the cases below (CASES_PDF, CASES_IMPORTANCE; deterministic and explicit draws):
    the fp32 oracle on the CPU                                          0.53
    on the MI355X: sample_pdf_kernel on free edges                      0.25
                   importance_z, wave kernel NR = 1 / 2 / 4             0.21 / 0.22 / 0.23
                   importance_z, LDS kernel                             0.25
  (importance_z's figures are sample_pdf_kernel's on z_mid at that kernel's shapes: every importance_z kernel returned the
  sorted concatenation of exactly those samples, bit for bit.)  No kernel needed a rejected entry forgiven or a larger C.
"""

import functools
from types import SimpleNamespace

import torch

from oracle import nerf_oracle as O

U = 2.0 ** -24
C = 24.0
THR = 1e-5
BAND = 64 * U              # |m - 1e-5| of a jump bin, and the distance of a loose draw from a jump bin's knots
TINY = 2.0 ** -149

# ---- the cases of the GPU tests (the host test runs the same) ---------------------------------------------------------------
R_CASE = 3 * 133           # 133 rays of each regime: 399 = 4 * 99 + 3, a ragged last block of the four-rays-per-workgroup kernel
CASES_PDF = [(R_CASE, Nb, Nf) for Nb in (2, 3, 64, 65, 512) for Nf in (1, 2, 63, 64, 65, 300)] + [(8195, 3, 2)]
IMPORTANCE_KERNEL = {
    "wave1": [(3, 0), (3, 5), (8, 16), (32, 32), (64, 0), (8, 1)],
    "wave2": [(33, 32), (64, 64)],
    "wave4": [(64, 65), (64, 128), (64, 192)],
    "lds": [(64, 193), (65, 0), (65, 63), (100, 156), (129, 128), (300, 724), (513, 1535)],
}
CASES_IMPORTANCE = [(R_CASE, Nc, Nf) for v in IMPORTANCE_KERNEL.values() for Nc, Nf in v] + [(32773, 4, 4), (8195, 65, 3)]


def kernel_of(Nc, Nf):
    for name, cases in IMPORTANCE_KERNEL.items():
        if (Nc, Nf) in cases:
            return name
    return "wave1" if Nc + Nf <= 64 else "lds"


# ---- the reference and the model --------------------------------------------------------------------------------------------
def linspace_u(R, Nf):
    return torch.linspace(0.0, 1.0, Nf).expand(R, Nf).contiguous()


def ref64(bins, w, u):
    """bins [R, nb], w [R, nb - 1], u [R, Nf], all fp32.  Returns F (float64, NaN rows as NaN), the bound e, the loose mask with
    the hull of each loose draw, and the cdf pieces the generators and tests look at.  Bins monotone within a row (either way)."""
    assert bins.dtype == w.dtype == u.dtype == torch.float32
    R, nb = bins.shape
    b, uu = bins.double(), u.double().contiguous()
    v = (w + 1e-5).double()                                   # fp32(w + 1e-5f), widened
    S = v.sum(-1, keepdim=True)
    nan_row = ~torch.isfinite(S[:, 0])
    p = torch.where(nan_row[:, None], torch.full_like(v, 1.0 / (nb - 1)), v / S)   # (a placeholder cdf: searchsorted needs order)
    c = torch.cat([torch.zeros(R, 1, dtype=torch.float64), torch.cumsum(p, -1)], -1).contiguous()
    m = c[:, 1:] - c[:, :-1]
    thr = m < THR
    den = torch.where(thr, torch.ones_like(m), m)
    db = b[:, 1:] - b[:, :-1]
    slope = db.abs() / den
    k = (torch.searchsorted(c, uu, right=True) - 1).clamp(0, nb - 2)
    F = b.gather(-1, k) + (uu - c.gather(-1, k)) / den.gather(-1, k) * db.gather(-1, k)
    F = torch.where(uu >= c[:, -1:], b[:, -1:].expand_as(F), F)
    smax = torch.maximum(slope.gather(-1, k), torch.maximum(slope.gather(-1, (k - 1).clamp(min=0)),
                                                            slope.gather(-1, (k + 1).clamp(max=nb - 2))))
    e = C * U * smax + 4 * U * F.abs()
    # loose draws: some jump bin j with c_j - BAND <= u <= c_{j+1} + BAND, i.e. jl <= j <= jr
    jump = thr | ((m - THR).abs() <= BAND)
    jr = (torch.searchsorted(c, uu + BAND, right=True) - 1).clamp(0, nb - 2)
    jl = torch.searchsorted(c[:, 1:].contiguous(), uu - BAND, right=False).clamp(0, nb - 2)
    ar = torch.arange(nb - 1).expand(R, nb - 1)
    nxt = torch.where(jump, ar, torch.full_like(ar, nb)).flip(-1).cummin(-1).values.flip(-1)    # first jump bin at or after j
    prv = torch.where(jump, ar, torch.full_like(ar, -1)).cummax(-1).values                     # last jump bin at or before j
    jf, jt = nxt.gather(-1, jl), prv.gather(-1, jr)
    loose = (jf <= jr) & ~nan_row[:, None]
    ea, eb = b.gather(-1, (jf - 1).clamp(0, nb - 1)), b.gather(-1, (jt + 2).clamp(0, nb - 1))
    F = torch.where(nan_row[:, None], torch.full_like(F, float("nan")), F)
    return SimpleNamespace(F=F, e=e, loose=loose, lo=torch.minimum(ea, eb), hi=torch.maximum(ea, eb), c=c, m=m, thr=thr,
                           jump=jump, k=k, v=v, nan_row=nan_row)


def compare(got, ref, planted=None):
    """got [R, Nf] against ref64's result.  Returns (rejected, worst): the [n, 2] indices of every rejected entry and the
    largest |err| / e over the strict draws.  planted: draws that count as strict although they lie inside a jump bin."""
    g = got.detach().cpu().double()
    assert g.shape == ref.F.shape, (tuple(g.shape), tuple(ref.F.shape))
    nan_g, nan_f = torch.isnan(g), torch.isnan(ref.F)
    num = ~nan_g & ~nan_f
    loose = ref.loose if planted is None else ref.loose & ~planted
    err = (g - ref.F).abs()
    bad = (nan_g ^ nan_f) | (num & ~loose & ~(err <= ref.e)) | (num & loose & ~((g >= ref.lo - ref.e) & (g <= ref.hi + ref.e)))
    strict = num & ~loose
    worst = float((err[strict] / (ref.e[strict] + TINY)).max()) if bool(strict.any()) else 0.0
    return bad.nonzero(), worst


def describe(rej, got, ref, u):
    r, s = (int(x) for x in rej[0])
    return (f"{rej.shape[0]} rejected; row {r} draw {s}: u {float(u[r, s])!r} got {float(got[r, s])!r} F {float(ref.F[r, s])!r} "
            f"e {float(ref.e[r, s]):.3e} loose {bool(ref.loose[r, s])} hull [{float(ref.lo[r, s])!r}, {float(ref.hi[r, s])!r}] "
            f"bin {int(ref.k[r, s])} mass {float(ref.m[r, int(ref.k[r, s])]):.4e}")


# ---- the inputs -------------------------------------------------------------------------------------------------------------
REGIMES = ("A", "C", "D")
ROW_ZERO, ROW_ONEHOT, ROW_DUP, ROW_NAN = 1, 2, 3, 5
ONEHOT = {"A": 0.5, "C": 0.5, "D": 1.0}
MAX_REDRAWS = 8


def _rows(regime, n, Nb, Nf, explicit, coarse, g):
    """n ordinary rays of one regime: (edges or coarse depths, interior weights, u or None, planted)."""
    nbin = Nb - 1

    def rnd(*shape):
        return torch.rand(*shape, generator=g, dtype=torch.float64)

    pts = torch.sort(2.0 + 4.0 * rnd(n, Nb + 1 if coarse else Nb), -1).values.float()
    zero_idx = small_idx = None
    if regime == "A":
        w = rnd(n, nbin) ** 3 + 0.02
    elif regime == "C":
        w = rnd(n, nbin) ** 3 + 0.02
        ni = nbin - 2
        nz = min(max(1, ni // 4), max(4, 24576 // max(Nf, 1))) if ni >= 1 else 0
        ns = max(1, ni // 8) if ni >= 2 else 0
        special = torch.zeros(n, nbin, dtype=torch.bool)
        if ni >= 1:
            perm = torch.argsort(rnd(n, ni), -1) + 1
            zero_idx, small_idx = perm[:, :nz], perm[:, nz:nz + ns]
            special.scatter_(1, perm[:, :nz + ns], True)
        rest = torch.where(special, torch.zeros_like(w), w)
        w = rest * ((2.0 - ns * 5e-5) / rest.sum(-1, keepdim=True))
        if ni >= 1:
            w.scatter_(1, zero_idx, 0.0)
            w.scatter_(1, small_idx, 5e-5)
    else:
        alpha = rnd(n, nbin + 2) ** 4
        alpha[rnd(n, nbin + 2) < 0.5] = 0.0
        T = torch.cumprod(torch.cat([torch.ones(n, 1, dtype=torch.float64), 1.0 - alpha[:, :-1]], -1), -1)
        w = (alpha * T)[:, 1:-1]
        if not explicit and Nf < 200:                         # linspace always draws u = 0 and u = 1: 2 / Nf of the row
            w[:, 0], w[:, -1] = w[:, 0].clamp(min=0.02), w[:, -1].clamp(min=0.02)
    w = w.float()
    u, planted = None, torch.zeros(n, Nf, dtype=torch.bool)
    if explicit:
        u = rnd(n, Nf).float()
        if zero_idx is not None and Nf > 0:
            v = (w + 1e-5).double()
            c = torch.cat([torch.zeros(n, 1, dtype=torch.float64), torch.cumsum(v / v.sum(-1, keepdim=True), -1)], -1)
            cols = [x[:, i:i + 1] for i in range(4) for x in (zero_idx, small_idx) if i < x.shape[1]]   # the kinds alternate
            idx = torch.cat(cols, -1)[:, :Nf]
            mids = 0.5 * (c.gather(-1, idx) + c.gather(-1, idx + 1))
            u[:, :idx.shape[1]] = mids.float()
            planted[:, :idx.shape[1]] = True
    return pts, w, u, planted


def _mid(z):
    return 0.5 * (z[:, 1:] + z[:, :-1])                       # fp32, as the kernels form z_mid


def _block(regime, n, Nb, Nf, explicit, coarse, g):
    pts, w, u, planted = _rows(regime, n, Nb, Nf, explicit, coarse, g)
    fixed = torch.zeros(n, dtype=torch.bool)
    if n >= 8:
        w[ROW_ZERO] = 0.0
        w[ROW_ONEHOT] = 0.0
        w[ROW_ONEHOT, (Nb - 1) // 2] = ONEHOT[regime]
        fixed[ROW_ZERO] = fixed[ROW_ONEHOT] = True
        if explicit:                                          # (their planted columns belonged to the weights just replaced)
            redo = planted[[ROW_ZERO, ROW_ONEHOT]]
            u[[ROW_ZERO, ROW_ONEHOT]] = torch.where(redo, torch.rand(2, Nf, generator=g, dtype=torch.float64).float(),
                                                    u[[ROW_ZERO, ROW_ONEHOT]])
            planted[[ROW_ZERO, ROW_ONEHOT]] = False
    for _ in range(MAX_REDRAWS):
        if Nf == 0:
            break
        ref = ref64(_mid(pts) if coarse else pts, w, u if explicit else linspace_u(n, Nf))
        loose = ref.loose & ~planted
        bad = (loose.any(-1) if regime in ("A", "C") else loose.double().mean(-1) > 0.01) & ~fixed
        if not bool(bad.any()):
            break
        p2, w2, u2, pl2 = _rows(regime, int(bad.sum()), Nb, Nf, explicit, coarse, g)
        pts[bad], w[bad], planted[bad] = p2, w2, pl2
        if explicit:
            u[bad] = u2
    if n >= 8:
        if coarse and Nb >= 5:                                # three equal depths make two equal z_mid
            pts[ROW_DUP, :3] = pts[ROW_DUP, 0]
            pts[ROW_DUP, -3:] = pts[ROW_DUP, -1]
        elif coarse:
            pts[ROW_DUP] = pts[ROW_DUP, 0]
        elif Nb >= 3:
            pts[ROW_DUP, 1] = pts[ROW_DUP, 0]
            pts[ROW_DUP, -1] = pts[ROW_DUP, -2]
        w[ROW_NAN, (Nb - 1) // 2] = float("nan")
    return pts, w, u, planted


@functools.lru_cache(maxsize=8)
def make_case(R, Nb, Nf, explicit, coarse=False):
    """R rays, a third from each regime (A, C, D, in this order), Nb bin edges, Nf draws (explicit: random and planted u;
    otherwise u is None and the draws are linspace).  coarse: the edges are z_mid of Nb + 1 sorted coarse depths z, and w_full
    [R, Nb + 1] holds the weights in its interior slice, as importance_z takes them.  Treat the result as read-only."""
    g = torch.Generator().manual_seed(((R * 1009 + Nb) * 2053 + Nf) * 4 + 2 * int(explicit) + int(coarse))
    sizes = [R - 2 * (R // 3), R // 3, R // 3]
    parts = [_block(reg, n, Nb, Nf, explicit, coarse, g) for reg, n in zip(REGIMES, sizes)]
    pts, w = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    case = SimpleNamespace(R=R, Nb=Nb, Nf=Nf, explicit=explicit, w=w.contiguous(),
                           u=torch.cat([p[2] for p in parts]).contiguous() if explicit else None,
                           planted=torch.cat([p[3] for p in parts]),
                           regime=torch.repeat_interleave(torch.arange(3), torch.tensor(sizes)),
                           starts=[0, sizes[0], sizes[0] + sizes[1]], sizes=sizes)
    if coarse:
        case.z = pts.contiguous()
        case.bins = _mid(pts).contiguous()
        case.w_full = torch.cat([torch.rand(R, 1, generator=g), w, torch.rand(R, 1, generator=g)], -1).contiguous()
    else:
        case.bins = pts.contiguous()
    case.u_eff = case.u if explicit else linspace_u(R, Nf)
    case.ref = ref64(case.bins, case.w, case.u_eff)
    return case


def special_rows(case, which):
    """The row of one kind of special ray in each regime's block (blocks shorter than 8 rays have none)."""
    return [s + which for s, n in zip(case.starts, case.sizes) if n >= 8]


# ---- fp32 mutants of the oracle ---------------------------------------------------------------------------------------------
def oracle32(bins, w, u, floor=1e-5, twice=False, thr=1e-5):
    """oracle.nerf_oracle.sample_pdf in fp32 with its constants exposed (the defaults are the oracle, bit for bit)."""
    v = w + floor
    S = torch.sum(v, -1, keepdim=True)
    if twice:
        S = S + v[:, (v.shape[1] // 2):(v.shape[1] // 2) + 1]
    cdf = torch.cumsum(v / S, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    u = u.contiguous()
    idx = torch.searchsorted(cdf, u, right=True)
    lo, hi = torch.clamp(idx - 1, min=0), torch.clamp(idx, max=cdf.shape[-1] - 1)
    cdf_lo, cdf_hi = torch.gather(cdf, -1, lo), torch.gather(cdf, -1, hi)
    bin_lo, bin_hi = torch.gather(bins, -1, lo), torch.gather(bins, -1, hi)
    denom = cdf_hi - cdf_lo
    denom = torch.where(denom < thr, torch.ones_like(denom), denom)
    return bin_lo + (u - cdf_lo) / denom * (bin_hi - bin_lo)


def _last_twice(case):
    out = oracle32(case.bins, case.w, case.u_eff).clone()
    out[:, -1] = out[:, -2]
    return out


def copied_draw(case):
    """(row, draw) of the copied-draw mutant in regimes A and C: an ordinary ray, the draw whose reference value differs most
    from its left neighbour's (a copy between two draws of one flat bin is no error)."""
    rows = [s + min(7, n - 1) for s, n in zip(case.starts[:2], case.sizes[:2])]
    return [(r, 1 + int((case.ref.F[r, 1:] - case.ref.F[r, :-1]).abs().argmax())) for r in rows]


def _one_copied(case):
    out = oracle32(case.bins, case.w, case.u_eff).clone()
    for r, s in copied_draw(case):
        out[r, s] = out[r, s - 1]
    return out


def _u_over_nf(case):
    u = (torch.arange(case.Nf, dtype=torch.float32) / case.Nf).expand(case.R, case.Nf).contiguous()
    return oracle32(case.bins, case.w, u)


# name: (fp32 result of the mutant on a case, the regimes in which it must be rejected, whether the case can show it)
MUTANTS = {
    "no_floor": (lambda c: oracle32(c.bins, c.w, c.u_eff, floor=0.0), "ACD", lambda c: True),
    "sum_term_twice": (lambda c: oracle32(c.bins, c.w, c.u_eff, twice=True), "ACD", lambda c: c.explicit or c.Nf >= 3),
    "u_over_nf": (_u_over_nf, "ACD", lambda c: not c.explicit and c.Nf >= 2),
    "never_threshold": (lambda c: oracle32(c.bins, c.w, c.u_eff, thr=-1.0), "C", lambda c: c.explicit and c.Nb >= 4),
    "threshold_1e-4": (lambda c: oracle32(c.bins, c.w, c.u_eff, thr=1e-4), "C",
                       lambda c: c.explicit and c.Nb >= 5 and c.Nf >= 2),
    "last_draw_twice": (_last_twice, "ACD", lambda c: c.Nf >= 2),
    "one_draw_copied": (_one_copied, "AC", lambda c: c.Nf >= 2),
}


def oracle(case):
    return O.sample_pdf(case.bins, case.w, case.Nf, det=True, u=case.u)
