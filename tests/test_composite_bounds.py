"""The float64 comparator of tests/composite_bounds.py can fail (not gpu): the oracle's compositing in float32 passes it at
every sample count of the sweep, and each float32 mutant of it -- one plausible kernel slip apiece -- is rejected at one or
more of them.  A bound loose enough to let a mutant through would let the same slip in a HIP kernel through."""

import pytest
import torch

import composite_bounds as CB
from oracle import nerf_oracle as O

MUTANTS = ("inclusive_transmittance", "no_1e-10", "no_ray_norm", "last_dist_is_a_gap", "noise_after_relu",
           "white_without_1_minus_acc")


def composite32(raw, z, rays_d, noise, white, mutant=None):
    """oracle.raw2outputs in float32 with one slip switched on; the six outputs the kernel returns."""
    R, N = z.shape
    dists = z[..., 1:] - z[..., :-1]
    last = dists[..., -1:] if (mutant == "last_dist_is_a_gap" and N > 1) else torch.tensor([1e10]).expand(dists[..., :1].shape)
    dists = torch.cat([dists, last], -1)
    if mutant != "no_ray_norm":
        dists = dists * torch.norm(rays_d[..., None, :], dim=-1)
    rgb = torch.sigmoid(raw[..., :3])
    add = noise if noise is not None else 0.0
    if mutant == "noise_after_relu":
        alphas = 1.0 - torch.exp(-(torch.relu(raw[..., 3]) + add) * dists)
    else:
        alphas = 1.0 - torch.exp(-torch.relu(raw[..., 3] + add) * dists)
    keep = 1.0 - alphas + (0.0 if mutant == "no_1e-10" else 1e-10)
    trans = torch.cumprod(torch.cat([torch.ones((R, 1)), keep], -1), -1)
    trans = trans[:, 1:] if mutant == "inclusive_transmittance" else trans[:, :-1]
    weights = alphas * trans
    rgb_map = torch.sum(weights[..., None] * rgb, -2)
    depth_map = torch.sum(weights * z, -1)
    acc_map = torch.sum(weights, -1)
    disp_map = 1.0 / torch.max(1e-10 * torch.ones_like(depth_map), depth_map / (acc_map + 1e-10))
    if white:
        rgb_map = rgb_map + (1.0 if mutant == "white_without_1_minus_acc" else (1.0 - acc_map[..., None]))
    if N == 1:
        rgb_map = torch.sum(rgb, -2)
        alphas, weights = alphas[:, :0], weights[:, :0]
    return rgb_map, disp_map, acc_map, depth_map, alphas, weights


def _cases(sweep):
    for N in sweep:
        for white in (False, True):
            for with_noise in (False, True):
                yield N, white, with_noise


def test_unmutated_float32_compositing_passes_the_float64_comparator():
    """The copy above without a mutant is the oracle's float32 arithmetic (bit for bit: checked here), and it stays inside every
    bound at every N of the sweep -- the model allows a correct fp32 implementation."""
    worst = {}
    for N, white, with_noise in _cases(CB.SWEEP):
        raw, z, d, noise = CB.make_inputs(CB.rays_for(N), N, seed=N, with_noise=with_noise)
        got = composite32(raw, z, d, noise, white)
        if N in (2, 64, 129):
            exp = O.raw2outputs(raw, z, d, 1.0 if noise is not None else 0.0, white, noise=noise)
            for a, b in zip(got[:4], exp[:4]):
                torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
        for k, (ratio, _) in CB.check(got, raw, z, d, noise, white).items():
            worst[k] = max(worst.get(k, 0.0), ratio)
    print("float32 oracle, worst |err| / bound:", {k: f"{v:.3f}" for k, v in worst.items()})


# a small sweep per mutant: one N of every layout, and multi-chunk rays with a partial last chunk
MUTANT_SWEEP = [1, 2, 3, 8, 9, 16, 17, 33, 64, 65, 130, 320]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_is_rejected(mutant):
    rejected = []
    for N, white, with_noise in _cases(MUTANT_SWEEP):
        raw, z, d, noise = CB.make_inputs(CB.rays_for(N), N, seed=N, with_noise=with_noise)
        got = composite32(raw, z, d, noise, white, mutant)
        try:
            CB.check(got, raw, z, d, noise, white)
        except AssertionError as e:
            rejected.append((N, white, with_noise, str(e).split(":")[0]))
    print(f"mutant {mutant}: rejected at {len(rejected)} of {4 * len(MUTANT_SWEEP)} cases, e.g. {rejected[:3]}")
    assert rejected, mutant
