"""The K-block-skipping render kernel (nerf_kbskip_ob16_kernel: the render kernel whose trunk layers 3..7 hand a live mask of
their tested output K-blocks on, and whose consumers jump over the MFMAs of a chunk step whose input K-block is all zero bits for
the wave) against the render kernel on the SAME handle, in one process through ns_debug_set("kblock_skip"), BIT FOR BIT on
every output -- and the counter of skipped chunk steps against the number the planted network predicts, so that no case passes
with the path never taken.

The "planted" field is the "signed" field of test_gpu_colour_skip.py (trunk units 0 / 1 carry relu(x) / relu(-x) of the point's
first coordinate through all eight layers exactly, sigma = 30 x; everything else seeded lego_synth weights) with every TESTED
K-block (hidden units 128..255 in blocks of 32) of every producing layer 3..7 put in one of four states:

  live   unit 32 kb has a zero row and bias +1: positive for every sample, so the block is live in every wave
  dead   all 32 units have zero rows and bias -1: the ReLU leaves 0x0000 everywhere
  zero   all 32 units have zero rows and bias 0: the pre-activation is +0 exactly (the +-0 case of the header's argument)
  plane  unit 32 kb reads the carried relu(x) with weight 1, the other 31 are `zero`: live exactly in the waves that hold a sample
         with x > 0, i.e. the unit switches on across the plane x = 0, which cuts groups and waves of the rays below

The module is packed with its units in their own order (unit_order = False), so the planted blocks stay where they are.  A wave
of 80 consecutive samples (the tail's waves hold clamped copies of the last sample) then skips, per statement, sub-blocks x dead
tested blocks of the statement's input: 16 for a trunk layer, 1 for sigma, 8 for colour -- unless the wave skips colour altogether,
which it does exactly when no sample has x > 0.  Layer 5's output is dead in all four tested blocks (mask 0)."""
import copy

import pytest
import torch

from test_gpu_colour_skip import EXTRAS, GROUP, WAVE, _assert_same, _build_nets, _n_waves, _signed_rays

pytestmark = pytest.mark.gpu

TESTED = (4, 5, 6, 7)            # tools/gen_ob16_asm.py KBS_TESTED
STATES = {3: ("live", "dead", "plane", "zero"),      # output of trunk layer l: the state of K-blocks 4, 5, 6, 7
          4: ("dead", "live", "live", "plane"),      # feeds the skip layer
          5: ("dead", "dead", "zero", "dead"),       # a whole mask of zeros
          6: ("plane", "zero", "dead", "live"),
          7: ("live", "plane", "dead", "zero")}      # feeds sigma and colour
SUB_BLOCKS = {3: 16, 4: 16, 5: 16, 6: 16}            # sub-blocks of the statement that consumes layer l's output (7: 1 + 8)


@torch.no_grad()
def _planted(signed):
    m = copy.deepcopy(signed)
    m.unit_order = False
    for l, states in STATES.items():
        lin = m.pts_linears[l]
        c0 = 63 if l == 5 else 0                      # the layer behind the skip sees cat[x(63), h]
        for kb, state in zip(TESTED, states):
            u = 32 * kb
            if state == "live":
                lin.weight[u] = 0.0
                lin.bias[u] = 1.0
                continue
            lin.weight[u:u + 32] = 0.0
            lin.bias[u:u + 32] = -1.0 if state == "dead" else 0.0
            if state == "plane":
                lin.weight[u, c0] = 1.0
    m.repack()
    return m


@pytest.fixture(scope="module")
def nets():
    out = _build_nets()
    out["planted"] = (_planted(out["signed"][0]), out["signed"][1])
    return out


def _render(dw, nw, skip, *, n=64, rays=None, camera=None, extras=EXTRAS):
    from nerf_sampling_amd import ops

    sw = dict(prod_tiles=5, count_colour_skips=1, kblock_skip=int(skip))
    with ops.debug_switch(**sw):
        out = ops.render_rays_depthnet(dw, nw, rays=rays, camera=camera, n_samples=n, mode="uniform", std=0.1,
                                       white_bkgd=True, extras=extras, one_kernel=True)
        return out, ops.kblock_skip_count(), ops.colour_skip_count()


def _predicted_steps(pts):
    """chunk steps the planted field's waves skip, from the sample positions the kernel formed (extras: pts [R, N, 3])"""
    pos = (pts[..., 0] > 0).reshape(-1)
    S = pos.numel()
    idx = torch.arange(_n_waves(S) * WAVE, device=pos.device).clamp_(max=S - 1)
    P = pos[idx].reshape(-1, WAVE).any(1)                       # the wave holds a sample with x > 0
    total = 0
    for l, states in STATES.items():
        fixed = sum(s in ("dead", "zero") for s in states)
        planes = sum(s == "plane" for s in states)
        dead = fixed + planes * (~P).long()                     # per wave
        if l == 7:
            total += int(dead.sum()) + 8 * int(dead[P].sum())   # sigma always; colour only in the waves that run it
        else:
            total += SUB_BLOCKS[l] * int(dead.sum())
    return total, int((~P).sum())


def _check(nets, dtype, empty, n=64, seed=0):
    from nerf_sampling_amd import ops

    field, dn = nets["planted"]
    dw, nw = dn.packed(ops.depthnet_dtype_for(dtype)), field.packed(dtype)
    rays = _signed_rays(empty, seed)
    new, steps, waves_c = _render(dw, nw, True, n=n, rays=rays)
    old, steps_old, waves_c_old = _render(dw, nw, False, n=n, rays=rays)
    assert steps_old == 0
    _assert_same(new, old, f"{dtype} {len(empty)} rays x {n}")
    want, want_c = _predicted_steps(new["pts"])
    print(f"planted {dtype} {len(empty)} x {n}: {steps} steps skipped (predicted {want}), {waves_c} waves skip colour (predicted {want_c})")
    assert waves_c == waves_c_old == want_c
    assert steps == want and steps > 0
    return new


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("rays", [5, 7])
def test_one_group_and_a_ragged_second_group(nets, dtype, rays):
    """5 rays x 64 samples are one group, all four waves; 7 rays are two groups, the second ragged.  Rays alternate between the
    two sides of the plane, so waves (80 samples) straddle it and the plane blocks are dead in some waves only."""
    _check(nets, dtype, [i % 3 != 1 for i in range(rays)])
    _check(nets, dtype, [True] * rays, seed=1)          # every wave also takes the colour skip
    _check(nets, dtype, [False] * rays, seed=2)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_every_workgroup_and_a_second_pass(nets, dtype):
    """5 x 256 + 3 rays: 257 groups -- every workgroup of a 256-CU device, a second pass for some; runs of four empty rays
    (whole groups take the colour skip) between runs of three mixed ones"""
    _check(nets, dtype, [(i // 4) % 2 == 0 or i % 3 == 0 for i in range(5 * 256 + 3)])


@pytest.mark.parametrize("dtype,n", [("bf16", 32), ("f16", 2)])
def test_short_rays(nets, dtype, n):
    _check(nets, dtype, [i % 2 == 0 for i in range(23)], n=n)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_nan_ray_inside_a_wave_with_dead_blocks(nets, dtype):
    """a ray with a NaN origin between rays of both sides: its samples come out NaN from both kernels, its neighbours' bits do not
    move, and the waves that hold it still skip their dead blocks"""
    from nerf_sampling_amd import ops

    field, dn = nets["planted"]
    dw, nw = dn.packed(ops.depthnet_dtype_for(dtype)), field.packed(dtype)
    o, d, v = _signed_rays([i % 2 == 0 for i in range(9)], seed=3)
    o[4, 1] = float("nan")
    new, steps, _ = _render(dw, nw, True, rays=(o, d, v))
    old, steps_old, _ = _render(dw, nw, False, rays=(o, d, v))
    _assert_same(new, old, "NaN ray")
    assert torch.isnan(new["rgb"][4]).all() and torch.isfinite(new["rgb"][[0, 1, 2, 3, 5, 6, 7, 8]]).all()
    assert steps > 0 and steps_old == 0


def test_a_handle_with_a_non_finite_weight_stays_on_the_render_kernel(nets):
    """inf * 0 is NaN: the packer keeps such a handle off the K-block-skipping kernel"""
    from nerf_sampling_amd import ops

    field, dn = nets["planted"]
    m = copy.deepcopy(field)
    with torch.no_grad():
        m.pts_linears[6].weight[200, 17] = float("inf")
    m.repack()
    dw, nw = dn.packed(ops.depthnet_dtype_for("bf16")), m.packed("bf16")
    rays = _signed_rays([True, False, True, True, False])
    _, steps, _ = _render(dw, nw, True, rays=rays)
    assert steps == 0


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fitted_scene_skips_steps_under_the_unit_order(nets, dtype):
    """20 rays of a bench pose on the fitted scene packed with the unit order: the counter is nonzero, and every output has the
    bits of the render kernel on the same handle"""
    from nerf_sampling_amd import ops, synthetic

    field, dn = nets["fit"]
    assert field.unit_order
    dw, nw = dn.packed(ops.depthnet_dtype_for(dtype)), field.packed(dtype)
    assert field.unit_orders is not None
    H = W = 800
    _, K = synthetic.blender_intrinsics(H, W)
    c2w = synthetic.render_poses(40)[17, :3, :4]
    o, d, v = ops.get_rays(H, W, K, c2w)[:3]
    pick = torch.arange(20, device=o.device) * (H * W // 20) + W // 3
    rays = tuple(t.reshape(-1, 3)[pick].contiguous() for t in (o, d, v))
    new, steps, _ = _render(dw, nw, True, rays=rays)
    old, steps_old, _ = _render(dw, nw, False, rays=rays)
    _assert_same(new, old, "fitted scene")
    print(f"fitted scene {dtype}: {steps} chunk steps skipped in {_n_waves(20 * 64)} waves of 1045 steps")
    assert steps > 0 and steps_old == 0
