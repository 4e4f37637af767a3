"""The dead-suffix render kernel (nerf_ksuffix_ob16_kernel: the render kernel whose trunk layers 3..7 hand a live mask of their
tested output K-blocks on, and whose consumers pick, once per statement, the straight-line body that lacks the steps of the mask's
TRAILING dead K-blocks) against the render kernel on the SAME handle, in one process through ns_debug_set("kblock_suffix"), BIT
FOR BIT on every output -- and the counter of absent chunk steps against the number the planted networks predict, so that no
case passes with a body never taken.

The planted fields are those of test_gpu_kblock_skip.py (the "signed" field of test_gpu_colour_skip.py with every tested K-block
of every producing layer 3..7 `live`, `dead`, `zero` or `plane`; packed with unit_order = False so the blocks stay where they
are).  Five of them, NETS[k]: the output of trunk layer l is in state ROTA[(l - 3 + k) % 5], so across the five networks every
consumer (layers 4 / 6, the skip layer 5, layer 7, sigma, colour) sees every state:

  A  (live, live, plane, dead)    suffix 1 in the waves that hold a sample with x > 0, 2 in the others
  B  (live, plane, zero, dead)    suffix 2 / 3
  C  (plane, dead, dead, zero)    suffix 3 / 4
  D  (dead, zero, dead, dead)     suffix 4
  E  (live, dead, plane, live)    K-block 7 live, K-block 5 dead: not a suffix, the d = 0 body, the dead block is computed

A `plane` block sits just above the dead suffix: the rays alternate between the two sides of the plane x = 0, so the four waves
of ONE group take different bodies of the same statement.  Colour runs exactly in the waves that hold a sample with x > 0, where
A..D give the suffixes 1..4."""
import copy

import pytest
import torch

from test_gpu_colour_skip import EXTRAS, WAVE, _assert_same, _build_nets, _n_waves, _signed_rays

pytestmark = pytest.mark.gpu

TESTED = (4, 5, 6, 7)            # tools/gen_ob16_asm.py KBS_TESTED
ROTA = (("live", "live", "plane", "dead"), ("live", "plane", "zero", "dead"), ("plane", "dead", "dead", "zero"),
        ("dead", "zero", "dead", "dead"), ("live", "dead", "plane", "live"))
NETS = tuple({l: ROTA[(l - 3 + k) % 5] for l in range(3, 8)} for k in range(5))      # states of the output of trunk layer l
SUB_BLOCKS = {3: 16, 4: 16, 5: 16, 6: 16}            # sub-blocks of the statement that consumes layer l's output (7: 1 + 8)


@torch.no_grad()
def _planted(signed, states_of):
    m = copy.deepcopy(signed)
    m.unit_order = False
    for l, states in states_of.items():
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
    for k, states_of in enumerate(NETS):
        out[f"planted{k}"] = (_planted(out["signed"][0], states_of), out["signed"][1])
    return out


def _render(dw, nw, mode, *, n=64, rays=None, camera=None, extras=EXTRAS):
    """mode: "suffix" (the new kernel), "off" (the render kernel), "skip" (the K-block-skipping kernel, which wins over the new
    switch) or an integer value of the new switch; returns the outputs and the three counters"""
    from nerf_sampling_amd import ops

    sw = dict(prod_tiles=5, count_colour_skips=1)
    sw["kblock_suffix"] = {"suffix": 1, "off": 0, "skip": 1}.get(mode, mode)
    if mode == "skip":
        sw["kblock_skip"] = 1
    with ops.debug_switch(**sw):
        out = ops.render_rays_depthnet(dw, nw, rays=rays, camera=camera, n_samples=n, mode="uniform", std=0.1,
                                       white_bkgd=True, extras=extras, one_kernel=True)
        return out, ops.kblock_suffix_count(), ops.colour_skip_count(), ops.kblock_skip_count()


def _predicted_steps(pts, states_of):
    """chunk steps absent from the bodies the waves run: sum over statements of sub-blocks x trailing dead blocks of the wave's
    mask, from the sample positions the kernel formed (extras: pts [R, N, 3]); also the bodies taken, {(layer, d)}"""
    pos = (pts[..., 0] > 0).reshape(-1)
    S = pos.numel()
    idx = torch.arange(_n_waves(S) * WAVE, device=pos.device).clamp_(max=S - 1)
    P = pos[idx].reshape(-1, WAVE).any(1)                       # the wave holds a sample with x > 0
    total, taken = 0, set()
    for l, states in states_of.items():
        d = torch.zeros_like(P, dtype=torch.long)
        run = torch.ones_like(P)
        for state in reversed(states):                          # K-block 7 first
            dead = {"live": torch.zeros_like(P), "plane": ~P}.get(state, torch.ones_like(P))
            run = run & dead
            d += run.long()
        if l == 7:
            total += int(d.sum()) + 8 * int(d[P].sum())         # sigma always; colour only in the waves that run it
            taken |= {("sigma", int(x)) for x in d.unique()} | {("colour", int(x)) for x in d[P].unique()}
        else:
            total += SUB_BLOCKS[l] * int(d.sum())
            taken |= {(l + 1, int(x)) for x in d.unique()}
    return total, int((~P).sum()), taken, d, P


def _check(nets, k, dtype, empty, n=64, seed=0, against_skip=False):
    from nerf_sampling_amd import ops

    field, dn = nets[f"planted{k}"]
    dw, nw = dn.packed(ops.depthnet_dtype_for(dtype)), field.packed(dtype)
    assert field.unit_orders is None
    rays = _signed_rays(empty, seed)
    new, steps, waves_c, old_steps = _render(dw, nw, "suffix", n=n, rays=rays)
    old, steps_off, waves_c_off, _ = _render(dw, nw, "off", n=n, rays=rays)
    _assert_same(new, old, f"net {k} {dtype} {len(empty)} rays x {n}")
    want, want_c, taken, d7, P = _predicted_steps(new["pts"], NETS[k])
    print(f"net {k} {dtype} {len(empty)} x {n}: {steps} steps absent (predicted {want}), {waves_c} waves skip colour (predicted {want_c})")
    assert waves_c == waves_c_off == want_c                     # the colour skip decides the same on both sides
    assert steps == want
    assert steps > 0 and steps_off == 0 and old_steps == 0      # on: counted in its own slot; off: nothing
    if against_skip:                                            # "kblock_skip" = 1 wins over the new switch
        third, steps3, waves3, skip_steps = _render(dw, nw, "skip", n=n, rays=rays)
        _assert_same(new, third, f"net {k} {dtype} against the K-block-skipping kernel")
        assert steps3 == 0 and skip_steps >= want and waves3 == want_c
    return taken, d7, P


MIXED = {r: [i % 3 != 1 for i in range(r)] for r in (5, 7)}      # (True: the ray stays on the side x < 0) wave 2 is rays 2 and 3


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("rays", [5, 7])
def test_one_group_and_a_ragged_second_group(nets, dtype, rays):
    """5 rays x 64 samples are one group, all four waves; 7 rays are two groups, the second ragged.  Rays of both sides of the
    plane share the group, so its waves (80 samples) take different bodies.  Over the five networks every body of every consumer
    is taken, d = 0 by the non-suffix mask as well."""
    taken = set()
    for k in range(5):
        t, d7, P = _check(nets, k, dtype, MIXED[rays], against_skip=(k == 0))
        taken |= t
        if NETS[k][7] in ROTA[:3]:                              # a plane above the suffix: waves of the FIRST group differ in d
            assert len(set(d7[:4].tolist())) > 1, (k, d7[:4].tolist())
        if NETS[k][7] == ROTA[4]:                               # K-block 7 live, 5 dead
            assert set(d7.tolist()) == {0}
    for consumer in (4, 5, 6, 7, "sigma", "colour"):
        assert {(consumer, d) for d in range(5)} <= taken, (consumer, sorted(x for x in taken if x[0] == consumer))
    _check(nets, 1, dtype, [True] * rays, seed=1)               # every wave also takes the colour skip
    _check(nets, 2, dtype, [False] * rays, seed=2)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_every_workgroup_and_a_second_pass(nets, dtype):
    """5 x 256 + 3 rays: 257 groups -- every workgroup of a 256-CU device, a second pass for some; runs of four empty rays
    (whole groups take the colour skip) between runs of three mixed ones"""
    for k in (0, 3):
        _check(nets, k, dtype, [(i // 4) % 2 == 0 or i % 3 == 0 for i in range(5 * 256 + 3)])


@pytest.mark.parametrize("dtype,n", [("bf16", 32), ("f16", 2)])
def test_short_rays(nets, dtype, n):
    _check(nets, 1, dtype, [i % 2 == 0 for i in range(23)], n=n)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_nan_ray_inside_a_wave_with_a_dead_suffix(nets, dtype):
    """a ray with a NaN origin between rays of both sides: its samples come out NaN from both kernels, its neighbours' bits do not
    move, and the waves that hold it still leave out their dead suffixes"""
    from nerf_sampling_amd import ops

    field, dn = nets["planted2"]
    dw, nw = dn.packed(ops.depthnet_dtype_for(dtype)), field.packed(dtype)
    o, d, v = _signed_rays([i % 2 == 0 for i in range(9)], seed=3)
    o[4, 1] = float("nan")
    new, steps, waves_c, _ = _render(dw, nw, "suffix", rays=(o, d, v))
    old, steps_off, waves_c_off, _ = _render(dw, nw, "off", rays=(o, d, v))
    _assert_same(new, old, "NaN ray")
    assert torch.isnan(new["rgb"][4]).all() and torch.isfinite(new["rgb"][[0, 1, 2, 3, 5, 6, 7, 8]]).all()
    assert steps > 0 and steps_off == 0 and waves_c == waves_c_off


def test_a_handle_with_a_non_finite_weight_stays_on_the_render_kernel(nets):
    """inf * 0 is NaN: the packer keeps such a handle off the kernels that leave products out"""
    from nerf_sampling_amd import ops

    field, dn = nets["planted0"]
    m = copy.deepcopy(field)
    with torch.no_grad():
        m.pts_linears[6].weight[200, 17] = float("inf")
    m.repack()
    dw, nw = dn.packed(ops.depthnet_dtype_for("bf16")), m.packed("bf16")
    rays = _signed_rays([True, False, True, True, False])
    _, steps, _, _ = _render(dw, nw, "suffix", rays=rays)
    assert steps == 0


def _fit_rays():
    from nerf_sampling_amd import ops, synthetic

    H = W = 800
    _, K = synthetic.blender_intrinsics(H, W)
    c2w = synthetic.render_poses(40)[17, :3, :4]
    o, d, v = ops.get_rays(H, W, K, c2w)[:3]
    pick = torch.arange(20, device=o.device) * (H * W // 20) + W // 3
    return tuple(t.reshape(-1, 3)[pick].contiguous() for t in (o, d, v))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fitted_scene_leaves_steps_out_under_the_unit_order(nets, dtype):
    """20 rays of a bench pose on the fitted scene packed with the unit order: the counter is nonzero, and every output has the
    bits of the render kernel on the same handle"""
    from nerf_sampling_amd import ops

    field, dn = nets["fit"]
    assert field.unit_order
    dw, nw = dn.packed(ops.depthnet_dtype_for(dtype)), field.packed(dtype)
    assert field.unit_orders is not None
    rays = _fit_rays()
    new, steps, waves_c, _ = _render(dw, nw, "suffix", rays=rays)
    old, steps_off, waves_c_off, _ = _render(dw, nw, "off", rays=rays)
    _assert_same(new, old, "fitted scene")
    print(f"fitted scene {dtype}: {steps} chunk steps absent in {_n_waves(20 * 64)} waves of 1045 steps")
    assert steps > 0 and steps_off == 0 and waves_c == waves_c_off


def test_the_initial_value_takes_unit_ordered_handles(nets):
    """with the switch untouched (2, unless NS_KBLOCK_SUFFIX says otherwise) the bench's handle runs the new kernel"""
    import os

    from nerf_sampling_amd import ops

    field, dn = nets["fit"]
    dw, nw = dn.packed(ops.depthnet_dtype_for("bf16")), field.packed("bf16")
    with ops.debug_switch(prod_tiles=5, count_colour_skips=1):
        ops.render_rays_depthnet(dw, nw, rays=_fit_rays(), n_samples=64, mode="uniform", std=0.1, white_bkgd=True, one_kernel=True)
        steps = ops.kblock_suffix_count()
    assert (steps > 0) == (os.environ.get("NS_KBLOCK_SUFFIX", "2")[:1] in ("1", "2"))


def test_switch_value_2_takes_unit_ordered_handles_only(nets):
    """value 2: a handle NeRF.packed() sorted by firing rate runs the new kernel; the same field packed in its own order does not"""
    from nerf_sampling_amd import ops

    field, dn = nets["fit"]
    dw, nw = dn.packed(ops.depthnet_dtype_for("bf16")), field.packed("bf16")
    assert field.unit_orders is not None
    own = copy.deepcopy(field)
    own.unit_order = False
    nw_own = own.packed("bf16")
    assert own.unit_orders is None
    rays = _fit_rays()
    new, steps, _, _ = _render(dw, nw, 2, rays=rays)
    old, steps_off, _, _ = _render(dw, nw, "off", rays=rays)
    _assert_same(new, old, "fitted scene, value 2")
    assert steps > 0 and steps_off == 0
    _, steps_own, _, _ = _render(dw, nw_own, 2, rays=rays)
    assert steps_own == 0
