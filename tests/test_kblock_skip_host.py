"""Host side of the K-block-skipping render kernel (no GPU needed): the pack-time unit order is an exact permutation, computed
once per pack; csrc/ns_ob16_kbskip_asm.inc is what the build has tools/gen_ob16_asm.py --kbskip emit; every mask path of every
statement passes the generator's checker and keeps the statement's barriers, vmcnt waits, DMA pieces, LDS reads and lgkmcnt waits;
and a fault that only a skip path shows is rejected."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_field as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "gen_ob16_asm.py")
INC = os.path.join(ROOT, "nerf_sampling_amd", "csrc", "ns_ob16_kbskip_asm.inc")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_ob16_asm_kbs", GEN)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- the unit order -------------------------------------------------------------------------------------------------
def _module(net):
    from nerf_sampling_amd.run_nerf_helpers import NeRF

    m = NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    mods = list(m.pts_linears) + [m.feature_linear, m.alpha_linear, m.views_linears[0], m.rgb_linear]
    with torch.no_grad():
        for mod, w, b in zip(mods, net["weights"], net["biases"]):
            mod.weight.copy_(torch.from_numpy(w))
            mod.bias.copy_(torch.from_numpy(b))
    return m


def test_the_unit_order_is_an_exact_deterministic_permutation():
    """on an exactly representable network the permuted tensors give the float64 chain's values, value for value"""
    from nerf_sampling_amd import run_nerf_helpers as H

    net = E.network("prod")
    m = _module(net)
    counts = H.firing_counts(m)
    orders = H.unit_orders(counts)
    assert all(torch.equal(a, b) for a, b in zip(orders, H.unit_orders(H.firing_counts(m))))
    for c, o in zip(counts, orders):
        assert sorted(o.tolist()) == list(range(256))
        s = c[o]
        assert bool((s[:-1] >= s[1:]).all())                               # descending firing count ...
        same = s[:-1] == s[1:]
        assert bool((o[:-1][same] < o[1:][same]).all())                     # ... ties by index
    assert any(not torch.equal(o, torch.arange(256)) for o in orders)
    ws, bs = H.permute_units([torch.from_numpy(w) for w in net["weights"]], [torch.from_numpy(b) for b in net["biases"]], orders, (4,))
    moved = dict(net, weights=[w.numpy() for w in ws], biases=[b.numpy() for b in bs])
    assert np.array_equal(E.chain(moved, net["pool"]), net["raw"])
    assert np.array_equal(E.folded_chain(moved, net["pool"]), E.folded_chain(net, net["pool"]))
    # the hidden activations are the original ones in the new order
    _, seen = E.chain(net, net["pool"][:64], keep=True)
    _, seen2 = E.chain(moved, net["pool"][:64], keep=True)
    for i in range(8):
        assert np.array_equal(seen2[f"pts{i}"][1], seen[f"pts{i}"][1][:, orders[i].numpy()])


def test_packed_orders_production_16_bit_handles_only_and_repack_recomputes(monkeypatch):
    from nerf_sampling_amd import ops
    from nerf_sampling_amd import run_nerf_helpers as H

    seen = []
    monkeypatch.setattr(ops, "pack_nerf", lambda ws, bs, *a, **k: seen.append([w.detach().clone() for w in ws]) or object())
    monkeypatch.delenv("NS_NO_UNIT_ORDER", raising=False)
    m = _module(E.network("prod"))
    m.packed("bf16")
    first = m.unit_orders
    assert first is not None and not torch.equal(seen[-1][3], m.pts_linears[3].weight)
    assert torch.equal(seen[-1][3], m.pts_linears[3].weight[first[3]][:, first[2]])
    for name in ("f16x3", "f32"):                                           # split and fp32 handles keep the trained order
        m.packed(name)
        assert m.unit_orders is None and torch.equal(seen[-1][3], m.pts_linears[3].weight)
    with torch.no_grad():                                                   # unit 7 of layer 3 now never fires: it moves to the end
        m.pts_linears[3].weight[7] = 0.0
        m.pts_linears[3].bias[7] = -1.0
    m.repack()
    m.packed("bf16")
    assert int(m.unit_orders[3][-1]) == 7 and int(first[3][-1]) != 7
    m.repack()
    m.unit_order = False                                                    # the switch
    m.packed("f16")
    assert m.unit_orders is None and torch.equal(seen[-1][3], m.pts_linears[3].weight)
    m.repack()
    m.unit_order = True
    monkeypatch.setenv("NS_NO_UNIT_ORDER", "1")
    m.packed("f16")
    assert m.unit_orders is None
    small = H.NeRF(D=4, W=128, input_ch=63, input_ch_views=27, output_ch=5, skips=[2], use_viewdirs=True)   # a generic shape
    monkeypatch.delenv("NS_NO_UNIT_ORDER")
    small.packed("bf16")
    assert small.unit_orders is None


# ---- the generator --------------------------------------------------------------------------------------------------
def test_the_statements_file_is_generated_by_the_build_and_deterministic(tmp_path):
    """csrc/ns_ob16_kbskip_asm.inc is not committed: the Makefile writes it with the generator, which gives the same text every
    time (and the file of a finished build is that text)"""
    outs = []
    for name in ("k1.inc", "k2.inc"):
        out = tmp_path / name
        subprocess.run([sys.executable, GEN, "--kbskip", "-o", str(out)], check=True, capture_output=True)
        outs.append(out.read_text())
    assert outs[0] == outs[1] and "struct KbsAsm<Mma16BF16, 5>" in outs[0] and "struct KbsAsm<Mma16F16, 0>" in outs[0]
    mk = open(os.path.join(os.path.dirname(INC), "Makefile")).read()
    assert "ns_ob16_kbskip_asm.inc: ../../tools/gen_ob16_asm.py" in mk and "--kbskip -o $@" in mk
    if os.path.exists(INC):
        assert open(INC).read() == outs[0], "stale build: make -C nerf_sampling_amd/csrc"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kid", range(6))
def test_every_mask_path_passes_the_checker_and_keeps_the_protocol(gen, dt, kid):
    prog = gen.gen_kbs(dt, kid)
    kind, kw = gen.KBS_KINDS[kid]
    consumer = kid > 0
    assert len(prog.bits) == (len(gen.KBS_TESTED) if consumer else 0) and len(list(prog.masks())) == (16 if consumer else 1)
    n = gen.kbs_verify(prog)                    # check() on every linearised path; the non-MFMA sequence is path-independent
    full = prog.linearise(max(prog.masks()))
    none = prog.linearise(0)
    nsb = {"hidden": 16, "sigma": 1, "colour": 8}[kind]
    steps = nsb * len(gen.KBS_TESTED) if consumer else 0
    assert sum(s[0] == "s" for s in prog.segs) == steps
    mf = lambda seq: sum(i.kind == "mfma" for i in seq)   # noqa: E731
    assert mf(full) - mf(none) == 5 * steps
    for text in ("s_barrier", "s_waitcnt vmcnt", "global_load_lds", "ds_read_b128", "s_waitcnt lgkmcnt"):
        assert sum(text in i.text for i in full) == sum(text in i.text for i in none) > 0, text
    assert sum("s_barrier" in i.text for i in full) == prog.slabs and sum(i.kind == "dma" for i in full) == 4 * prog.slabs
    assert n == len([i for i in none if i.kind not in ("mfma", "nop")]) - 3 * steps      # less test, branch and jump of each twin
    if kind == "hidden":                        # a producer: every dword of a tested output K-block ORed once, one compare per block
        ors = [i for i in full if i.text.startswith(("v_or_b32", "v_or3_b32"))]
        acc = gen.regs_of(gen.KBS_ACC)
        assert all(i.writes == acc for i in ors) and sum(len(i.reads - acc) for i in ors) == 20 * len(gen.KBS_TESTED)
        assert len(ors) <= 12 * len(gen.KBS_TESTED)
        assert sum(i.text.startswith("v_cmp_ne_u32") for i in full) == len(gen.KBS_TESTED)
        assert sum(i.text.startswith("s_addc_u32 %[omask]") for i in full) == len(gen.KBS_TESTED)
    # every K-block but the bias step's can be tested: 128 paths, still clean
    if kid == 1 and dt == "bf16":
        wide = gen.gen_kbs(dt, kid, tested=(1, 2, 3, 4, 5, 6, 7))
        assert len(list(wide.masks())) == 128
        gen.kbs_verify(wide)


def test_a_fault_that_only_a_skip_path_shows_is_rejected(gen):
    prog = gen.gen_kbs("bf16", 1)
    k = next(n for n, s in enumerate(prog.segs) if s[0] == "s")
    # (1) a conversion-like VALU read of the accumulator the LAST MFMA in front of a tested step wrote, at gap 2 of that step in both
    # arms: three MFMAs and their gaps away on the live path, a test, a branch and one gap instruction away when the step is skipped
    writer = [i for i in prog.segs[k - 1][1] if i.kind == "mfma"][-1]
    reg = sorted(writer.writes)[0]
    mk = lambda: gen.Ins(f"v_or_b32_e32 v64, v{reg[1]}, v64", "valu", reads=(gen.R(*reg),), writes=(gen.KBS_ACC,))   # noqa: E731
    saved = list(prog.segs)
    kind, bit, live, dead = prog.segs[k]
    at = [n for n, i in enumerate(live) if i.kind == "mfma"][3]
    fake_live, fake_dead = mk(), mk()
    prog.segs[k] = (kind, bit, live[:at] + [fake_live] + live[at:], dead[:1] + [fake_dead] + dead[1:])
    gen.check(prog.linearise(max(prog.masks())))            # the all-live text alone is clean
    with pytest.raises(AssertionError, match="MFMA D->valu|clock model"):
        gen.kbs_verify(prog)
    assert any(n > 0 for i, n in gen.kbs_deficits(prog.linearise(0)) if i is fake_dead)
    gen.kbs_repair(prog)                        # ... and the repair pads exactly that arm
    assert prog.pads.get(id(fake_dead), 0) > 0 and prog.pads.get(id(fake_live), 0) == 0
    gen.kbs_verify(prog)
    prog.pads.clear()                           # (2) the pad of the skip path dropped again
    with pytest.raises(AssertionError, match="MFMA D->valu|clock model"):
        gen.kbs_verify(prog)
    prog.segs[:] = saved
    # (3) a dead twin that loses its fragment read-ahead: the lgkmcnt counts of the path no longer hold
    kind, bit, live, dead = prog.segs[k]
    prog.segs[k] = (kind, bit, live, [i for i in dead if i.kind != "lds"])
    with pytest.raises(AssertionError):
        gen.kbs_verify(prog)
    prog.segs[:] = saved
    # (4) a dead twin without the slab's barrier (the skip layer: ten steps per sub-block, a slab starts at a tested step)
    prog = gen.gen_kbs("bf16", 2)
    kb = next(n for n, s in enumerate(prog.segs) if s[0] == "s" and any("s_barrier" in i.text for i in s[3]))
    kind, bit, live, dead = prog.segs[kb]
    prog.segs[kb] = (kind, bit, live, [i for i in dead if "s_barrier" not in i.text])
    with pytest.raises(AssertionError, match="drops or reorders"):
        gen.kbs_verify(prog)
