"""Host side of the dead-suffix render kernel (no GPU needed): csrc/ns_ob16_ksuffix_asm.inc is what the build has
tools/gen_ob16_asm.py --ksuffix emit; every body of every consumer statement passes the generator's checker, keeps body 0's
barriers, vmcnt and lgkmcnt waits, DMA pieces, LDS reads, conversions, ORs and mask instructions text for text, and lacks exactly
the MFMAs of its dead suffix; the scalar dispatch in front of the bodies sends every mask to the body of its trailing zeros; and
a fault that only a shortened body shows is rejected."""
import importlib.util
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "gen_ob16_asm.py")
INC = os.path.join(ROOT, "nerf_sampling_amd", "csrc", "ns_ob16_ksuffix_asm.inc")

CONSUMERS = (1, 2, 3, 4, 5)                   # KBS_KINDS: trunk layers 4 / 6, 5 and 7, sigma, colour
SUB_BLOCKS = {1: 16, 2: 16, 3: 16, 4: 1, 5: 8}
K_BLOCKS = {1: 8, 2: 10, 3: 8, 4: 9, 5: 9}    # chunk steps of a sub-block: the skip layer's embedded point, the view direction


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_ob16_asm_ksx", GEN)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def progs(gen):
    """(dtype, kind) -> (program, bodies), generated once for the module"""
    out = {}
    for dt in ("bf16", "f16"):
        for kid in range(len(gen.KBS_KINDS)):
            prog = gen.gen_kbs(dt, kid)
            out[dt, kid] = (prog, gen.ksx_bodies(prog))
    return out


def _protocol(seq):
    return [i.text for i in seq if i.kind not in ("mfma", "nop")]


def test_the_statements_file_is_generated_by_the_build_and_deterministic(tmp_path):
    outs = []
    for name in ("k1.inc", "k2.inc"):
        out = tmp_path / name
        subprocess.run([sys.executable, GEN, "--ksuffix", "-o", str(out)], check=True, capture_output=True)
        outs.append(out.read_text())
    assert outs[0] == outs[1] and "struct KsxAsm<Mma16BF16, 5>" in outs[0] and "struct KsxAsm<Mma16F16, 0>" in outs[0]
    assert "s_bitcmp1" not in outs[0]                       # no per-step test in any body
    mk = open(os.path.join(os.path.dirname(INC), "Makefile")).read()
    assert "ns_ob16_ksuffix_asm.inc: ../../tools/gen_ob16_asm.py" in mk and "--ksuffix -o $@" in mk
    assert "-DNS_OB16_TU_RENDER -DNS_OB16_TU_KSUFFIX" in mk and "ns_ob16_ksuffix_asm.inc" in mk.split("clean:")[1]
    assert "nerf_sampling_amd/csrc/ns_ob16_ksuffix_asm.inc" in open(os.path.join(ROOT, ".gitignore")).read().split()
    if os.path.exists(INC):
        assert open(INC).read() == outs[0], "stale build: make -C nerf_sampling_amd/csrc"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kid", CONSUMERS)
def test_every_body_passes_the_checker_keeps_the_protocol_and_lacks_its_suffix(gen, progs, dt, kid):
    prog, bodies = progs[dt, kid]
    nbits = len(gen.KBS_TESTED)
    assert len(bodies) == nbits + 1 == 5
    want = _protocol(bodies[0])
    control = ("s_bitcmp1", "s_cbranch", "s_branch")
    for d, body in enumerate(bodies):
        gen.check(body)
        assert not any(i.text.startswith(control) for i in body), d
        # barriers, vmcnt / lgkmcnt waits with their counts, DMA pieces with their operands, LDS reads, conversions, ORs, mask instructions
        assert _protocol(body) == want, d
        assert sum(i.kind == "mfma" for i in body) == 5 * SUB_BLOCKS[kid] * (K_BLOCKS[kid] - d), d
        # the MFMAs left out are those of the LAST d tested K-blocks: the body is the skip program's path of that mask
        path = [i for i in prog.linearise(gen.ksx_mask(d, nbits)) if i not in (prog.test, prog.cbr, prog.jmp)]
        strip = lambda seq: [i.text for i in seq if i.kind != "nop"]   # noqa: E731
        assert strip(body) == strip(path), d
    assert sum("s_barrier" in t for t in want) == prog.slabs and sum(t.startswith("global_load_lds") for t in want) == 4 * prog.slabs
    assert gen.ksx_verify(prog, bodies) == len(want)
    if gen.KBS_KINDS[kid][0] == "hidden":                   # every body is a producer of its output's mask
        assert sum(t.startswith("s_addc_u32 %[omask]") for t in want) == nbits
        assert sum(t.startswith(("v_or_b32", "v_or3_b32")) for t in want) > 0
    # the d = 0 body is the all-live path: nothing of the statement is missing
    assert [i.text for i in bodies[0] if i.kind == "mfma"] == [i.text for i in prog.linearise(max(prog.masks())) if i.kind == "mfma"]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_layer_3_is_a_producer_with_one_body(gen, progs, dt):
    prog, bodies = progs[dt, 0]
    assert len(bodies) == 1 and not prog.bits
    text = gen.ksx_text(bodies, 0)
    assert text == [i.text for i in bodies[0]] and not any("kd" in t or t.startswith(".L") for t in text)
    assert sum(i.kind == "mfma" for i in bodies[0]) == 5 * 16 * 8


def _run_dispatch(lines, kmask):
    """interprets the scalar dispatch: returns the label branched to, or None when it falls through"""
    reg, scc = {"%[kmask]": kmask}, 0
    val = lambda t: reg[t] if t in reg else int(t, 0)   # noqa: E731
    for line in lines:
        op, args = line.split(None, 1)
        args = [a.strip() for a in args.split(",")]
        if op == "s_or_b32":
            reg[args[0]] = val(args[1]) | val(args[2])
        elif op == "s_ff1_i32_b32":
            v = val(args[1])
            assert v != 0
            reg[args[0]] = (v & -v).bit_length() - 1
        elif op == "s_cmp_eq_u32":
            scc = int(val(args[0]) == val(args[1]))
        elif op == "s_cbranch_scc1":
            if scc:
                return args[0]
        else:
            raise AssertionError(f"unexpected instruction in the dispatch: {line}")
    return None


@pytest.mark.parametrize("kid", CONSUMERS)
def test_the_dispatch_sends_every_mask_to_the_body_of_its_trailing_zeros(gen, progs, kid):
    prog, bodies = progs["bf16", kid]
    nbits = len(gen.KBS_TESTED)
    text = gen.ksx_text(bodies, nbits)
    head = gen.ksx_dispatch(nbits)
    assert text[:len(head)] == head
    # the text behind the dispatch: body 0, then label d and body d for d = 1 .. 4, each body but the last ending in a jump to the join
    at, where = len(head), {}
    for d, body in enumerate(bodies):
        if d:
            m = re.fullmatch(r"(\.Lksd%=_(\d+)):", text[at])
            assert m and int(m.group(2)) == d
            where[m.group(1)] = d
            at += 1
        assert text[at:at + len(body)] == [i.text for i in body]
        at += len(body)
        if d + 1 < len(bodies):
            assert text[at] == "s_branch .Lksj%="
            at += 1
    assert text[at:] == [".Lksj%=:"]
    for mask in range(1 << nbits):
        tz = next((b for b in range(nbits) if (mask >> b) & 1), nbits)
        label = _run_dispatch(head, mask)
        assert (0 if label is None else where[label]) == tz, mask
        # the body taken never leaves out a live block: its dead suffix is dead in the mask
        assert mask & ((1 << tz) - 1) == 0
    assert _run_dispatch(head, (1 << nbits) - 1) is None     # all live: falls through into body 0
    assert gen.ksx_mask(0, nbits) == (1 << nbits) - 1 and gen.ksx_mask(nbits, nbits) == 0
    assert _run_dispatch(head, 0b1010) == ".Lksd%=_1" and _run_dispatch(head, 0b0101) is None   # not pure suffixes: trailing zeros only


def test_planted_faults_are_rejected(gen):
    prog = gen.gen_kbs("bf16", 1)
    nbits = len(prog.bits)
    k = next(n for n, s in enumerate(prog.segs) if s[0] == "s" and sum(i.kind != "mfma" for i in s[2]) >= 5)   # a step with full gaps
    # (1) a conversion-like VALU read of the accumulator the LAST MFMA in front of a removed step wrote, one gap into that step: on
    # the all-live body four MFMAs and their gaps lie between the two, in a body without the step one gap instruction does
    writer = [i for i in prog.segs[k - 1][1] if i.kind == "mfma"][-1]
    reg = sorted(writer.writes)[0]
    mk = lambda: gen.Ins(f"v_or_b32_e32 v64, v{reg[1]}, v64", "valu", reads=(gen.R(*reg),), writes=(gen.KBS_ACC,))   # noqa: E731
    saved = list(prog.segs)
    kind, bit, live, dead = prog.segs[k]
    at = [n for n, i in enumerate(live) if i.kind == "mfma"][4]
    fake_live, fake_dead = mk(), mk()
    prog.segs[k] = (kind, bit, live[:at] + [fake_live] + live[at:], dead[:1] + [fake_dead] + dead[1:])
    d = bit + 1                                 # the shortest suffix that removes this step
    mask = gen.ksx_mask(d, nbits)
    raw = [i for i in prog.linearise(mask) if i not in (prog.test, prog.cbr, prog.jmp)]
    gen.check([i for i in prog.linearise(gen.ksx_mask(0, nbits)) if i not in (prog.test, prog.cbr, prog.jmp)])   # clean where the step stays
    with pytest.raises(AssertionError, match="MFMA D->valu|clock model"):
        gen.check(raw)
    body = gen.ksx_body(prog, d)                # ... and the body is padded in front of exactly that instruction
    n = body.index(fake_dead)
    assert body[n - 1].kind == "nop"
    gen.check(body)
    with pytest.raises(AssertionError, match="MFMA D->valu|clock model"):
        gen.check([i for j, i in enumerate(body) if j != n - 1])
    prog.segs[:] = saved
    # (2) a body that drops a slab's barrier (the skip layer: ten steps per sub-block, a slab starts at a removed step)
    prog = gen.gen_kbs("bf16", 2)
    kb = next(n for n, s in enumerate(prog.segs) if s[0] == "s" and any("s_barrier" in i.text for i in s[3]))
    kind, bit, live, dead = prog.segs[kb]
    prog.segs[kb] = (kind, bit, live, [i for i in dead if "s_barrier" not in i.text])
    bodies = gen.ksx_bodies(prog)               # every body passes check() on its own: the hazard rules know nothing of the ring
    with pytest.raises(AssertionError, match="drops or reorders"):
        gen.ksx_verify(prog, bodies)
    assert _protocol(bodies[0]).count("s_barrier") - _protocol(bodies[nbits]).count("s_barrier") == 1
