"""Static invariants of the render kernel's gfx950 code (no GPU needed), in the style of test_kernel_invariants.py and for
nerf_render_ob16_kernel only (the third translation unit of ns_nerf_mlp_ob16.hip, NS_OB16_TU_RENDER): the five-tile production
program on the sigma-first stream, whose tail is sigma | colour, rgb OR their drain twins behind one scalar branch."""
import os
import re
import subprocess
import tempfile

import pytest

from test_kernel_invariants import LIB, LLVM, _functions, _gfx950_code_objects

NAME = b"nerf_render_ob16_kernel"
OPENING = r"ds_read_b128 v\[56:59\], v\d+$"          # a computing statement opens with its first bias read (five-tile map)
COPIES = ("v_accvgpr_mov", "v_mov_b32", "v_mov_b64", "v_accvgpr_read")


@pytest.fixture(scope="module")
def render_fns():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump not available")
    found = [co for co in _gfx950_code_objects(LIB) if NAME in co]
    assert len(found) == 1, "the render kernels live in one code object of their own"
    assert b"nerf_mlp_ob16_kernel" not in found[0]
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(found[0])
        f.flush()
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", f.name], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], capture_output=True, text=True, check=True).stdout
    fns = {k: [i.split("//")[0].strip() for i in v] for k, v in _functions(dis).items() if NAME.decode() in k}
    assert len(fns) == 2 and all("ELb0ELb1ELi5EEE" in k for k in fns), sorted(fns)      # bf16 / f16, rays, PROD, five tiles
    return fns, notes


def _statements(ins):
    """(openings of the computing statements, (first, last) instruction of every generated statement).  Every statement saves M0
    and forms the refill address in v61 right away (a computing one reads its first bias in between); it restores M0 last."""
    starts = [n for n, i in enumerate(ins) if re.match(OPENING, i)]
    spans = []
    for n, i in enumerate(ins):
        if re.match(r"s_mov_b32 s\d+, m0$", i) and any(re.match(r"v_lshl_add_u32 v61, s\d+, 14, v\d+$", j) for j in ins[n + 1:n + 3]):
            spans.append((n, next(k for k in range(n, len(ins)) if ins[k].startswith("s_mov_b32 m0,"))))
    return starts, spans


def test_render_kernel_walks_the_ring_without_scratch_or_full_dma_waits(render_fns):
    fns, notes = render_fns
    for name, ins in fns.items():
        starts, spans = _statements(ins)
        # layer 0, seven hidden layers, sigma, colour, rgb open with a bias read; the two drain twins do not: 13 statements in all
        assert len(starts) == 11 and len(spans) == 13, (name, len(starts), len(spans))
        first, last = spans[0][0], max(b for _, b in spans)
        for n, i in enumerate(ins):
            if i.startswith("scratch_"):
                assert n < first or n > last, (name, n, i)
        full_waits = sum(bool(re.search(r"s_waitcnt vmcnt\(0\)(?! *lgkmcnt)|s_waitcnt vmcnt\(0\)$", i)) for i in ins)
        assert full_waits <= 10, f"{name}: {full_waits} s_waitcnt vmcnt(0)"
        m = re.search(re.escape(name) + r".*?\.private_segment_fixed_size:\s*(\d+)", notes, re.S)
        if m:
            assert int(m.group(1)) == 0
        # every slab of the 67 is refilled once on the computing path; the drain twins refill their statements' six again
        assert sum("global_load_lds_dwordx4" in i for i in ins if "v61" in i) == 4 * (67 + 6), name
        assert sum(i == "s_barrier" for a, b in spans for i in ins[a:b]) == 67 + 6


def test_render_kernel_is_straight_line_code_with_every_mfma_once(render_fns):
    """5 225 MFMAs per 80-sample wave pass, each once: the sigma-first tail issues the view layer's and the rgb head's, split
    45 + 360 + 20, and the drain twins none; between the statements the compiler moves no activation set."""
    fns, _ = render_fns
    for name, ins in fns.items():
        assert sum("v_mfma_f32_16x16x32" in i for i in ins) == 5225, name
        starts, spans = _statements(ins)
        per = [sum("v_mfma" in i for i in ins[a:b]) for a, b in zip(starts, starts[1:] + [len(ins)])]
        assert per == [160, 640, 640, 640, 640, 800, 640, 640, 45, 360, 20], (name, per)
        # the drain twins (the statements without a bias read): ring bookkeeping only
        drains = [(a, b) for a, b in spans if not any(a <= n <= b for n in starts)]
        assert len(drains) == 2
        tail = [i for a, b in drains for i in ins[a:b + 1]]
        assert sum("global_load_lds_dwordx4" in i for i in tail) == 4 * 6 and sum(i == "s_barrier" for i in tail) == 6
        assert not any(i.startswith(("v_mfma", "v_cvt_pk", "v_pk_max", "v_accvgpr_write")) for i in tail)
        assert sum(i.startswith("ds_read_b128") for i in tail) == 2 * 3           # the two closing read-aheads
        # inside a statement the text is the generator's; between two statements the compiler may not move an activation set
        # (160 dwords).  The gap behind sigma holds the skip decision and hands the view direction to the colour statement
        # (56 moves in this build, most of them parking the ring's fragments around the branch); the gap between the rgb statement
        # and the drain twins is the join of the two arms (24); the others hold 1 .. 8.  The limits: 24 as for the five-tile
        # production kernel (test_kernel_invariants.py), 72 behind sigma -- under half a set either way
        order = sorted(spans)
        for k, ((_, e0), (s1, _)) in enumerate(zip(order, order[1:])):
            gap = ins[e0 + 1:s1]
            moves = sum(i.startswith(COPIES) or i.startswith("v_accvgpr_write") for i in gap)
            assert moves <= (72 if k == 8 else 24), (name, k, moves)
        own = [sum(i.startswith("v_accvgpr_write") for i in ins[a:b]) for a, b in order]
        assert own == [160, 0, 160, 0, 160, 0, 160, 0, 0, 80, 0, 0, 0], (name, own)      # V -> A layers, the colour statement
        # the choice between the colour statements and the drain twins is ONE scalar branch on the wave's ballot: no statement
        # runs under a partial exec mask (a saveexec between the sigma and the rgb statement would be a vector branch)
        body = [i for a, b in spans[9:] for i in ins[a:b + 1]]
        assert len(spans[9:]) == 4 and not any("saveexec" in i or i.startswith("s_cbranch") for i in body), name
        between = ins[spans[8][1]:min(a for a, _ in spans[9:])]                   # sigma's end .. the first of the four
        assert any(i.startswith(("s_cbranch_vcc", "s_cbranch_scc")) for i in between), name
