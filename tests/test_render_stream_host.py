"""The render kernel's inputs, on the host (no GPU needed): the sigma-first weight stream of a production field is a
permutation of the stream every other kernel walks (ns_pack.hip), and the generated statements of its tail
(tools/gen_ob16_asm.py --render) keep the weight ring's protocol -- a drain twin issues exactly the barriers, refill pieces,
vmcnt waits and closing read-aheads of the statement it stands in for, and nothing else."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nerf_sampling_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "gen_ob16_asm.py")
CSRC = os.path.join(ROOT, "nerf_sampling_amd", "csrc")
CHUNK, SLAB = 1024, 16 * 1024
NS_E_UNSUPPORTED = -2          # include/nerf_sampling_hip.h


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_ob16_asm", GEN)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _production_tensors(seed=0, W=256, D=8):
    g = torch.Generator().manual_seed(seed)
    shapes = [(W, 63)] + [(W, W + 63) if l == 5 else (W, W) for l in range(1, D)]
    shapes += [(W, W), (1, W), (W // 2, W + 27), (3, W // 2)]          # feature, alpha, views.0, rgb
    w = [(torch.randn(s, generator=g) / s[1] ** 0.5).numpy() for s in shapes]
    b = [(0.1 * torch.randn(s[0], generator=g)).numpy() for s in shapes]
    return w, b


def _image(w, b, dtype, sigma_first, D=8, W=256, skip_mask=1 << 4):
    lib = _lib.load()
    keep_w = [np.ascontiguousarray(a, dtype=np.float32) for a in w]
    keep_b = [np.ascontiguousarray(a, dtype=np.float32) for a in b]
    wa = (C.c_void_p * len(w))(*[k.ctypes.data for k in keep_w])
    ba = (C.c_void_p * len(b))(*[k.ctypes.data for k in keep_b])
    nbytes, nbias = C.c_int64(0), C.c_int64(0)
    args = (D, W, skip_mask, 1, 4, wa, ba, dtype, int(sigma_first))
    rc = lib.ns_pack_nerf_host_image(*args, None, 0, None, 0, C.byref(nbytes), C.byref(nbias))
    if rc != _lib.NS_OK:
        return rc, None, None
    stream = np.zeros(nbytes.value, np.uint8)
    bias = np.zeros(nbias.value, np.float32)
    _lib.check(lib.ns_pack_nerf_host_image(*args, stream.ctypes.data_as(C.c_void_p), stream.size,
                                           bias.ctypes.data_as(C.c_void_p), bias.size, C.byref(nbytes), C.byref(nbias)),
               "ns_pack_nerf_host_image")
    return rc, stream, bias


@pytest.mark.parametrize("dtype", [1, 2], ids=["bf16", "f16"])
def test_sigma_first_stream_is_a_permutation_of_the_stream(dtype):
    """Chunk by chunk: the 60 slabs in front of the view layer are the same bytes; behind them the old order is nine sub-blocks
    of nine K-blocks (colour 0..7, then sigma) + pad | rgb, the new one sigma | colour 0..7 | rgb, each statement padded to the
    fragment depth and a slab boundary.  The biases move with their sub-blocks."""
    w, b = _production_tensors()
    _, old, old_bias = _image(w, b, dtype, False)
    _, new, new_bias = _image(w, b, dtype, True)
    assert old.size == new.size == 67 * SLAB and old_bias.size == new_bias.size
    head = 60 * SLAB                                             # layer 0 (2 slabs), six layers of 8, the skip layer's 10
    assert np.array_equal(old[:head], new[:head])
    oc = old[head:].reshape(-1, CHUNK)
    nc = new[head:].reshape(-1, CHUNK)
    assert oc.shape[0] == nc.shape[0] == 7 * 16
    zero = np.zeros(CHUNK, np.uint8)
    want = np.zeros_like(nc)
    want[0:9] = oc[72:81]                                        # sigma sub-block (its ninth, view K-block included)
    want[16:16 + 72] = oc[0:72]                                  # the eight colour sub-blocks, second to sixth slab
    want[96:100] = oc[96:100]                                    # rgb head, last slab
    assert np.array_equal(nc, want)
    assert all(np.array_equal(c, zero) for c in nc[9:16]) and all(np.array_equal(c, zero) for c in nc[88:96])
    assert oc[72:81].any() and oc[0:72].any() and oc[96:100].any()
    # the same multiset of chunks (padding included): a permutation
    assert sorted(c.tobytes() for c in oc) == sorted(c.tobytes() for c in nc)
    # biases: 8 layers of 256 | old: colour 128, sigma 16 | rgb 16;  new: sigma 16, colour 128 | rgb 16
    t = 8 * 256
    assert np.array_equal(old_bias[:t], new_bias[:t])
    assert np.array_equal(new_bias[t:t + 16], old_bias[t + 128:t + 144])
    assert np.array_equal(new_bias[t + 16:t + 144], old_bias[t:t + 128])
    assert np.array_equal(new_bias[t + 144:], old_bias[t + 144:]) and new_bias.size == t + 160
    assert new_bias[t] == np.float32(b[9][0]) and old_bias[t:t + 128].any()


def test_only_production_16bit_fields_have_a_sigma_first_stream():
    w, b = _production_tensors()
    assert _image(w, b, 3, True)[0] == NS_E_UNSUPPORTED            # f16x3: out of scope
    assert _image(w, b, 0, True)[0] == NS_E_UNSUPPORTED            # f32: another layout
    w6, b6 = _production_tensors(D=6)
    # six layers with the skip after layer 4: not the production program
    assert _image(w6, b6, 1, True, D=6)[0] == NS_E_UNSUPPORTED
    assert _image(w6, b6, 1, False, D=6)[0] == _lib.NS_OK


def _counts(e):
    vm = [i.text for i in e.ins if i.text.startswith("s_waitcnt vmcnt")]
    return dict(barriers=sum(i.text == "s_barrier" for i in e.ins), dma=[i.text for i in e.ins if i.kind == "dma"], vmcnt=vm,
                islab=sum("%[islab]" in i.text and i.kind == "salu" for i in e.ins),
                dsto=sum("%[dsto]" in i.text and i.kind == "salu" for i in e.ins),
                m0=[i.text for i in e.ins if " m0" in i.text])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kind,slabs_want,chunks", [("colour", 5, 72), ("rgb", 1, 4)])
def test_drain_twin_keeps_the_ring_protocol_of_its_statement(gen, dt, kind, slabs_want, chunks):
    """five tiles (the only tile count the render statements are generated for)"""
    m = gen.Map5
    full, slabs = gen.gen_layer_special(dt, kind, m)
    drain, dslabs = gen.gen_layer_special(dt, kind, m, drain=True)
    assert slabs == dslabs == slabs_want
    a, d = _counts(full), _counts(drain)
    assert a == d, (a, d)
    assert a["barriers"] == slabs and len(a["dma"]) == 4 * slabs and len(a["vmcnt"]) == slabs
    # the same closing read-ahead: the next statement's first DEPTH - 1 fragments, from the slab behind this statement's last
    tail = lambda e: [(i.text, sorted(i.writes)) for i in e.ins if i.kind == "lds"][-(gen.DEPTH - 1):]      # noqa: E731
    assert tail(full) == tail(drain) and len(tail(drain)) == gen.DEPTH - 1
    assert all(f"%[rb{slabs % gen.RING}]" in t for t, _ in tail(drain))
    kinds = [i.kind for i in drain.ins]
    assert kinds.count("mfma") == 0 and kinds.count("lds") == gen.DEPTH - 1          # no fragment and no bias read
    assert not any(i.text.startswith(("v_cvt", "v_pk", "v_accvgpr")) for i in drain.ins)
    assert [i.kind for i in full.ins].count("mfma") == m.T * chunks
    gen.check(full.ins)
    gen.check(drain.ins)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_sigma_first_statements(gen, dt):
    """sigma: one raw sub-block of nine K-blocks on the view layer's operands; colour: eight converted sub-blocks into set A
    K-blocks 0..3; together with rgb they issue the MFMAs of the view layer + rgb head and walk as many slabs"""
    m = gen.Map5
    sig, s_sl = gen.gen_layer_special(dt, "sigma", m)
    col, c_sl = gen.gen_layer_special(dt, "colour", m)
    rgb, r_sl = gen.gen_layer_special(dt, "rgb", m)
    views, v_sl = gen.gen_layer_special(dt, "views", m)
    n = lambda e: sum(i.kind == "mfma" for i in e.ins)      # noqa: E731
    assert (n(sig), n(col), n(rgb)) == (5 * 9, 5 * 72, 5 * 4) and n(sig) + n(col) == n(views)
    assert s_sl + c_sl == v_sl == 6 and r_sl == 1
    assert not any(i.text.startswith("v_cvt_pk") for i in sig.ins)
    assert sum(i.text.startswith("v_cvt_pk") for i in col.ins) == 2 * 5 * 8
    wr = set().union(*[i.writes for i in col.ins if i.text.startswith("v_accvgpr_write")])
    assert wr == {("a", 32 * t + r) for t in range(5) for r in range(16)}
    # the sigma accumulators' chain is the view layer's: the MFMAs that write tile t's accumulator of the sigma sub-block read
    # the same B operands in the same order (the fragments differ only in the register the ring hands them over in)
    def chain(e, lo, hi):
        out = []
        for i in [i for i in e.ins if i.kind == "mfma"][lo:hi]:
            ops_ = i.text.split(None, 1)[1].split(", ")
            out.append((ops_[0], ops_[2], ops_[3]))
        return out
    assert chain(sig, 0, 45) == chain(views, 5 * 72, 5 * 81)
    for e in (sig, col, rgb):
        gen.check(e.ins)


def test_generator_outputs_are_the_committed_files(tmp_path):
    out = tmp_path / "x.inc"
    subprocess.run([sys.executable, GEN, "-o", str(out)], check=True, capture_output=True)
    assert out.read_text() == open(os.path.join(CSRC, "ns_ob16_asm.inc")).read(), "regenerate: python tools/gen_ob16_asm.py"
    out2 = tmp_path / "y.inc"
    subprocess.run([sys.executable, GEN, "--render", "-o", str(out2)], check=True, capture_output=True)
    assert out2.read_text() == open(os.path.join(CSRC, "ns_ob16_render_asm.inc")).read(), "regenerate: python tools/gen_ob16_asm.py --render"
