"""ns_mesh_simplify / ops.mesh_simplify: a mesh simplified by vertex clustering on the device.  Yardstick:
tests/mesh_simplify_reference.py, numpy's restatement of the header's definitions.  rep, the emitted faces and every counter must
equal it bit for bit; nothing is compared with a tolerance.

S, the number of vertices or faces one workgroup takes per launch, is the header's NS_MESH_SIMPLIFY_SHARE.  Every call of ``run``
goes through the C ABI with rep, the emitted faces, the counters and the workspace fenced by FENCE sentinel elements before and
after, all of them holding garbage before the call; the emitted faces are checked to be untouched from the kept count (or the
capacity) on."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mesh_reference as MR
import mesh_simplify_reference as SR
from test_mesh_simplify_host import ball_lattice

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = int(re.search(r"#define NS_MESH_SIMPLIFY_SHARE (\d+)", open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()).group(1))
FENCE = 64
SENTINEL = -0x5A5A5A5B
_reference = {}


def reference(name, make):
    """(vertices, faces, lo, cell, dims, rep, faces_out, count) of a named case: built and simplified on the host once, shared,
    never modified"""
    if name not in _reference:
        vertices, faces, lo, cell, dims = make()
        vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        faces = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
        rep, out, count = SR.entry(vertices, faces, lo, cell, dims)
        for a in (vertices, faces, rep, out, count):
            a.setflags(write=False)
        _reference[name] = (vertices, faces, lo, cell, dims, rep, out, count)
    return _reference[name]


def run(vertices, faces, lo, cell, dims, capacity=None, stream=None, workspace_byte=0xA5):
    """One call through the C ABI -> (rep, the faces written, count [6]) as host arrays, after checking that nothing was written
    around the outputs, beyond min(kept, capacity) faces, around the counters or outside the workspace"""
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    V, F = vertices.shape[0], faces.shape[0]
    capacity = F if capacity is None else capacity
    stream = stream or torch.cuda.current_stream()
    need = lib.ns_mesh_simplify_workspace_bytes(V, F, *dims)
    assert need > 0 and need % 8 == 0
    host = [np.array(lo, dtype=np.float32), np.array(cell, dtype=np.float32), np.array(dims, dtype=np.int32)]
    with torch.cuda.stream(stream):
        v_dev = torch.from_numpy(vertices.copy()).cuda() if V else None
        f_dev = torch.from_numpy(faces.copy()).cuda() if F else None
        rep = torch.full((V + 2 * FENCE,), SENTINEL, dtype=torch.int32, device="cuda")
        out = torch.full((3 * capacity + 2 * FENCE,), SENTINEL, dtype=torch.int64, device="cuda")
        counters = torch.full((6 + 2 * FENCE,), SENTINEL, dtype=torch.int64, device="cuda")
        ws = torch.full((need + 2 * FENCE * 8,), workspace_byte, dtype=torch.uint8, device="cuda")
        p = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + off)        # noqa: E731
        rc = lib.ns_mesh_simplify(p(v_dev), V, p(f_dev), F, *(a.ctypes.data_as(C.c_void_p) for a in host),
                                  p(rep, 4 * FENCE) if V else None, p(out, 8 * FENCE) if F and capacity else None, capacity,
                                  p(counters, 8 * FENCE), p(ws, 8 * FENCE), C.c_void_p(stream.cuda_stream))
        assert rc == 0, lib.ns_last_error()
        stream.synchronize()
    r, o, c, w = rep.cpu().numpy(), out.cpu().numpy(), counters.cpu().numpy(), ws.cpu().numpy()
    assert (r[:FENCE] == SENTINEL).all() and (r[FENCE + V:] == SENTINEL).all(), "written outside rep[0 .. V)"
    assert (c[:FENCE] == SENTINEL).all() and (c[FENCE + 6:] == SENTINEL).all(), "written around the counters"
    assert (w[:8 * FENCE] == workspace_byte).all() and (w[8 * FENCE + need:] == workspace_byte).all(), "written outside the workspace"
    count = c[FENCE:FENCE + 6].copy()
    written = min(int(count[0]), capacity)
    assert (o[:FENCE] == SENTINEL).all() and (o[FENCE + 3 * written:] == SENTINEL).all(), "written beyond the kept faces"
    return r[FENCE:FENCE + V].copy(), o[FENCE:FENCE + 3 * written].reshape(-1, 3).copy(), count


def check(name, make, **kw):
    vertices, faces, lo, cell, dims, rep, out, count = reference(name, make)
    got = run(vertices, faces, lo, cell, dims, **kw)
    assert np.array_equal(got[2], count), f"{name}: counters {got[2].tolist()}, want {count.tolist()}"
    assert np.array_equal(got[0], rep), f"{name}: {(got[0] != rep).sum()} representatives differ"
    capacity = kw.get("capacity")
    want = out if capacity is None else out[:capacity]
    assert got[1].shape == want.shape and np.array_equal(got[1], want), f"{name}: the emitted faces differ"
    return got


@pytest.mark.parametrize("case", SR.HAND_CASES, ids=[c[0] for c in SR.HAND_CASES])
def test_hand_cases(case):
    """two members equidistant from the centroid, a lone vertex, a vertex exactly on a cell boundary and one a half step either
    side of it, vertices outside the lattice, a NaN and an infinite vertex and the faces on them, indices -1 and V, faces
    collapsing to an edge and to a point, V = 0 and F = 0: the numbers worked out by hand"""
    vertices, faces, lo, cell, dims, rep, faces_out, count = SR.hand_case(case)[:8]
    got_rep, got_faces, got_count = run(vertices, faces, lo, cell, dims)
    assert np.array_equal(got_rep, rep) and np.array_equal(got_faces, faces_out) and np.array_equal(got_count, count)


def _one_cluster():
    rng = np.random.default_rng(11)
    V, F = 3 * S + 17, 2 * S + 9
    vertices = rng.uniform(0.0, 1.0, size=(V, 3)).astype(np.float32)
    return vertices, rng.integers(0, V, size=(F, 3), dtype=np.int64), (0, 0, 0), (1, 1, 1), (1, 1, 1)


def test_all_in_one_cluster():
    """a few thousand vertices in the one cell: every atomic of a launch lands on the same 40 bytes, and n is the largest there is"""
    rep, faces, count = check("one cluster", _one_cluster)
    V, F = 3 * S + 17, 2 * S + 9
    assert (rep == rep[0]).all() and 0 <= rep[0] < V and count.tolist() == [0, F, 0, 0, 0, 1] and faces.shape == (0, 3)


def _all_alone():
    rng = np.random.default_rng(12)
    V, F = 2 * S + 5, 2 * S + 3
    cells = rng.permutation(16 ** 3)[:V]
    centre = np.stack([cells % 16, (cells // 16) % 16, cells // 256], axis=1) + rng.uniform(0.1, 0.9, size=(V, 3))
    first = rng.permutation(V)[:F]                                             # three distinct vertices per face
    faces = np.stack([first, (first + rng.integers(1, 10, size=F)) % V, (first + rng.integers(10, 20, size=F)) % V], axis=1)
    return (centre * 0.125).astype(np.float32), faces.astype(np.int64), (0, 0, 0), (0.125, 0.125, 0.125), (16, 16, 16)


def test_every_vertex_alone():
    """a cell so small that every vertex is alone: rep is the identity, the faces come back unchanged and in order"""
    vertices, faces = reference("all alone", _all_alone)[:2]
    V, F = vertices.shape[0], faces.shape[0]
    rep, out, count = check("all alone", _all_alone)
    assert np.array_equal(rep, np.arange(V)) and np.array_equal(out, faces) and count.tolist() == [F, 0, 0, 0, 0, V]


def _soup():
    vertices, faces = SR.soup(5000, 10000)
    return vertices, faces, (0, 0, 0), (1, 1, 1), (8, 8, 8)


def test_random_soup_twice():
    """5 000 vertices and 10 000 faces on an 8^3 lattice: more than two shares of every kernel and no multiple of one; the
    workspace full of 0xFF, then zeroed: the same bits"""
    assert 5000 > 2 * S and 5000 % S != 0 and 10000 > 2 * S and 10000 % S != 0
    first = check("soup", _soup, workspace_byte=0xFF)
    second = check("soup", _soup, workspace_byte=0x00)
    third = check("soup", _soup, stream=torch.cuda.Stream())
    for other in (second, third):
        assert all(np.array_equal(a, b) for a, b in zip(first, other))
    count = first[2]
    print(f"soup: counters {count.tolist()}")
    assert count[0] > 2 * S and count[1] > 1000 and count[2] == 7 and count[3] == 5 and count[4] > 0 and count[5] == 512
    assert count[:3].sum() + count[4] == 10000


@pytest.mark.parametrize("capacity", [0, 1, S - 1, S + 300, 2 * S])
def test_capacity_below_the_kept_faces(capacity):
    """what exceeds the capacity is counted and never written: ``run`` finds its sentinels behind the capacity untouched"""
    _, out, count = check("soup", _soup, capacity=capacity)
    assert count[0] > capacity and out.shape[0] == capacity


@pytest.mark.parametrize("V,F", [(1, 1), (S - 1, S), (S, S + 1), (S + 1, S - 1), (2 * S + 1, 2 * S + 1)])
def test_share_boundaries(V, F):
    def make():
        rng = np.random.default_rng(V * 7 + F)
        vertices = rng.uniform(0.0, 4.0, size=(V, 3)).astype(np.float32)
        return vertices, rng.integers(0, V, size=(F, 3), dtype=np.int64), (0, 0, 0), (1, 1, 1), (4, 4, 4)

    check(f"shares {V} {F}", make)


# ---- the analytic ball through ops.mesh_extract, ops.mesh_weld and ops.mesh_simplify -----------------------------------------
G = 24
_ball = {}


def ball():
    """the welded ball of 24^3 lattice points as device tensors: extracted once, shared, never modified"""
    from nerf_sampling_amd import ops

    if not _ball:
        sigma, lo, h = MR.sphere(G)
        got = ops.mesh_extract(torch.from_numpy(sigma).cuda(), 0.0, lo.tolist(), h.tolist())
        _ball["mesh"] = ops.mesh_weld(got["triangles"], got["keys"]) + (lo, h)
    return _ball["mesh"]


@pytest.mark.parametrize("factor", [2, 3])
def test_extracted_ball(factor):
    from nerf_sampling_amd import ops

    vertices, faces, lo, h = ball()
    lo, cell, dims = ball_lattice(lo, h, G, factor)
    host_v, host_f = vertices.cpu().numpy(), faces.cpu().numpy()
    tag = torch.arange(host_v.shape[0], device="cuda")
    got = ops.mesh_simplify(vertices, faces, lo.tolist(), cell.tolist(), dims, extras=(tag, None))
    want = SR.simplify(host_v, host_f, lo, cell, dims)
    # the reference's bits
    assert got["rep"].dtype == torch.int32 and np.array_equal(got["rep"].cpu().numpy(), want["rep"])
    assert got["index"].dtype == torch.int64 and np.array_equal(got["index"].cpu().numpy(), want["index"])
    assert got["faces"].dtype == torch.int64 and np.array_equal(got["faces"].cpu().numpy(), want["faces"])
    for k in ("n_collapsed", "n_invalid", "n_nonfinite", "n_nonfinite_faces", "n_duplicate", "n_clusters"):
        assert got[k] == want[k], k
    out_v, out_f = got["vertices"].cpu().numpy(), got["faces"].cpu().numpy()
    # every output vertex is a row of the input, bit for bit, and the extras are cut alike
    rows = got["extras"][0].cpu().numpy()
    assert got["extras"][1] is None and (np.diff(rows) > 0).all() and rows.size == got["n_clusters"] == out_v.shape[0]
    assert np.array_equal(out_v.view(np.int32), host_v[rows].view(np.int32)) and np.array_equal(want["index"][rows], np.arange(rows.size))
    assert out_f.min() >= 0 and out_f.max() < rows.size
    # a vertex and its representative lie in one cell: no farther apart than the cell's diagonal
    rep = want["rep"]
    diagonal = float(np.linalg.norm(cell.astype(np.float64)))
    moved = np.linalg.norm(host_v.astype(np.float64) - host_v[rep].astype(np.float64), axis=1)
    assert (rep >= 0).all() and moved.max() <= diagonal
    # after dedupe no two faces share a vertex set
    assert len({tuple(sorted(f)) for f in out_f.tolist()}) == out_f.shape[0]
    # the signed volume: within the input's area times the diagonal (tests/test_mesh_simplify_host.py shows that the reference
    # itself stays inside this bound at both factors, so the bound is the issue's)
    volume_in, volume_out = SR.signed_volume(host_v, host_f), SR.signed_volume(out_v, out_f)
    bound = SR.surface_area(host_v, host_f) * diagonal
    print(f"factor {factor}: {host_f.shape[0]} -> {out_f.shape[0]} faces on {host_v.shape[0]} -> {out_v.shape[0]} vertices; "
          f"volume {volume_in:.4f} -> {volume_out:.4f}, bound {bound:.4f}; moved at most {moved.max():.4f} of {diagonal:.4f}")
    assert abs(volume_out - volume_in) <= bound and 0 < out_f.shape[0] < host_f.shape[0] / factor


def test_ops_dedupe_workspace_and_argument_errors():
    from nerf_sampling_amd import ops

    vertices, faces, lo, cell, dims = (a for a in reference("soup", _soup)[:5])
    dev_v, dev_f = torch.from_numpy(vertices.copy()).cuda(), torch.from_numpy(faces.copy()).cuda()
    ws = torch.full((ops.mesh_simplify_workspace_bytes(5000, 10000, dims),), 0xFF, dtype=torch.uint8, device="cuda")
    plain = ops.mesh_simplify(dev_v, dev_f, lo, cell, dims, dedupe=False)
    again = ops.mesh_simplify(dev_v, dev_f, lo, cell, dims, dedupe=False, workspace=ws)
    deduped = ops.mesh_simplify(dev_v, dev_f, lo, cell, dims, extras=(dev_v * 2.0,))
    want_plain = SR.simplify(vertices, faces, lo, cell, dims, dedupe_faces=False)
    want = SR.simplify(vertices, faces, lo, cell, dims)
    for got, ref in ((plain, want_plain), (again, want_plain), (deduped, want)):
        assert np.array_equal(got["faces"].cpu().numpy(), ref["faces"]) and np.array_equal(got["index"].cpu().numpy(), ref["index"])
        assert np.array_equal(got["vertices"].cpu().numpy().view(np.int32), ref["vertices"].view(np.int32))
        assert all(got[k] == ref[k] for k in ("n_collapsed", "n_invalid", "n_nonfinite", "n_nonfinite_faces", "n_duplicate", "n_clusters"))
    assert plain["n_duplicate"] == 0 and deduped["n_duplicate"] > 0
    assert torch.equal(deduped["extras"][0], deduped["vertices"] * 2.0)
    empty = ops.mesh_simplify(dev_v[:0], dev_f[:0], lo, cell, dims)
    assert tuple(empty["vertices"].shape) == (0, 3) and tuple(empty["faces"].shape) == (0, 3) and empty["n_clusters"] == 0
    with pytest.raises(ValueError):
        ops.mesh_simplify(dev_v, dev_f, lo, cell, dims, workspace=ws[1:])                  # misaligned and too small
    with pytest.raises(ValueError):
        ops.mesh_simplify(dev_v.double(), dev_f, lo, cell, dims)
    with pytest.raises(ValueError):
        ops.mesh_simplify(dev_v, dev_f.to(torch.int32), lo, cell, dims)
    with pytest.raises(ValueError):
        ops.mesh_simplify(dev_v, dev_f.t(), lo, cell, dims)
    with pytest.raises(ValueError):
        ops.mesh_simplify(dev_v, dev_f, lo, cell, dims, extras=(dev_v[:7],))
