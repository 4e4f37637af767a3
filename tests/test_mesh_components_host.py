"""The component filter's host side: the reference union-find (tests/mesh_components_reference.py) on cases worked out by hand,
ops.mesh_select and nerf_utils.mesh_component_keep on CPU tensors (plain torch, no kernel), the argument checks of
ns_mesh_components through the library on a machine without a GPU, and the new switches."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mesh_components_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", CR.HAND_CASES, ids=[c[0] for c in CR.HAND_CASES])
def test_reference_on_hand_cases(case):
    faces, V, labels, tri, vert, n_components, n_ignored = CR.hand_case(case)
    got = CR.components(faces, V)
    assert np.array_equal(got[0], labels) and np.array_equal(got[1], tri) and np.array_equal(got[2], vert)
    assert got[3:] == (n_components, n_ignored)


def test_reference_on_a_strip_and_its_pieces():
    faces = CR.strip(40)
    labels, tri, vert, n, ignored = CR.components(faces, 42)
    assert (labels == 0).all() and tri[0] == 40 and vert[0] == 42 and (n, ignored) == (1, 0)
    cut = np.delete(faces, [10, 11, 25, 26], axis=0)           # two faces out: the strip falls apart between them
    labels, tri, vert, n, _ = CR.components(cut, 42)
    assert n == 3 and sorted(set(labels.tolist())) == [0, 12, 27]
    assert (tri[0], tri[12], tri[27]) == (10, 13, 13) and (vert[0], vert[12], vert[27]) == (12, 15, 15)


def _mesh():
    """two triangles on vertices {0, 2, 3, 5} (component 0), one on {1, 4, 6} (component 1), vertex 7 alone"""
    vertices = torch.arange(24, dtype=torch.float32).reshape(8, 3)
    faces = torch.tensor([[5, 3, 0], [1, 4, 6], [0, 2, 3]], dtype=torch.int64)
    labels = torch.tensor(CR.components(faces.numpy(), 8)[0])
    assert labels.tolist() == [0, 1, 0, 0, 1, 0, 1, 7]
    return vertices, faces, labels


def test_mesh_select_order_renumbering_map_and_extras():
    from nerf_sampling_amd import ops

    vertices, faces, labels = _mesh()
    rgb, tag = vertices * 0.5, torch.arange(8)
    keep = torch.zeros(8, dtype=torch.bool)
    keep[0] = True
    keep[4] = True                                            # not a root: read at the roots only, so it changes nothing
    got = ops.mesh_select(vertices, faces, labels, keep, extras=(rgb, None, tag))
    assert got["index"].dtype == torch.int64 and got["index"].tolist() == [0, -1, 1, 2, -1, 3, -1, -1]
    assert torch.equal(got["vertices"], vertices[[0, 2, 3, 5]])                  # ascending old index
    assert got["faces"].dtype == torch.int64 and got["faces"].tolist() == [[3, 2, 0], [0, 1, 2]]      # original order, renumbered
    assert torch.equal(got["extras"][0], rgb[[0, 2, 3, 5]]) and got["extras"][1] is None
    assert got["extras"][2].tolist() == [0, 2, 3, 5]
    keep = torch.zeros(8, dtype=torch.bool)
    keep[1] = keep[7] = True
    got = ops.mesh_select(vertices, faces, labels, keep)
    assert got["index"].tolist() == [-1, 0, -1, -1, 1, -1, 2, 3] and got["faces"].tolist() == [[0, 1, 2]]
    assert torch.equal(got["vertices"], vertices[[1, 4, 6, 7]]) and got["extras"] == ()


def test_mesh_select_everything_nothing_and_bad_faces():
    from nerf_sampling_amd import ops

    vertices, faces, labels = _mesh()
    rgb = vertices + 1.0
    got = ops.mesh_select(vertices, faces, labels, torch.ones(8, dtype=torch.bool), extras=(rgb,))
    assert torch.equal(got["vertices"], vertices) and torch.equal(got["faces"], faces) and torch.equal(got["extras"][0], rgb)
    assert got["index"].tolist() == list(range(8))
    got = ops.mesh_select(vertices, faces, labels, torch.zeros(8, dtype=torch.bool), extras=(rgb,))
    assert tuple(got["vertices"].shape) == (0, 3) and tuple(got["faces"].shape) == (0, 3) and tuple(got["extras"][0].shape) == (0, 3)
    assert got["faces"].dtype == torch.int64 and got["index"].tolist() == [-1] * 8
    bad = torch.cat([faces, torch.tensor([[0, 8, 2], [-1, 0, 2]])])              # out of range: they never stay
    got = ops.mesh_select(vertices, bad, labels, torch.ones(8, dtype=torch.bool))
    assert torch.equal(got["faces"], faces)
    empty = ops.mesh_select(vertices[:0], faces[:0], labels[:0], torch.zeros(0, dtype=torch.bool))
    assert tuple(empty["vertices"].shape) == (0, 3) and tuple(empty["faces"].shape) == (0, 3) and empty["index"].numel() == 0
    with pytest.raises(ValueError):
        ops.mesh_select(vertices, faces, labels, torch.ones(7, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.mesh_select(vertices, faces, labels, torch.ones(8, dtype=torch.bool), extras=(rgb[:5],))


def _five_components():
    """components of 4, 2, 4, 1 and 0 triangles at the roots 0, 6, 10, 16 and 19 (19: a vertex in no face)"""
    faces = np.concatenate([CR.strip(4), CR.strip(2) + 6, CR.strip(4) + 10, CR.strip(1) + 16])
    labels, tri, _, n, _ = CR.components(faces, 20)
    assert n == 5 and {r: int(tri[r]) for r in (0, 6, 10, 16, 19)} == {0: 4, 6: 2, 10: 4, 16: 1, 19: 0}
    return torch.tensor(labels), torch.tensor(tri)


def test_selection_rule():
    from nerf_sampling_amd.nerf_utils import mesh_component_keep

    labels, tri = _five_components()
    kept = lambda **kw: torch.nonzero(mesh_component_keep(labels, tri, **kw))[:, 0].tolist()          # noqa: E731
    assert kept() == [0, 6, 10, 16, 19]
    assert kept(min_component_triangles=1) == [0, 6, 10, 16]
    assert kept(min_component_triangles=2) == [0, 6, 10] and kept(min_component_triangles=3) == [0, 10]
    assert kept(min_component_triangles=5) == []
    assert kept(keep_largest=1) == [0]                         # 0 and 10 tie at 4 triangles: the smaller label
    assert kept(keep_largest=2) == [0, 10] and kept(keep_largest=3) == [0, 6, 10]
    assert kept(keep_largest=9) == [0, 6, 10, 16, 19]
    assert kept(min_component_triangles=2, keep_largest=1) == [0]
    assert kept(min_component_triangles=3, keep_largest=5) == [0, 10]              # both must hold
    assert kept(min_component_triangles=5, keep_largest=1) == []
    with pytest.raises(ValueError):
        mesh_component_keep(labels, tri, min_component_triangles=-1)
    with pytest.raises(ValueError):
        mesh_component_keep(labels, tri, keep_largest=-1)


def test_argument_checks_without_a_gpu():
    """every refusal comes before any HIP call: -1 (NS_E_INVALID) on a machine without a GPU, the pointers never dereferenced"""
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    p = C.c_void_p
    faces, label, tri, vert, count, ws = p(0x1000), p(0x2000), p(0x3000), p(0x4000), p(0x5000), p(0x6000)

    def call(faces=faces, F=8, V=9, label=label, tri=tri, vert=vert, count=count, ws=ws):
        return lib.ns_mesh_components(faces, F, V, label, tri, vert, count, ws, None)

    bad = [dict(F=-1), dict(V=-1), dict(F=-2 ** 63), dict(V=-2 ** 63), dict(V=2 ** 31), dict(F=2 ** 31), dict(V=2 ** 62),
           dict(faces=None), dict(label=None), dict(tri=None), dict(vert=None), dict(count=None), dict(ws=None),
           dict(count=None, V=0, F=0), dict(faces=None, V=0), dict(label=None, F=0), dict(ws=None, F=0),
           dict(count=p(0x5004)), dict(ws=p(0x6004)), dict(label=p(0x2002)), dict(label=p(0x2001)), dict(tri=p(0x3002)),
           dict(vert=p(0x4002)), dict(faces=p(0x1004))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"ns_mesh_components" in lib.ns_last_error()
    size = lib.ns_mesh_components_workspace_bytes
    assert size(9, 8) > 0 and size(9, 8) % 8 == 0 and size(0, 0) >= 0 and size(2 ** 31 - 1, 2 ** 31 - 1) > 0
    for V, F in ((-1, 8), (9, -1), (2 ** 31, 8), (9, 2 ** 31), (2 ** 62, 2 ** 62), (-2 ** 63, 0)):
        assert size(V, F) == 0, (V, F)
    assert int(re.search(r"#define NS_MESH_COMPONENTS_SHARE (\d+)",
                         open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()).group(1)) > 0


def test_ops_mesh_components_refuses_before_any_launch():
    from nerf_sampling_amd import ops

    for faces in (torch.zeros((4, 3), dtype=torch.int64), np.zeros((4, 3), np.int64), None):      # not on the device
        with pytest.raises(ValueError):
            ops.mesh_components(faces, 5)
    p = inspect.signature(ops.mesh_components).parameters
    assert list(p) == ["faces", "n_vertices", "workspace"] and p["workspace"].default is None
    assert list(inspect.signature(ops.mesh_select).parameters) == ["vertices", "faces", "labels", "keep", "extras"]


def test_new_switches_default_off_and_reject_negatives():
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.experiments.render import main
    from nerf_sampling_amd.trainers import Trainer

    p = inspect.signature(Trainer.__init__).parameters
    assert p["mesh_min_triangles"].default == 0 and p["mesh_keep_largest"].default == 0
    s = inspect.signature(nerf_utils.scene_mesh_filtered).parameters
    assert list(s) == list(inspect.signature(nerf_utils.scene_mesh).parameters) + ["min_component_triangles", "keep_largest"]
    assert s["min_component_triangles"].default == 0 and s["keep_largest"].default == 0
    assert all(s[k].default == v.default for k, v in inspect.signature(nerf_utils.scene_mesh).parameters.items())
    f = inspect.signature(nerf_utils.mesh_filter).parameters
    assert list(f) == ["vertices", "faces", "rgb", "min_component_triangles", "keep_largest"]
    assert [f[k].default for k in list(f)[2:]] == [None, 0, 0]
    base = dict(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="")
    t = Trainer(**base, device_mesh=True, mesh_min_triangles=100, mesh_keep_largest=2)
    assert (t.mesh_min_triangles, t.mesh_keep_largest) == (100, 2)
    t = Trainer(**base)
    assert (t.mesh_min_triangles, t.mesh_keep_largest) == (0, 0)
    for kw in (dict(mesh_min_triangles=-1), dict(mesh_keep_largest=-1), dict(mesh_keep_largest=1.5), dict(mesh_min_triangles="3"),
               dict(mesh_keep_largest=True)):
        with pytest.raises(ValueError):
            Trainer(**base, **kw)
    opts = {o.name: o for o in main.params}
    for name, flag in (("mesh_min_triangles", "--mesh-min-triangles"), ("mesh_keep_largest", "--mesh-keep-largest")):
        assert opts[name].default == 0 and flag in opts[name].opts
        with pytest.raises(Exception):
            opts[name].type.convert("-1", opts[name], None)
        assert opts[name].type.convert("3", opts[name], None) == 3
