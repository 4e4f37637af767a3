"""The probe fields of tests/exact_field_probes.py on the CPU (no GPU needed): every embedding column lies in exactly one head,
the packer's fold stays a 0 / +-1 matrix, the float64 reference agrees with the fp32 oracle, an fp32 transcription of
to_rev / Trig<> stays inside the gates on every probe input -- a correct kernel passes with no row left out -- and every
mutant of the embedding is rejected by the gate of every operand type.  tests/test_gpu_exact_field_probes.py runs the
kernels on the same probes and inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_field as E
import exact_field_probes as P
import exact_tangent as X
import exact_tangent_probes as T
from nerf_sampling_amd import _lib
from oracle import nerf_oracle

PROBES = P.probes()
IDS = [f"{s}-{r}-{p}" for s, r, p in PROBES]
_inputs, _emb = {}, {}


def _sets(shape):
    if shape not in _inputs:
        _inputs[shape] = P.input_sets(shape)
    return _inputs[shape]


def _embedding(shape, name):
    """(embedding64 rows, the input set) of a shape's input set, computed once."""
    if (shape, name) not in _emb:
        s = _sets(shape)[name]
        _emb[shape, name] = P.embedding64(s["pts"], s["dirs"], E.NETWORKS[shape]["use_viewdirs"])
    return _emb[shape, name], _sets(shape)[name]


def test_every_column_is_in_exactly_one_head():
    assert len(PROBES) == 19
    for shape in P.SHAPES:
        for route in P.routes_of(shape):
            seen = []
            for s, r, p in PROBES:
                if (s, r) == (shape, route):
                    net = P.make_probe(s, r, p)
                    seen += [j for _, cols, _ in net["heads"] for j in cols]
                    assert len({c for c, _, _ in net["heads"]}) == len(net["heads"])
            assert sorted(seen) == list(range(P.ROUTE_COLUMNS[route])), (shape, route)
    assert [P.routes_of(s) for s in P.SHAPES] == [["layer0", "skip", "views"], ["layer0", "views"], ["layer0", "skip"]]
    for route in P.ROUTES:
        for cols in P.groups(route):
            assert len(cols) in (5, 6)
            info = [P.column_info(j) for j in cols]
            assert all(a != b for a, b in zip(P.PROBE_HEAD, P.PROBE_HEAD[1:]))
            assert all(a[2] != b[2] or a[1] != b[1] for a, b in zip(info, info[1:])), "neighbours share component and phase"
            if route != "views":
                assert len({a[0] for a in info}) == len(info), "two columns of a head on one level"
    assert all(P.column_of(*P.column_info(j)) == j for j in range(63))


@pytest.mark.parametrize("shape,route,part", PROBES, ids=IDS)
def test_probe_is_one_hot_and_reads_only_its_route(shape, route, part):
    net = P.make_probe(shape, route, part)
    w = dict(zip(net["names"], net["weights"]))
    for name, a in w.items():
        assert set(np.unique(a)) <= {0.0, 1.0, -1.0, 0.5, -0.5} and E.fits16(a).all()
        if name not in ("alpha", "rgb", "output"):
            assert set(np.unique(a)) <= {0.0, 1.0, -1.0} and ((a != 0).sum(axis=1) <= (2 if name == "feature" else 1)).all(), name
    assert all(not b.any() for b in net["biases"])
    # on a one-hot embedding row e_j = t every head returns w_j t for its own columns and 0 for every other column
    n = 90 if net["use_viewdirs"] else 63
    off = E.IN_PTS if route == "views" else 0
    want = np.zeros((n, net["output_ch"]))
    for c, cols, wts in net["heads"]:
        for j, wj in zip(cols, wts):
            want[off + j, c] = wj
    for t in (0.75, -0.75):
        assert (E.chain(net, t * np.eye(n)) == t * want).all()
    if route == "skip":
        assert not w["pts0"][:, 3:].any() and w["pts0"][:, :3].any(), "layer 0 of the skip route reads the raw coordinates only"
        s = net["skips"][0] + 1
        assert not w[f"pts{s}"][:, E.IN_PTS:].any(), "nothing of layer 0's reaches the layer behind the skip"


@pytest.mark.parametrize("shape,route,part", [p for p in PROBES if E.NETWORKS[p[0]]["use_viewdirs"]],
                         ids=[i for i, p in zip(IDS, PROBES) if E.NETWORKS[p[0]]["use_viewdirs"]])
def test_the_packers_fold_is_a_sign_matrix(shape, route, part):
    net = P.make_probe(shape, route, part)
    W = net["W"]
    w = dict(zip(net["names"], net["weights"]))
    b = dict(zip(net["names"], net["biases"]))
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (w["feature"], b["feature"], w["views"], b["views"])]
    wo = np.zeros((W // 2, W + 27), np.float32)
    bo = np.zeros((W // 2,), np.float32)
    _lib.check(_lib.load().ns_fold_nerf_views(W, *[a.ctypes.data_as(C.c_void_p) for a in arrs], wo.ctypes.data_as(C.c_void_p),
                                              bo.ctypes.data_as(C.c_void_p)), "ns_fold_nerf_views")
    wf, bf = E.fold_views(net)
    assert (wo.astype(np.float64) == wf).all() and not bo.any() and not bf.any()
    assert set(np.unique(wf)) <= {0.0, 1.0, -1.0}
    units = sum(2 * len(cols) for c, cols, _ in net["heads"] if c < 3)
    assert (wf != 0).any(axis=1).sum() == units and ((wf != 0).sum(axis=1) <= 2).all()
    e, _ = _embedding(shape, "points5x7")
    assert (E.folded_chain(net, e) == E.chain(net, e)).all()


def test_inputs():
    pts = P.probe_points()
    flat = pts.reshape(-1)
    assert pts.shape == (321, 3) and np.abs(pts).max() == 8 and (flat == 2.0 ** -20).any() and (flat < 0).any()
    assert ((flat == 0) & np.signbit(flat)).any() and ((flat == 0) & ~np.signbit(flat)).any()
    full = np.frexp(flat.astype(np.float64))[0] * 2.0 ** 24
    assert (full % 2 == 1).sum() > 300, "few full-mantissa components"
    x = flat.astype(np.float64)
    for l in range(10):                     # within a few ulp of a zero of the level's sine and of its cosine
        for fn in (np.sin, np.cos):
            nz = x != 0
            assert (np.abs(fn(x[nz] * 2.0 ** l)) <= 4 * 2.0 ** l * np.spacing(np.abs(flat[nz])).astype(np.float64)).any(), (l, fn)
    for R in (321, 33):
        d = P.probe_dirs(R)
        ch = P.one_component_changes(d)
        assert {0, 1, 2} <= set(ch.tolist())
        norm = np.linalg.norm(d.astype(np.float64), axis=1)
        assert (np.abs(norm - 1) < 1e-6).any() and (np.abs(norm - 1) > 0.1).any()
        same = (d[1:] == d[:-1]).all(axis=1)
        assert same.any() and (same[1:] & same[:-1]).any(), "no run of three rays"
    d = P.probe_dirs(321)                   # one sample per ray: changes at a tile boundary and inside a tile, and a tile inside a run
    change = np.flatnonzero((d[1:] != d[:-1]).any(axis=1)) + 1
    assert (change % 16 == 0).any() and (change % 16 != 0).any()
    d = P.probe_dirs(33)                    # 31 samples a ray: ray 16 begins at sample 496, a tile boundary
    assert (d[16] != d[15]).any() and (31 * 16) % 16 == 0 and (d[2] != d[3]).any() and (31 * 3) % 16 != 0
    for shape in P.SHAPES:
        for R, N in P.RAY_SHAPES:
            o, dd, z, pts = P.ray_inputs(shape, R, N)
            fused = o.astype(np.float64)[:, None, :] + dd.astype(np.float64)[:, None, :] * z.astype(np.float64)[..., None]
            assert (fused == pts.astype(np.float64)).all() and (o[:, None, :] + dd[:, None, :] * z[..., None] == pts).all()


def _state_dict(net):
    names = {f"pts{i}": f"pts_linears.{i}" for i in range(net["D"])}
    names.update(feature="feature_linear", alpha="alpha_linear", views="views_linears.0", rgb="rgb_linear", output="output_linear")
    p = {}
    for n, w, b in zip(net["names"], net["weights"], net["biases"]):
        p[names[n] + ".weight"] = torch.from_numpy(w).float()
        p[names[n] + ".bias"] = torch.from_numpy(b).float()
    return p


@pytest.mark.parametrize("shape,route,part", PROBES, ids=IDS)
def test_reference_agrees_with_the_fp32_oracle(shape, route, part):
    net = P.make_probe(shape, route, part)
    p = _state_dict(net)
    top = 0.0
    for name in _sets(shape):
        e, s = _embedding(shape, name)
        raw64 = P.reference(net, e)
        dirs = torch.from_numpy(s["dirs"]) if net["use_viewdirs"] else None
        got = nerf_oracle.run_network(p, torch.from_numpy(s["pts"]), dirs, skips=net["skips"]).double().numpy()
        ratio, at = P.worst(got.reshape(raw64.shape), raw64, P.gate(net, e, "f32"))
        assert ratio <= 1.0, (name, ratio, at)
        top = max(top, ratio)
    print(f"{shape} {route} {part}: the fp32 oracle's worst |err| / gate {top:.3f}")


@pytest.mark.parametrize("shape,route,part", PROBES, ids=IDS)
def test_transcription_of_trig_stays_inside_every_gate(shape, route, part):
    """to_rev and Trig<true> in fp32, Trig<false> up to v_sin_f32's own error: the embedding as each engine holds it, through
    the float64 chain, on every probe input"""
    net = P.make_probe(shape, route, part)
    top = {}
    for name in _sets(shape):
        e, s = _embedding(shape, name)
        raw64 = P.reference(net, e)
        for dtype in P.PROBE_DTYPES:
            key = (shape, name, dtype in P.ROUNDED_DTYPES)
            if key not in _emb:
                _emb[key] = P.embedding32(s["pts"], s["dirs"], dtype not in P.ROUNDED_DTYPES, net["use_viewdirs"])
            got = P.reference(net, P.operand(_emb[key], dtype))
            allow = P.gate(net, e, dtype)
            if dtype in P.ROUNDED_DTYPES:               # the transcription spends nothing of v_sin_f32's allowance
                allow = allow - P.VSIN_ALLOWANCE * sum(np.abs(np.array(w)).sum() * (np.arange(net["output_ch"]) == c) for c, _, w in net["heads"])
            ratio, at = P.worst(got, raw64, allow)
            assert ratio <= 1.0, (name, dtype, ratio, at)
            top[dtype] = max(top.get(dtype, 0.0), ratio)
    print(f"{shape} {route} {part}: the transcription's worst |err| / gate " + ", ".join(f"{k} {v:.3f}" for k, v in top.items()))


def _rejected(net, e, e_mut, what):
    """the mutant's raw64 leaves the gate of every operand type by more than the gate itself: no kernel error inside the gate
    can bring it back"""
    rows = np.arange(0, e.shape[0], max(1, e.shape[0] // P.MUTANT_ROWS))
    raw64, bad = P.reference(net, e[rows]), P.reference(net, e_mut[rows])
    for dtype in P.PROBE_DTYPES:
        ratio, _ = P.worst(bad, raw64, P.gate(net, e[rows], dtype))
        assert ratio > 2.0, f"{what}: moves raw by {ratio:.3g} of the {dtype} gate only"


@pytest.mark.parametrize("shape,route,part", PROBES, ids=IDS)
def test_column_mutants_are_rejected(shape, route, part):
    """sine and cosine swapped, the level off by one, the component (i + 1) mod 3, the column zeroed: each column in turn"""
    net = P.make_probe(shape, route, part)
    e, s = _embedding(shape, "points321")
    x3 = (s["dirs"] if route == "views" else s["pts"].reshape(-1, 3)).astype(np.float64)
    lo, hi = (E.IN_PTS, e.shape[1]) if route == "views" else (0, E.IN_PTS)
    count = 0
    for _, cols, _ in net["heads"]:
        for j in cols:
            for kind in P.COLUMN_MUTANTS:
                part_mut = P.mutate_column(x3, e[:, lo:hi], j, kind)
                if part_mut is None:
                    continue
                e_mut = e.copy()
                e_mut[:, lo:hi] = part_mut
                _rejected(net, e, e_mut, f"column {j} {kind}")
                count += 1
    assert count >= 4 * sum(len(c) for _, c, _ in net["heads"]) - 2 * 3


@pytest.mark.parametrize("shape,route,part", [p for p in PROBES if p[1] == "skip"], ids=[i for i, p in zip(IDS, PROBES) if p[1] == "skip"])
def test_exchanged_stash_slots_are_rejected(shape, route, part):
    net = P.make_probe(shape, route, part)
    for name in ("points321", "rays33x31"):
        e, _ = _embedding(shape, name)
        e_mut = e.copy()
        e_mut[:, :E.IN_PTS] = P.stash_exchanged(e[:, :E.IN_PTS])
        _rejected(net, e, e_mut, f"stash slots exchanged on {name}")


@pytest.mark.parametrize("shape,route,part", [p for p in PROBES if p[1] == "views"], ids=[i for i, p in zip(IDS, PROBES) if p[1] == "views"])
def test_a_stale_view_embedding_is_rejected(shape, route, part):
    """the previous ray's embedding reused where one component alone differs: each component in turn"""
    net = P.make_probe(shape, route, part)
    for name in ("points321", "points33x31", "rays33x31"):
        e, s = _embedding(shape, name)
        ch = P.one_component_changes(s["dirs"])
        N = s["pts"].shape[1]
        for comp in range(3):
            rays = np.flatnonzero(ch == comp)
            assert len(rays)
            dirs = s["dirs"].copy()
            dirs[rays] = s["dirs"][rays - 1]
            e_mut = P.embedding64(s["pts"], dirs)
            rows = (rays[:, None] * N + np.arange(N)[None, :]).reshape(-1)
            raw64, bad = P.reference(net, e[rows]), P.reference(net, e_mut[rows])
            for dtype in P.PROBE_DTYPES:
                ratio, _ = P.worst(bad, raw64, P.gate(net, e[rows], dtype))
                assert ratio > 2.0, (name, comp, dtype, ratio)
    assert (P.stale_dirs(s["dirs"]) != s["dirs"]).any()


# ---- the tangent probes (tests/exact_tangent_probes.py) -------------------------------------------------------------
TPROBES = T.probes()
TIDS = [f"{s}-{r}-{p}" for s, r, p in TPROBES]


def test_every_columns_derivative_is_in_exactly_one_head():
    assert len(TPROBES) == 12
    for shape in T.SHAPES:
        for route in T.ROUTES:
            nets = [T.network(*p) for p in TPROBES if p[:2] == (shape, route)]
            if not nets:
                assert (shape, route) == ("d2w128", "skip")
                continue
            seen = sorted(j for net in nets for c, cols, _ in net["heads"] for j in cols)
            assert seen == list(range(63)) and all(c < 3 for net in nets for c, _, _ in net["heads"])
            for net in nets:
                w = dict(zip(net["names"], net["weights"]))
                b = dict(zip(net["names"], net["biases"]))
                assert not w["alpha"].any() and b["alpha"][0] == T.SIGMA and (net["raw"][:, 3] == T.SIGMA).all()
                assert (net["G"][:, 3] == 0).all() and len(np.unique(net["G"][:, 0])) > 50


@pytest.mark.parametrize("shape,route,part", TPROBES, ids=TIDS)
def test_tangent_reference(shape, route, part):
    """the tables against torch autograd of the literal chain in float64; the pool's points are dyadic and o + d z is exact;
    an activation is exactly zero only for a sine at p_i = 0, where the transcription's sine is 0 too, and no other is small"""
    net = T.network(shape, route, part)
    r = net["rays"]
    pts = r["o"][:, None, :] + r["d"][:, None, :] * r["z"][None, :, None]
    assert (net["points"] == pts.reshape(-1, 3)).all() and E.is_f32(pts) and (pts * 8 == np.rint(pts * 8)).all()
    p = {k: v.double() for k, v in _state_dict(net).items()}
    rows = np.arange(0, len(net["points"]), 5)
    z = torch.zeros(len(rows), 1, dtype=torch.float64, requires_grad=True)
    x = torch.from_numpy(net["points"][rows]) + torch.from_numpy(net["dirs"][rows]) * z
    emb = torch.cat([nerf_oracle.posenc(x, 10), torch.from_numpy(net["pool"][rows, E.IN_PTS:])], -1)
    raw = nerf_oracle.nerf_forward(p, emb, skips=net["skips"])
    assert np.abs(raw.detach().numpy() - net["raw"][rows]).max() < 1e-12
    for c in range(4):
        (g,) = torch.autograd.grad(raw[:, c].sum(), z, retain_graph=True)
        assert np.abs(g[:, 0].numpy() - net["G"][rows, c]).max() <= 1e-12 * (1 + net["Gabs"][rows, c].max()), c
    e = net["pool"][:, :E.IN_PTS]
    zero = e == 0
    sines = np.array([P.column_info(j)[1] == 0 for j in range(63)])
    comp = np.array([P.column_info(j)[2] for j in range(63)])
    assert zero.any() and (zero == ((net["points"][:, comp] == 0) & sines[None, :])).all()
    assert np.abs(e[~zero]).min() >= T.MIN_ACTIVATION
    for precise in (True, False):
        e32 = P.gamma32(net["points"].astype(np.float32), 10, precise)
        assert ((e32 == 0) == zero).all() and (np.sign(e32) == np.sign(e)).all()


@pytest.mark.parametrize("instance", T.INSTANCES)
@pytest.mark.parametrize("shape,route,part", TPROBES, ids=TIDS)
def test_tangent_transcription_and_mutants(shape, route, part, instance):
    """an fp32 transcription of embed3_tan, the operand tiles and walk_samples stays inside the bound on every ray; a tangent
    without its 2^l, with the primal's phase, or with pd of the wrong component leaves it in every colour channel"""
    net = T.network(shape, route, part)
    tr = T.transcription(net, instance)
    top = 0.0
    for case in T.cases(net, instance):
        assert len(case["ray"]) <= 32
        ref = T.jacobian64(net, case, instance)
        if case["N"] > 1:
            assert np.isnan(case["mean"][T.NAN_AT]) and (ref["samples"]["dz"] == 0).all(axis=1).sum() == 1
            assert (ref["samples"]["dz"][np.arange(len(ref["keep"])) != T.CLIPPED_AT - 1].sum(axis=1) > 1).all()
            J = X.walk_fp32(tr, case)
        else:
            S = X._single64(tr, case)
            J = S["J"]
        ratio = np.abs(J - ref["J"]) / ref["bound"]
        assert ratio.max() <= 1.0, (case["N"], case["white"], float(ratio.max()))
        top = max(top, float(ratio.max()))
        heads = [c for c, _, _ in net["heads"]]
        for mutant in T.TANGENT_MUTANTS:
            got = X.jacobian64(T.mutated(net, mutant), case, instance="f16x3" if instance == "single" else instance)["J"]
            move = (np.abs(got - ref["J"]) / ref["bound"]).max(axis=0)
            assert (move[heads] > 2.0).all(), (mutant, case["N"], case["white"], move[:3])
    print(f"{shape} {route} {part} {instance}: the transcription's worst |J - J64| / bound {top:.3f}")
