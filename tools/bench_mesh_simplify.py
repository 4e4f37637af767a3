"""A mesh simplified by vertex clustering on the device (ns_mesh_simplify), piece by piece on one box:

  * the entry alone (its seven launches through the C ABI: no allocation, no readback), event-timed, at factors 2, 4 and 8 on the
    welded surface of a ball of radius 0.7 on a --resolution^3 lattice over [-1, 1]^3, beside ops.mesh_weld and
    ns_mesh_components on the same surface -- the stages it sits next to;
  * the same on the fitted scene's surface at --threshold with keep_largest=1;
  * nerf_utils.scene_mesh_simplified as a whole at factors 0, 2, 4 and 8 (grid, extraction, weld, normals, components,
    [simplification,] colours), with vertices, faces and PLY bytes before and after;
  * nerf_utils.score_mesh_views' three scores of those meshes against --views held-out views at --size x --size.

A factor k is a cluster cell of k lattice cells (nerf_utils.simplify_lattice).  The package depends on no mesh library, so there is
no host implementation to race: the times stand alone.  Each time is the median of --alternations runs with the spread
(max - min) beside it.

    python tools/bench_mesh_simplify.py [--resolution 256] [--threshold 50] [--skip-scene]
"""
import argparse
import ctypes as C
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_device_mesh import event_timed, wall_timed  # noqa: E402
from nerf_sampling_amd import _lib, nerf_utils, ops  # noqa: E402

FACTORS = (2, 4, 8)


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def bench_surface(label, vertices, faces, lo, h, G, a, dev, triangles=None, keys=None):
    """ns_mesh_simplify alone at every factor on one welded surface, beside the weld and the components of the same surface"""
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    lib, p = _lib.load(), lambda t: C.c_void_p(t.data_ptr())
    print(f"  {label}: {F} triangles on {V} vertices")
    if triangles is not None:
        ms_w, sp_w = wall_timed(lambda: ops.mesh_weld(triangles, keys), a.alternations)
        print(f"    ops.mesh_weld on its triangles           {ms_w:9.3f} ms (spread {sp_w:.3f})")
    labels, tri, vert = (torch.empty((V,), dtype=torch.int32, device=dev) for _ in range(3))
    counters = torch.empty((6,), dtype=torch.int64, device=dev)
    ws_c = torch.empty((ops.mesh_components_workspace_bytes(V, F),), dtype=torch.uint8, device=dev)
    us_c, sp_c = event_timed(lambda: _lib.check(lib.ns_mesh_components(p(faces), F, V, p(labels), p(tri), p(vert), p(counters), p(ws_c),
                                                                       stream(dev)), "ns_mesh_components"), a.alternations, a.reps)
    print(f"    ns_mesh_components, the entry alone      {us_c:9.1f} us (spread {sp_c:.1f})")
    rep = torch.empty((V,), dtype=torch.int32, device=dev)
    out = torch.empty((F, 3), dtype=torch.int64, device=dev)
    for k in FACTORS:
        lo3, cell3, dims3 = nerf_utils.simplify_lattice(lo, h, (G, G, G), k)
        host = [np.array(lo3, np.float32), np.array(cell3, np.float32), np.array(dims3, np.int32)]
        ws = torch.empty((ops.mesh_simplify_workspace_bytes(V, F, dims3),), dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.ns_mesh_simplify(p(vertices), V, p(faces), F, *(x.ctypes.data_as(C.c_void_p) for x in host), p(rep), p(out), F,
                                            p(counters), p(ws), stream(dev)), "ns_mesh_simplify")

        us, sp = event_timed(call, a.alternations, a.reps)
        ms_o, sp_o = wall_timed(lambda: ops.mesh_simplify(vertices, faces, lo3, cell3, dims3), a.alternations)
        got = ops.mesh_simplify(vertices, faces, lo3, cell3, dims3)
        kept = int(counters.cpu()[0])
        assert torch.equal(got["rep"], rep) and kept == got["faces"].shape[0] + got["n_duplicate"]
        print(f"    factor {k}: {dims3[0]}^3 cells, {ws.numel() / 2 ** 20:6.1f} MiB   ns_mesh_simplify alone {us:9.1f} us (spread {sp:.1f})   "
              f"{(V + F) / us:7.1f} M items/s   ops.mesh_simplify (readback, renumbering, dedupe) {ms_o:8.3f} ms (spread {sp_o:.3f})   "
              f"-> {got['faces'].shape[0]} triangles on {got['vertices'].shape[0]} vertices, {got['n_duplicate']} duplicates, "
              f"{got['n_collapsed']} collapsed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=50.0)
    ap.add_argument("--bound", type=float, default=1.5)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-scene", action="store_true", help="the ball alone")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    G = a.resolution
    print(f"vertex clustering of a welded surface; median of {a.alternations} runs ({a.reps} calls each where event-timed)")
    ax = torch.linspace(-1.0, 1.0, G, device=dev)
    Z, Y, X = torch.meshgrid(ax, ax, ax, indexing="ij")
    lo, h, _ = nerf_utils.mesh_lattice(-1.0, 1.0, G)
    got = ops.mesh_extract((0.7 - torch.sqrt(X * X + Y * Y + Z * Z)).contiguous(), 0.0, lo, h)
    vertices, faces = ops.mesh_weld(got["triangles"], got["keys"])
    bench_surface(f"ball r = 0.7 at {G}^3", vertices, faces.contiguous(), lo, h, G, a, dev, got["triangles"], got["keys"])
    del got, vertices, faces
    if a.skip_scene:
        return
    from bench_mesh_raster import scene_setup

    fine, ds, poses, hwf, K, kw = scene_setup(a, dev)
    bound = a.bound
    mesh_kw = dict(bound=bound, resolution=G, threshold=a.threshold, keep_largest=1)
    base = nerf_utils.scene_mesh_shaded(fine, **mesh_kw)
    bench_surface(f"the fitted scene at {G}^3, threshold {a.threshold}, largest component", base["vertices"].contiguous(),
                  base["faces"].contiguous(), base["lo"], base["h"], G, a, dev)
    ids = list(range(a.views))
    first = nerf_utils.score_mesh_views(ds, ids, poses, hwf, K, base, 2.0, render_kwargs=kw, background=1.0)
    print(f"  scene_mesh_simplified as a whole (bf16, normals, keep_largest=1, colours on, no file) and its mesh against {a.views} "
          f"held-out views at {a.size} x {a.size}:")
    with tempfile.TemporaryDirectory() as d:
        for k in (0,) + FACTORS:
            ms, sp = wall_timed(lambda: nerf_utils.scene_mesh_simplified(fine, simplify=k, **mesh_kw), a.alternations)
            m = nerf_utils.scene_mesh_simplified(fine, simplify=k, savedir=d, **mesh_kw)
            size = os.path.getsize(os.path.join(d, "scene_mesh.ply"))
            s = nerf_utils.score_mesh_views(ds, ids, poses, hwf, K, m, 2.0, field_depths=first["field_depths"],
                                            field_accs=first["field_accs"], background=1.0)
            print(f"    factor {k}: {ms:9.2f} ms (spread {sp:.2f})   {m['faces'].shape[0]:8d} triangles on {m['vertices'].shape[0]:8d} "
                  f"vertices, PLY {size / 1e6:7.2f} MB   mesh_psnr {s['avg_mesh_psnr']:7.3f} dB  depth_mse {s['avg_depth_mse']:.4e}  "
                  f"silhouette_iou {s['avg_silhouette_iou']:.4f}  clipped {sum(s['n_clipped'])}")


if __name__ == "__main__":
    main()
