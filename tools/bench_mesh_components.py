"""The connected components of a mesh's faces on the device (ns_mesh_components), piece by piece on one box:

  * the entry alone (its four launches through the C ABI: no allocation, no readback), event-timed, and ops.mesh_components (with
    its allocations and its one readback), wall-timed, on the welded surface of a ball of radius 0.7 on a --resolution^3 lattice
    over [-1, 1]^3 (898 728 triangles at 256^3), beside ops.mesh_weld on the same triangles;
  * the same on the fitted scene's surface at --threshold, beside ops.mesh_weld -- the stage the new one sits next to;
  * nerf_utils.scene_mesh_filtered as a whole without and with keep_largest=1 (grid, extraction, weld, [components, selection,] colours).

The package depends on no graph library and scipy is not installed, so there is no host implementation to race: the times stand
alone.  Each time is the median of --alternations runs with the spread (max - min) beside it.

    python tools/bench_mesh_components.py [--resolution 256] [--threshold 50] [--skip-scene]
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_device_mesh import event_timed, wall_timed  # noqa: E402
from nerf_sampling_amd import _lib, nerf_utils, ops  # noqa: E402


def bench_mesh(label, triangles, keys, a, dev):
    ms_w, sp_w = wall_timed(lambda: ops.mesh_weld(triangles, keys), a.alternations)
    vertices, faces = ops.mesh_weld(triangles, keys)
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    labels, tri, vert = (torch.empty((V,), dtype=torch.int32, device=dev) for _ in range(3))
    counters = torch.empty((2,), dtype=torch.int64, device=dev)
    ws = torch.empty((ops.mesh_components_workspace_bytes(V, F),), dtype=torch.uint8, device=dev)
    lib, p = _lib.load(), lambda t: C.c_void_p(t.data_ptr())

    def call():
        _lib.check(lib.ns_mesh_components(p(faces), F, V, p(labels), p(tri), p(vert), p(counters), p(ws),
                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ns_mesh_components")

    us, sp = event_timed(call, a.alternations, a.reps)
    ms_o, sp_o = wall_timed(lambda: ops.mesh_components(faces, V), a.alternations)
    got = ops.mesh_components(faces, V)
    assert torch.equal(got["labels"], labels) and int(counters.cpu()[0]) == got["n_components"]
    sizes = torch.sort(got["triangles"][got["triangles"] > 0], descending=True).values
    print(f"  {label}: {F} triangles on {V} vertices, {got['n_components']} components (the largest: {sizes[:4].tolist()} triangles)")
    print(f"    ns_mesh_components, the entry alone   {us:9.1f} us (spread {sp:.1f})   {F / us:7.1f} M faces/s")
    print(f"    ops.mesh_components (with readback)   {ms_o:9.3f} ms (spread {sp_o:.3f})")
    print(f"    ops.mesh_weld on the same triangles   {ms_w:9.3f} ms (spread {sp_w:.3f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=50.0)
    ap.add_argument("--bound", type=float, default=1.5)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-scene", action="store_true", help="the ball alone")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    G = a.resolution
    print(f"connected components of a welded surface; median of {a.alternations} runs ({a.reps} calls each where event-timed)")
    ax = torch.linspace(-1.0, 1.0, G, device=dev)
    Z, Y, X = torch.meshgrid(ax, ax, ax, indexing="ij")
    got = ops.mesh_extract(0.7 - torch.sqrt(X * X + Y * Y + Z * Z), 0.0, [-1.0] * 3, [2.0 / (G - 1)] * 3)
    bench_mesh(f"ball r = 0.7 at {G}^3", got["triangles"], got["keys"], a, dev)
    if a.skip_scene:
        return
    import bench

    _coarse, fine, _dn, _params = bench.build_modules("shapes_fit", dev)
    ops.set_compute_dtype("bf16")
    bound = a.bound
    lo, h, _ = nerf_utils.mesh_lattice(-bound, bound, G)
    grid = nerf_utils.field_density_grid(fine, -bound, bound, G)
    got = ops.mesh_extract(grid, a.threshold, lo, h)
    bench_mesh(f"the fitted scene at {G}^3, threshold {a.threshold}", got["triangles"], got["keys"], a, dev)
    for label, kw in (("without a filter ", {}), ("keep_largest = 1 ", dict(keep_largest=1))):
        ms, sp = wall_timed(lambda: nerf_utils.scene_mesh_filtered(fine, bound=bound, resolution=G, threshold=a.threshold, **kw),
                            a.alternations)
        mesh = nerf_utils.scene_mesh_filtered(fine, bound=bound, resolution=G, threshold=a.threshold, **kw)
        print(f"  scene_mesh as a whole, bf16, colours on, no file, {label} {ms:9.2f} ms (spread {sp:.2f})   "
              f"{mesh['faces'].shape[0]} triangles on {mesh['vertices'].shape[0]} vertices")


if __name__ == "__main__":
    main()
