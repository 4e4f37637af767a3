"""The field's mesh on the device, piece by piece on one box:

  * ns_mesh_extract alone on a --resolution^3 lattice (default 256), event-timed, for a lattice without a crossing, a ball and
    normal noise: us per call (count + scan, and count + scan + emit), the bytes it has to move -- every lattice point read once
    per pass, 60 bytes written per triangle -- and the TB/s that makes, beside ns_cloud_append on as many elements;
  * nerf_utils.field_density_grid on the fitted scene's field, per compute dtype;
  * ops.mesh_weld of the scene's triangles;
  * nerf_utils.scene_mesh as a whole (grid, extraction, weld, colours; no file).

The project depends on no marching-cubes or marching-tetrahedra library (skimage, mcubes, trimesh, open3d, vtk), so there is no
host implementation to race, and the numpy restatement of tests/mesh_reference.py is a yardstick for bits at toy sizes, not a
baseline: the times stand alone.  Each time is the median of --alternations runs with the spread beside it.

    python tools/bench_device_mesh.py [--resolution 256] [--threshold 50] [--skip-scene]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nerf_sampling_amd import _lib, nerf_utils, ops  # noqa: E402


def event_timed(fn, alternations, reps):
    for _ in range(3):
        fn()
    per = []
    for _ in range(alternations):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per.append(1e3 * e0.elapsed_time(e1) / reps)
    return statistics.median(per), max(per) - min(per)


def bench_kernel(a, dev):
    G = a.resolution
    ax = torch.linspace(-1.0, 1.0, G, device=dev)
    Z, Y, X = torch.meshgrid(ax, ax, ax, indexing="ij")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    lattices = [("no crossing", torch.full((G, G, G), -1.0, device=dev)), ("ball r = 0.7", 0.7 - torch.sqrt(X * X + Y * Y + Z * Z)),
                ("normal noise", torch.randn((G, G, G), device=dev, generator=gen))]
    lo, h = [-1.0] * 3, [2.0 / (G - 1)] * 3
    ws = torch.empty((ops.mesh_workspace_bytes(G, G, G),), dtype=torch.uint8, device=dev)
    print(f"ns_mesh_extract alone, {G}^3 lattice points; us per call, median of {a.alternations} x {a.reps} calls")
    for label, sigma in lattices:
        n = ops.mesh_extract(sigma, 0.0, lo, h, capacity=0, workspace=ws)["n_triangles"]
        tri = torch.empty((max(n, 1), 3, 3), dtype=torch.float32, device=dev)
        keys = torch.empty((max(n, 1), 3), dtype=torch.int64, device=dev)
        counters = torch.empty((2,), dtype=torch.int64, device=dev)
        lib, p = _lib.load(), lambda t: C.c_void_p(t.data_ptr())                 # the entry itself: no allocation, no readback

        def call(capacity):
            _lib.check(lib.ns_mesh_extract(p(sigma), 1, G, G, G, 0.0, *lo, *h, p(tri), p(keys), capacity, p(counters), p(ws),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ns_mesh_extract")

        us0, sp0 = event_timed(lambda: call(0), a.alternations, a.reps)
        us1, sp1 = event_timed(lambda: call(max(n, 1)), a.alternations, a.reps)
        assert int(counters.cpu()[0]) == n
        b0, b1 = 4 * G ** 3, 2 * 4 * G ** 3 + 60 * n
        print(f"  {label:<13s} {n:10d} triangles   count {us0:9.1f} us (spread {sp0:.1f}) {b0 / us0 / 1e6:6.2f} TB/s   "
              f"count + emit {us1:9.1f} us (spread {sp1:.1f}) {b1 / us1 / 1e6:6.2f} TB/s")
    # ns_cloud_append on as many elements: G^3 weights as G^2 rays of G samples, none and 5 % kept
    R, N = G * G, G
    o, d = torch.randn((R, 3), device=dev), torch.randn((R, 3), device=dev)
    z, w = torch.rand((R, N), device=dev), torch.rand((R, N), device=dev)
    for label, t in (("none kept", 2.0), ("5 % kept", 0.95)):
        kept = int((w >= t).sum())
        cloud = ops.PointCloud(max(kept, 1), colours=False, device=dev)

        def call():
            cloud.count_dev.zero_()
            cloud.append(o, d, z, w, min_weight=t)

        us, sp = event_timed(call, a.alternations, a.reps)
        nbytes = 2 * 4 * R * N + kept * (4 + 16) + min(kept, R) * 24
        print(f"  ns_cloud_append ({R}, {N}) {label:<10s} {us:9.1f} us (spread {sp:.1f}) {nbytes / us / 1e6:6.2f} TB/s")


def wall_timed(fn, alternations):
    fn()
    per = []
    for _ in range(alternations):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        per.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(per), max(per) - min(per)


def bench_scene(a, dev):
    import bench

    _coarse, fine, _dn, _params = bench.build_modules("shapes_fit", dev)
    G, bound = a.resolution, a.bound
    print(f"the fitted scene's field, {G}^3 lattice points over [-{bound}, {bound}]^3, threshold {a.threshold}; ms, median of "
          f"{a.alternations} runs")
    for dtype in ("bf16", "f16", "f16x3", "f32"):
        ops.set_compute_dtype(dtype)
        ms, sp = wall_timed(lambda: nerf_utils.field_density_grid(fine, -bound, bound, G), a.alternations)
        print(f"  field_density_grid {dtype:<6s} {ms:9.2f} ms (spread {sp:.2f})   {G ** 3 / ms / 1e6:6.2f} G points/s")
    ops.set_compute_dtype("bf16")
    lo, h, _ = nerf_utils.mesh_lattice(-bound, bound, G)
    grid = nerf_utils.field_density_grid(fine, -bound, bound, G)
    got = ops.mesh_extract(grid, a.threshold, lo, h)
    print(f"  density: max {float(grid.max()):.1f}, {float((grid >= a.threshold).float().mean()):.4f} of the lattice at or above the "
          f"threshold; {got['n_triangles']} triangles, {got['n_skipped']} cells skipped")
    ms, sp = wall_timed(lambda: ops.mesh_extract(grid, a.threshold, lo, h), a.alternations)
    print(f"  ops.mesh_extract (count, readback, allocation, emit) {ms:9.2f} ms (spread {sp:.2f})")
    ms, sp = wall_timed(lambda: ops.mesh_weld(got["triangles"], got["keys"]), a.alternations)
    v, _f = ops.mesh_weld(got["triangles"], got["keys"])
    print(f"  ops.mesh_weld {got['n_triangles']} triangles -> {v.shape[0]} vertices {ms:9.2f} ms (spread {sp:.2f})")
    ms, sp = wall_timed(lambda: nerf_utils.scene_mesh(fine, bound=bound, resolution=G, threshold=a.threshold), a.alternations)
    print(f"  scene_mesh as a whole, bf16, colours on, no file    {ms:9.2f} ms (spread {sp:.2f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=50.0)
    ap.add_argument("--bound", type=float, default=1.5)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-scene", action="store_true", help="the kernel alone")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    bench_kernel(a, dev)
    if not a.skip_scene:
        bench_scene(a, dev)


if __name__ == "__main__":
    main()
