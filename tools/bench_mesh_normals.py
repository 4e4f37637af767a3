"""The vertex normals of the device mesh (ns_mesh_normals), piece by piece on one box:

  * the entry alone (its two launches through the C ABI: no allocation, no readback), event-timed, and ops.mesh_normals (with its
    allocations and its one readback), wall-timed, on the welded keys of a ball of radius 0.7 on a --resolution^3 lattice over
    [-1, 1]^3, beside ops.mesh_weld and ns_mesh_components on the same surface;
  * the same on the fitted scene's surface at --threshold;
  * nerf_utils.scene_mesh_shaded as a whole without normals, with them, and with colour_view="normal".

The kernel is a gather: its time stands beside the bytes it must move -- V * (8 + 12) for the keys and the normals plus the
distinct lattice values its stencils touch, counted here -- as an effective bandwidth.  Each time is the median of --alternations
runs with the spread (max - min) beside it.

    python tools/bench_mesh_normals.py [--resolution 256] [--threshold 50] [--skip-scene]
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


def stencil_points(keys, dims):
    """the number of distinct lattice points the stencils of ``keys`` (valid, int64 on the device) read"""
    Gx, Gy, Gz = dims
    lin, code = keys >> 3, keys & 7
    a = torch.stack([lin % Gx, lin // Gx % Gy, lin // (Gx * Gy)], dim=1)
    b = a + torch.stack([code & 1, (code >> 1) & 1, code >> 2], dim=1)
    top = torch.tensor([Gx - 1, Gy - 1, Gz - 1], device=keys.device)
    row = torch.tensor([1, Gx, Gx * Gy], device=keys.device)
    seen = torch.zeros((Gx * Gy * Gz,), dtype=torch.bool, device=keys.device)
    for q in (a, b):
        at = (q * row).sum(dim=1)
        seen[at] = True
        for x in range(3):
            seen[at + (torch.clamp(q[:, x] - 1, min=0) - q[:, x]) * row[x]] = True
            seen[at + (torch.minimum(q[:, x] + 1, top[x]) - q[:, x]) * row[x]] = True
    return int(seen.sum())


def bench_surface(label, sigma, iso, h, triangles, keys, a, dev):
    Gz, Gy, Gx = (int(v) for v in sigma.shape)
    ms_w, sp_w = wall_timed(lambda: ops.mesh_weld(triangles, keys), a.alternations)
    vertices, faces = ops.mesh_weld(triangles, keys)
    unique = torch.unique(keys)
    V, F = int(unique.shape[0]), int(faces.shape[0])
    normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
    counters = torch.empty((2,), dtype=torch.int64, device=dev)
    ws = torch.empty((ops.mesh_normals_workspace_bytes(V),), dtype=torch.uint8, device=dev)
    lib, p = _lib.load(), lambda t: C.c_void_p(t.data_ptr())
    h3 = [float(v) for v in h]

    def call():
        _lib.check(lib.ns_mesh_normals(p(sigma), 1, Gx, Gy, Gz, float(iso), *h3, p(unique), V, p(normals), p(counters), p(ws),
                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ns_mesh_normals")

    us, sp = event_timed(call, a.alternations, a.reps)
    ms_o, sp_o = wall_timed(lambda: ops.mesh_normals(sigma, iso, h3, unique), a.alternations)
    got = ops.mesh_normals(sigma, iso, h3, unique)
    assert torch.equal(got["normals"], normals) and got["n_invalid"] == 0
    moved = V * (8 + 12) + 4 * stencil_points(unique, (Gx, Gy, Gz))
    labels, tri, vert = (torch.empty((V,), dtype=torch.int32, device=dev) for _ in range(3))
    cc_ws = torch.empty((ops.mesh_components_workspace_bytes(V, F),), dtype=torch.uint8, device=dev)

    def components():
        _lib.check(lib.ns_mesh_components(p(faces), F, V, p(labels), p(tri), p(vert), p(counters), p(cc_ws),
                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ns_mesh_components")

    us_c, sp_c = event_timed(components, a.alternations, a.reps)
    print(f"  {label}: {F} triangles on {V} vertices, {got['n_degenerate']} degenerate normals")
    print(f"    ns_mesh_normals, the entry alone      {us:9.1f} us (spread {sp:.1f})   {V / us:7.1f} M vertices/s   "
          f"{moved / 1e6:.1f} MB it must move: {moved / us / 1e3:.1f} GB/s")
    print(f"    ops.mesh_normals (with readback)      {ms_o:9.3f} ms (spread {sp_o:.3f})")
    print(f"    ns_mesh_components, the entry alone   {us_c:9.1f} us (spread {sp_c:.1f})")
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
    print(f"vertex normals of a welded surface; median of {a.alternations} runs ({a.reps} calls each where event-timed)")
    ax = torch.linspace(-1.0, 1.0, G, device=dev)
    Z, Y, X = torch.meshgrid(ax, ax, ax, indexing="ij")
    ball = (0.7 - torch.sqrt(X * X + Y * Y + Z * Z)).contiguous()
    h = [2.0 / (G - 1)] * 3
    got = ops.mesh_extract(ball, 0.0, [-1.0] * 3, h)
    bench_surface(f"ball r = 0.7 at {G}^3", ball, 0.0, h, got["triangles"], got["keys"], a, dev)
    if a.skip_scene:
        return
    import bench

    _coarse, fine, _dn, _params = bench.build_modules("shapes_fit", dev)
    ops.set_compute_dtype("bf16")
    bound = a.bound
    lo, h, _ = nerf_utils.mesh_lattice(-bound, bound, G)
    grid = nerf_utils.field_density_grid(fine, -bound, bound, G)
    got = ops.mesh_extract(grid, a.threshold, lo, h)
    bench_surface(f"the fitted scene at {G}^3, threshold {a.threshold}", grid, a.threshold, h, got["triangles"], got["keys"], a,
                  dev)
    for label, kw in (("without normals      ", dict(normals=False)), ("with normals         ", dict(normals=True)),
                      ("colour_view = normal ", dict(normals=True, colour_view="normal"))):
        run = lambda: nerf_utils.scene_mesh_shaded(fine, bound=bound, resolution=G, threshold=a.threshold, **kw)  # noqa: E731
        ms, sp = wall_timed(run, a.alternations)
        mesh = run()
        print(f"  scene_mesh_shaded as a whole, bf16, colours on, no file, {label} {ms:9.2f} ms (spread {sp:.2f})   "
              f"{mesh['faces'].shape[0]} triangles on {mesh['vertices'].shape[0]} vertices")


if __name__ == "__main__":
    main()
