"""The device mesh rasterised and scored (ns_mesh_raster), piece by piece on one box:

  * the entry alone (its five launches through the C ABI: no allocation, no readback), event-timed at --size x --size, on the
    welded ball of radius 0.7 on a --resolution^3 lattice and on the fitted scene's mesh at --threshold, with and without the
    colour frame, each at the two path thresholds tried (ns_debug_set "mesh_raster_big_box") -- the frames of the two are
    compared bit for bit --, beside ns_mesh_components on the same mesh and one field frame of the one-call renderer;
  * a frame-covering quad (two triangles, every pixel through the workgroup launch), at both thresholds (the second puts it
    through the per-thread loop instead: what the workgroup launch is for);
  * nerf_utils.score_mesh_views per view, the field's maps rendered afresh and passed in;
  * the fitted scene's mesh_psnr, depth_mse and silhouette_iou at thresholds 25, 50 and 100 with keep_largest=1.

There is no host rasteriser on these machines to race (as there was no marching-cubes library): the times stand beside the
field frame and the component labelling instead.  Each time is the median of --alternations runs with the spread (max - min).
``bench.py`` with the switch off against the parent commit is a shell matter: alternate the two checkouts on one box.

    python tools/bench_mesh_raster.py [--size 800] [--resolution 256] [--threshold 50] [--views 4] [--skip-scene]
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_device_mesh import event_timed, wall_timed  # noqa: E402
from nerf_sampling_amd import _lib, nerf_utils, ops, synthetic  # noqa: E402

BOXES = (256, 1024)                                       # the two path thresholds tried


def entry(vertices, faces, attr, c2w, K, H, W, near, dev):
    """-> (call, outputs): the C entry on preallocated outputs and workspace"""
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    depth = torch.empty((H * W,), dtype=torch.float32, device=dev)
    tri = torch.empty((H * W,), dtype=torch.int32, device=dev)
    rgb = torch.empty((H * W, 3), dtype=torch.float32, device=dev) if attr is not None else None
    counters = torch.empty((4,), dtype=torch.int64, device=dev)
    ws = torch.empty((ops.mesh_raster_workspace_bytes(V, F, H, W),), dtype=torch.uint8, device=dev)
    lib = _lib.load()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                             # noqa: E731
    m = (C.c_float * 12)(*[float(v) for v in np.asarray(c2w, dtype=np.float32)[:3, :4].reshape(-1)])
    cam = [float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])]

    def call():
        _lib.check(lib.ns_mesh_raster(p(vertices), V, p(faces), F, p(attr), m, *cam, H, W, near, 0, 1.0, p(depth), p(tri), p(rgb),
                                      p(counters), p(ws), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "ns_mesh_raster")

    return call, (depth, tri, rgb, counters)


def bench_mesh(label, vertices, faces, attr, c2w, K, size, near, a, dev):
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    print(f"  {label}: {F} triangles on {V} vertices, frame {size} x {size}")
    kept = {}
    for colours in (False, True):
        for box in BOXES:
            call, outs = entry(vertices, faces, attr if colours else None, c2w, K, size, size, near, dev)
            with ops.debug_switch(mesh_raster_big_box=box):
                us, sp = event_timed(call, a.alternations, a.reps)
            torch.cuda.synchronize()
            key = tuple(None if t is None else t.clone() for t in outs)
            if colours in kept:
                assert all(x is None or torch.equal(x, y) for x, y in zip(key, kept[colours])), "the path threshold changed bits"
            kept[colours] = key
            counts = [int(v) for v in outs[3].cpu()]
            print(f"    ns_mesh_raster, the entry alone, {'depth + face + colour' if colours else 'depth + face         '}, "
                  f"big box {box:5d}  {us:9.1f} us (spread {sp:.1f})   {F / us:7.2f} M faces/s   counts {counts}")
    labels, tri, vert = (torch.empty((V,), dtype=torch.int32, device=dev) for _ in range(3))
    counters = torch.empty((2,), dtype=torch.int64, device=dev)
    cc_ws = torch.empty((ops.mesh_components_workspace_bytes(V, F),), dtype=torch.uint8, device=dev)
    lib, p = _lib.load(), lambda t: C.c_void_p(t.data_ptr())

    def components():
        _lib.check(lib.ns_mesh_components(p(faces), F, V, p(labels), p(tri), p(vert), p(counters), p(cc_ws),
                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ns_mesh_components")

    us_c, sp_c = event_timed(components, a.alternations, a.reps)
    print(f"    ns_mesh_components on the same mesh                                          {us_c:9.1f} us (spread {sp_c:.1f})")
    ms_o, sp_o = wall_timed(lambda: ops.mesh_rasterize(vertices, faces, c2w, size, size, K, near, rgb=attr), a.alternations)
    print(f"    ops.mesh_rasterize (allocations, one readback)                               {ms_o:9.3f} ms (spread {sp_o:.3f})")


def bench_quad(size, K, a, dev):
    # two triangles in the plane z = 3 in front of the identity camera, far larger than the frame
    e = 4.0 * size / float(K[0][0])
    vertices = torch.tensor([[-e, -e, -3.0], [e, -e, -3.0], [e, e, -3.0], [-e, e, -3.0]], dtype=torch.float32, device=dev)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int64, device=dev)
    c2w = np.eye(4, dtype=np.float32)
    print(f"  a frame-covering quad, 2 triangles, frame {size} x {size}")
    for box, how in ((BOXES[1], "the workgroup launch"), (1 << 30, "one lane per triangle")):
        call, outs = entry(vertices, faces, None, c2w, K, size, size, 0.5, dev)
        with ops.debug_switch(mesh_raster_big_box=box):
            us, sp = event_timed(call, a.alternations, max(1, a.reps // 4))
        assert int(outs[3][3]) == size * size
        print(f"    ns_mesh_raster, {how}   {us:11.1f} us (spread {sp:.1f})")


def scene_setup(a, dev):
    import bench
    from nerf_sampling_amd import analytic_scene
    from nerf_sampling_amd.ray_batches import DeviceRayDataset
    from nerf_sampling_amd.run_nerf_helpers import get_embedder
    from nerf_sampling_amd.trainers import DepthNetTrainer

    _coarse, fine, dn, _params = bench.build_modules("shapes_fit", dev)
    H = W = a.size
    focal, K = synthetic.blender_intrinsics(H, W)
    poses = synthetic.render_poses(40)[:: 40 // a.views][: a.views].cpu()
    gt = np.stack([analytic_scene.frame(H, W, K, p[:3, :4], device=dev)[0].float().cpu().numpy() for p in poses])
    ds = DeviceRayDataset(gt, poses.numpy().astype(np.float32), K, [0])
    ops.set_compute_dtype("bf16")
    ops.set_psnr_guard(True)
    tr = DepthNetTrainer(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="", half_res=False,
                         white_bkgd=True, N_importance=128, N_samples=64, use_viewdirs=True, input_dims_embed=3, device="cuda",
                         n_depth_samples=64, sampling_mode="uniform", distance=0.1)
    e1, _ = get_embedder(10, 0, 3)
    e2, _ = get_embedder(4, 0, 3)
    q = nerf_utils.standard_query_fn(lambda i, v, f: tr.run_network(i, v, f, embed_fn=e1, embeddirs_fn=e2, netchunk=tr.netchunk))
    kw = dict(network_query_fn=q, perturb=0.0, N_importance=128, network_fine=fine, N_samples=64, network_fn=fine,
              use_viewdirs=True, white_bkgd=True, raw_noise_std=0.0, trainer=tr, lindisp=True, depth_network=dn,
              model_mode="test", near=2.0, far=6.0, ndc=False)
    return fine, ds, poses, (H, W, focal), K, kw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=50.0)
    ap.add_argument("--bound", type=float, default=1.5)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-scene", action="store_true", help="the ball and the quad alone")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    G, size = a.resolution, a.size
    focal, K = synthetic.blender_intrinsics(size, size)
    pose = synthetic.pose_spherical(30.0, -30.0, 4.0).cpu().numpy()
    print(f"the mesh rasteriser; median of {a.alternations} runs ({a.reps} calls each where event-timed)")
    ax = torch.linspace(-1.0, 1.0, G, device=dev)
    Z, Y, X = torch.meshgrid(ax, ax, ax, indexing="ij")
    got = ops.mesh_extract((0.7 - torch.sqrt(X * X + Y * Y + Z * Z)).contiguous(), 0.0, [-1.0] * 3, [2.0 / (G - 1)] * 3)
    vertices, faces = ops.mesh_weld(got["triangles"], got["keys"])
    attr = (0.5 + 0.5 * vertices / 0.7).contiguous()
    bench_mesh(f"ball r = 0.7 at {G}^3", vertices, faces.contiguous(), attr, pose, K, size, 2.0, a, dev)
    bench_quad(size, K, a, dev)
    if a.skip_scene:
        return
    fine, ds, poses, hwf, K, kw = scene_setup(a, dev)
    mesh_kw = dict(bound=a.bound, resolution=G, keep_largest=1, normals=False)
    mesh = nerf_utils.scene_mesh_shaded(fine, threshold=a.threshold, **mesh_kw)
    bench_mesh(f"the fitted scene at {G}^3, threshold {a.threshold}, largest component", mesh["vertices"].contiguous(),
               mesh["faces"].contiguous(), mesh["rgb"].contiguous(), poses[0].numpy(), K, size, 2.0, a, dev)
    render = nerf_utils._field_map_renderer(kw, size, size, K, dev)
    us_f, sp_f = event_timed(lambda: render(poses[0][:3, :4]), a.alternations, 3)
    print(f"    one field frame of the one-call renderer (bf16, guard, depth + acc extras)      {us_f / 1e3:9.2f} ms (spread {sp_f / 1e3:.2f})")
    ids = list(range(a.views))
    first = nerf_utils.score_mesh_views(ds, ids, poses, hwf, K, mesh, 2.0, render_kwargs=kw, background=1.0)
    fresh = lambda: nerf_utils.score_mesh_views(ds, ids, poses, hwf, K, mesh, 2.0, render_kwargs=kw, background=1.0)   # noqa: E731
    cached = lambda: nerf_utils.score_mesh_views(ds, ids, poses, hwf, K, mesh, 2.0, field_depths=first["field_depths"],  # noqa: E731
                                                 field_accs=first["field_accs"], background=1.0)
    ms_a, sp_a = wall_timed(fresh, a.alternations)
    ms_b, sp_b = wall_timed(cached, a.alternations)
    print(f"  score_mesh_views, {a.views} views: field maps rendered {ms_a / a.views:8.2f} ms per view (spread {sp_a / a.views:.2f}), "
          f"passed in {ms_b / a.views:8.2f} ms per view (spread {sp_b / a.views:.2f})")
    print(f"  the fitted scene's mesh against {a.views} held-out views at {size} x {size}, keep_largest=1:")
    for threshold in (25.0, 50.0, 100.0):
        m = nerf_utils.scene_mesh_shaded(fine, threshold=threshold, **mesh_kw)
        s = nerf_utils.score_mesh_views(ds, ids, poses, hwf, K, m, 2.0, field_depths=first["field_depths"],
                                        field_accs=first["field_accs"], background=1.0)
        print(f"    threshold {threshold:5.0f}: {m['faces'].shape[0]:8d} triangles  mesh_psnr {s['avg_mesh_psnr']:7.3f} dB  depth_mse "
              f"{s['avg_depth_mse']:.4e}  silhouette_iou {s['avg_silhouette_iou']:.4f}  clipped {sum(s['n_clipped'])}")


if __name__ == "__main__":
    main()
