"""ms per held-out view of render_path(gt_imgs=...) -- the frame and its per-sample arrays copied to the host, the PSNR in numpy,
a PNG -- against nerf_utils.evaluate_views -- the frame rendered in one call, scored on the device by ns_image_sqerr -- on the
fitted scene at 800 x 800 x 64, bf16 field with the PSNR guard; and the scoring launch alone at 800 x 800.  Each figure is the
median of three alternations on one box, with the spread of the first path beside it.  --ssim: evaluate_views without and
with ssim=True instead (the host path is not run), and ns_image_ssim alone beside ns_image_sqerr.  --depth: evaluate_views
without depth, with depth=True and the field's depth maps rendered afresh, and with them passed in as field_depths, the three
alternating; then ns_depth_sqerr alone at (640 000, 64) and (640 000, 1).  --frames: render_path(gt_imgs=..., savedir=...),
evaluate_views without frames and evaluate_views(frames=True) -- the PNGs written by nerf_utils.FrameWriter -- the three
alternating; then evaluate_views(frames=...) at workers = 1, 2, 4, 8 with PIL's default compress_level and with 1; then
ns_frame_to8b alone beside ns_image_sqerr.  --video: the 40-pose spiral as the reference's i_video branch writes it -- render_path,
numpy's to8b(rgbs) and to8b(disps / np.max(disps)), PIL saves of both sequences -- against nerf_utils.write_video, the two
alternating; then ns_map_max and ns_map_to8b alone on a packed map and on the [:, 3] column of a shard.

    python tools/bench_device_eval.py [--views 6] [--size 800] [--samples 64] [--ssim | --depth | --frames | --video]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from nerf_sampling_amd import analytic_scene, nerf_utils, ops, synthetic  # noqa: E402
from nerf_sampling_amd.ray_batches import DeviceRayDataset  # noqa: E402
from nerf_sampling_amd.run_nerf_helpers import get_embedder  # noqa: E402
from nerf_sampling_amd.trainers import DepthNetTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--ssim", action="store_true", help="evaluate_views with ssim=True against without; ns_image_ssim alone")
    ap.add_argument("--depth", action="store_true",
                    help="evaluate_views without depth, with depth=True and fresh field depths, with cached ones; ns_depth_sqerr alone")
    ap.add_argument("--frames", action="store_true",
                    help="render_path with PNGs, evaluate_views without and with frames=True; the workers x compress_level "
                         "table; ns_frame_to8b alone")
    ap.add_argument("--video", action="store_true",
                    help="the 40-pose spiral: render_path + numpy + PIL saves of the rgb and disparity sequences against "
                         "write_video; ns_map_max and ns_map_to8b alone")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _coarse, fine, dn, _params = bench.build_modules("shapes_fit", dev)
    H = W = a.size
    focal, K = synthetic.blender_intrinsics(H, W)
    if a.video:                                              # the whole spiral, and no ground truth: nothing is scored
        a.views = 40
    poses = synthetic.render_poses(40)[:: 40 // a.views][: a.views].cpu()
    gt = ds = None
    if not a.video:
        gt = np.stack([analytic_scene.frame(H, W, K, p[:3, :4], device=dev)[0].float().cpu().numpy() for p in poses])
        ds = DeviceRayDataset(gt, poses.numpy().astype(np.float32), K, [0])
    ops.set_compute_dtype("bf16")
    ops.set_psnr_guard(True)
    tr = DepthNetTrainer(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="", half_res=False,
                         white_bkgd=True, N_importance=128, N_samples=64, use_viewdirs=True, input_dims_embed=3, device="cuda",
                         n_depth_samples=a.samples, sampling_mode="uniform", distance=0.1)
    e1, _ = get_embedder(10, 0, 3)
    e2, _ = get_embedder(4, 0, 3)
    q = nerf_utils.standard_query_fn(lambda i, v, f: tr.run_network(i, v, f, embed_fn=e1, embeddirs_fn=e2, netchunk=tr.netchunk))
    kw = dict(network_query_fn=q, perturb=0.0, N_importance=128, network_fine=fine, N_samples=64, network_fn=fine,
              use_viewdirs=True, white_bkgd=True, raw_noise_std=0.0, trainer=tr, lindisp=True, depth_network=dn,
              model_mode="test", near=2.0, far=6.0, ndc=False)
    ids = list(range(a.views))

    def host_path(savedir):
        with torch.no_grad():
            return nerf_utils.render_path(poses, [H, W, focal], K, tr.chunk, kw, step=0, gt_imgs=gt, savedir=savedir)[2]

    def device_path(savedir):
        return nerf_utils.evaluate_views(ds, ids, poses, [H, W, focal], K, kw, savedir=savedir)[1]

    def device_ssim_path(savedir):
        return nerf_utils.evaluate_views(ds, ids, poses, [H, W, focal], K, kw, savedir=savedir, ssim=True)[3]

    def timed(fn):
        with tempfile.TemporaryDirectory() as d:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            psnr = fn(d)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / a.views, float(psnr)

    if a.video:
        return bench_video(a, dev, poses, [H, W, focal], K, kw, tr, timed)
    if a.depth:
        return bench_depth(a, dev, ds, ids, poses, [H, W, focal], K, kw, timed)
    if a.frames:
        return bench_frames(a, dev, ds, ids, poses, [H, W, focal], K, kw, timed, host_path, device_path)
    # the first path of the pair is the one the second is measured against
    first, second = ((device_path, device_ssim_path) if a.ssim else (host_path, device_path))
    timed(first), timed(second)                              # warm-up: pinned buffers, packed streams, workspaces
    host, device = [], []
    for _ in range(a.alternations):
        host.append(timed(first))
        device.append(timed(second))
    h, d = [t for t, _ in host], [t for t, _ in device]
    print(f"{H} x {W} x {a.samples}, bf16 + PSNR guard, {a.views} views; ms per view, median of {a.alternations} alternations")
    if a.ssim:
        print(f"  evaluate_views            {statistics.median(h):8.2f}   (spread {max(h) - min(h):.2f})   avg PSNR {host[-1][1]:.4f}")
        print(f"  evaluate_views(ssim=True) {statistics.median(d):8.2f}   (spread {max(d) - min(d):.2f})   avg SSIM {device[-1][1]:.6f}")
    else:
        print(f"  render_path(gt_imgs=...)  {statistics.median(h):8.2f}   (spread {max(h) - min(h):.2f})   avg PSNR {host[-1][1]:.4f}")
        print(f"  evaluate_views            {statistics.median(d):8.2f}   (spread {max(d) - min(d):.2f})   avg PSNR {device[-1][1]:.4f}")
    # the scoring launch alone (two kernels: per-workgroup partial sums, their ordered sum)
    rgb = torch.rand((H * W, 3), device=dev)
    out = torch.empty((1,), dtype=torch.float64, device=dev)
    ws = torch.empty((ds.sqerr_workspace_bytes(H * W),), dtype=torch.uint8, device=dev)
    for _ in range(10):
        ds.image_sqerr(0, rgb, out=out, workspace=ws)
    reps, per = 200, []
    for _ in range(a.alternations):
        e0, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ds.image_sqerr(0, rgb, out=out, workspace=ws)
        e1_.record()
        torch.cuda.synchronize()
        per.append(1e3 * e0.elapsed_time(e1_) / reps)
    print(f"  ns_image_sqerr alone      {statistics.median(per):8.2f} us per {H} x {W} frame   (spread {max(per) - min(per):.2f})")
    if a.ssim:
        ws = torch.empty((ds.ssim_workspace_bytes(),), dtype=torch.uint8, device=dev)
        for _ in range(10):
            ds.image_ssim(0, rgb, out=out, workspace=ws)
        per = []
        for _ in range(a.alternations):
            e0, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ds.image_ssim(0, rgb, out=out, workspace=ws)
            e1_.record()
            torch.cuda.synchronize()
            per.append(1e3 * e0.elapsed_time(e1_) / reps)
        print(f"  ns_image_ssim alone       {statistics.median(per):8.2f} us per {H} x {W} frame   (spread {max(per) - min(per):.2f})")


def bench_frames(a, dev, ds, ids, poses, hwf, K, kw, timed, host_path, device_path):
    """--frames: the host path, the device path and the device path with its PNGs in alternation; the device path with its PNGs
    per worker count and compress_level; ns_frame_to8b alone (one launch) beside ns_image_sqerr (two) on an 800 x 800 frame"""
    H, W = hwf[0], hwf[1]

    def with_frames(**writer):
        return lambda d: nerf_utils.evaluate_views(ds, ids, poses, hwf, K, kw, savedir=d, frames=writer or True)[1]

    paths = [("render_path(gt_imgs, savedir)", host_path), ("evaluate_views", device_path),
             ("evaluate_views(frames=True)", with_frames())]
    for _name, fn in paths:
        timed(fn)                                            # warm-up: pinned buffers, packed streams, workspaces
    runs = [[] for _ in paths]
    for _ in range(a.alternations):
        for r, (_name, fn) in zip(runs, paths):
            r.append(timed(fn))
    print(f"{H} x {W} x {a.samples}, bf16 + PSNR guard, {a.views} views; ms per view, median of {a.alternations} alternations")
    for (name, _fn), r in zip(paths, runs):
        t = [ms for ms, _ in r]
        print(f"  {name:<32s} {statistics.median(t):8.2f}   (spread {max(t) - min(t):.2f})   avg PSNR {r[-1][1]:.4f}")
    print("  evaluate_views(frames=dict(workers=w, compress_level=c)), n_buffers = 4:")
    table = [(w, c) for c in (None, 1) for w in (1, 2, 4, 8)]
    runs = [[] for _ in table]
    for _ in range(a.alternations):
        for r, (w, c) in zip(runs, table):
            r.append(timed(with_frames(workers=w, compress_level=c))[0])
    for (w, c), r in zip(table, runs):
        print(f"    workers {w}  compress_level {'default' if c is None else c}   {statistics.median(r):8.2f}   "
              f"(spread {max(r) - min(r):.2f})")
    rgb = torch.rand((H * W, 3), device=dev)
    shard = torch.rand((H * W, 4), device=dev)[:, :3]
    out8 = torch.empty((H * W, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((1,), dtype=torch.float64, device=dev)
    ws = torch.empty((ds.sqerr_workspace_bytes(H * W),), dtype=torch.uint8, device=dev)
    calls = [("ns_frame_to8b alone, packed rgb", lambda: ops.frame_to8b(rgb, out=out8)),
             ("ns_frame_to8b alone, [R,4] shard", lambda: ops.frame_to8b(shard, out=out8)),
             ("ns_image_sqerr alone", lambda: ds.image_sqerr(0, rgb, out=out, workspace=ws))]
    reps = 200
    for name, call in calls:
        for _ in range(10):
            call()
        per = []
        for _ in range(a.alternations):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            per.append(1e3 * e0.elapsed_time(e1) / reps)
        print(f"  {name:<34s} {statistics.median(per):8.2f} us per {H} x {W} frame   (spread {max(per) - min(per):.2f})")


def bench_video(a, dev, poses, hwf, K, kw, tr, timed):
    """--video: the host route of the reference's i_video branch (Trainer.py:350-376, the mp4 encoder replaced by PIL saves of
    the same bytes) and write_video in alternation, ms per view of the 40-pose spiral; then ns_map_max (both launches) and
    ns_map_to8b alone on an 800 x 800 map in both layouts"""
    from PIL import Image

    from nerf_sampling_amd.run_nerf_helpers import to8b

    H, W = hwf[0], hwf[1]

    def host_route(d):
        with torch.no_grad():
            rgbs, disps, _ = nerf_utils.render_path(poses, hwf, K, tr.chunk, kw, step=0)
        with np.errstate(all="ignore"):
            rgb8, disp8 = to8b(rgbs), to8b(disps / np.max(disps))
        for name, frames in (("rgb", rgb8), ("disp", disp8)):
            os.makedirs(os.path.join(d, name))
            for k, f in enumerate(frames):
                Image.fromarray(f).save(os.path.join(d, name, "{:03d}.png".format(k)))
        return float(np.max(disps))

    def device_route(d):
        return nerf_utils.write_video(poses, hwf, K, kw, os.path.join(d, ""))["disp_max"]

    paths = [("render_path + numpy + PIL", host_route), ("write_video", device_route)]
    for _name, fn in paths:
        timed(fn)                                            # warm-up: pinned buffers, packed streams, workspaces
    runs = [[] for _ in paths]
    for _ in range(a.alternations):
        for r, (_name, fn) in zip(runs, paths):
            r.append(timed(fn))
    print(f"{H} x {W} x {a.samples}, bf16 + PSNR guard, the {a.views}-pose spiral, rgb and disparity sequences as PNGs; "
          f"ms per view, median of {a.alternations} alternations")
    for (name, _fn), r in zip(paths, runs):
        t = [ms for ms, _ in r]
        print(f"  {name:<28s} {statistics.median(t):8.2f}   (spread {max(t) - min(t):.2f})   max disparity {r[-1][1]:.6g}")
    packed = torch.rand((H * W,), device=dev)
    column = torch.rand((H * W, 4), device=dev)[:, 3]
    state = torch.empty((2,), dtype=torch.float32, device=dev)
    ws = torch.empty((ops.map_max_workspace_bytes(H * W),), dtype=torch.uint8, device=dev)
    out8 = torch.empty((H * W,), dtype=torch.uint8, device=dev)
    calls = [("ns_map_max alone, packed map", lambda: ops.map_max(packed, state=state, accumulate=True, workspace=ws)),
             ("ns_map_max alone, [:, 3] column", lambda: ops.map_max(column, state=state, accumulate=True, workspace=ws)),
             ("ns_map_to8b alone, packed map", lambda: ops.map_to8b(packed, denom=state[:1], out=out8)),
             ("ns_map_to8b alone, [:, 3] column", lambda: ops.map_to8b(column, denom=state[:1], out=out8)),
             ("ns_frame_to8b alone, packed rgb", lambda rgb=torch.rand((H * W, 3), device=dev),
              o=torch.empty((H * W, 3), dtype=torch.uint8, device=dev): ops.frame_to8b(rgb, out=o))]
    ops.map_max(packed, state=state, workspace=ws)
    reps = 200
    for name, call in calls:
        for _ in range(10):
            call()
        per = []
        for _ in range(a.alternations):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            per.append(1e3 * e0.elapsed_time(e1) / reps)
        print(f"  {name:<34s} {statistics.median(per):8.2f} us per {H} x {W} map   (spread {max(per) - min(per):.2f})")


def bench_depth(a, dev, ds, ids, poses, hwf, K, kw, timed):
    """--depth: the three evaluations in alternation, then ns_depth_sqerr alone (both launches) on the placed samples of an
    800 x 800 x 64 frame and on a depth vector of its rays"""
    field = nerf_utils.evaluate_views(ds, ids, poses, hwf, K, kw, depth=True, return_depths=True)[-1]
    field = [max_z for _z, _mean, max_z in field]
    paths = [("evaluate_views", lambda d: nerf_utils.evaluate_views(ds, ids, poses, hwf, K, kw, savedir=d)[1]),
             ("  depth=True, fresh field", lambda d: nerf_utils.evaluate_views(ds, ids, poses, hwf, K, kw, savedir=d, depth=True)[3]),
             ("  depth=True, cached field", lambda d: nerf_utils.evaluate_views(ds, ids, poses, hwf, K, kw, savedir=d, depth=True,
                                                                              field_depths=field)[3])]
    for _name, fn in paths:
        timed(fn)                                            # warm-up: packed streams, workspaces
    runs = [[] for _ in paths]
    for _ in range(a.alternations):
        for r, (_name, fn) in zip(runs, paths):
            r.append(timed(fn))
    print(f"{hwf[0]} x {hwf[1]} x {a.samples}, bf16 + PSNR guard, {a.views} views; ms per view, median of {a.alternations} alternations")
    for (name, _fn), r, what in zip(paths, runs, ("avg PSNR", "avg sample MSE", "avg sample MSE")):
        t = [ms for ms, _ in r]
        print(f"  {name:<28s} {statistics.median(t):8.2f}   (spread {max(t) - min(t):.2f})   {what} {r[-1][1]:.6g}")
    out = torch.empty((1,), dtype=torch.float64, device=dev)
    R = 640000
    ref = torch.rand((R,), device=dev) * 4.0 + 2.0
    for N in (64, 1):
        z = torch.rand((R, N), device=dev) * 4.0 + 2.0
        ws = torch.empty((ops.depth_sqerr_workspace_bytes(R, N),), dtype=torch.uint8, device=dev)
        for _ in range(10):
            ops.depth_sqerr(z, ref, out=out, workspace=ws)
        reps, per = 200, []
        for _ in range(a.alternations):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.depth_sqerr(z, ref, out=out, workspace=ws)
            e1.record()
            torch.cuda.synchronize()
            per.append(1e3 * e0.elapsed_time(e1) / reps)
        print(f"  ns_depth_sqerr alone ({R}, {N:2d}) {statistics.median(per):8.2f} us   (spread {max(per) - min(per):.2f})")


if __name__ == "__main__":
    main()
