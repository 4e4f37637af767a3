"""Time the preparation of a training ray batch (Trainer.sample_random_ray_batch) and the whole training iteration it feeds,
for the default host path and the two device_batches modes, on one MI355X.  One JSON line per figure.

  python tools/bench_batch_draw.py [--size 800] [--n-rand 1024] [--images 8] [--iters 30] [--modes default,gather,draw]
                                   [--dtype bf16] [--skip-step] [--memory-images 25]

  prep       per-iteration wall time of batch preparation alone (synchronised after every batch), median of --iters
  iteration  preparation + the graphed DepthNet step (production networks), fused_step off and on; in draw mode the draw is
             part of the captured graph
  memory     peak device memory of the use_batching path (rays_rgb and its epoch reshuffle) against draw mode's all-images
             scope, on --memory-images images (0 skips it)

--modes default alone needs nothing of ray_batches.py, so the same file times a checkout that predates it."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from nerf_sampling_amd import nerf_utils, ops, synthetic
from nerf_sampling_amd.autograd import HipAdam
from nerf_sampling_amd.depth_net import DepthNet
from nerf_sampling_amd.run_nerf_helpers import NeRF, get_embedder
from nerf_sampling_amd.trainers import DepthNetTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--n-rand", type=int, default=1024)
ap.add_argument("--images", type=int, default=8)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--modes", default="default,gather,draw")
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--skip-step", action="store_true")
ap.add_argument("--memory-images", type=int, default=25)
a = ap.parse_args()
modes = [m for m in a.modes.split(",") if m]
H = W = a.size
_, K = synthetic.blender_intrinsics(H, W)
ops.set_compute_dtype(a.dtype)


def scene(n):
    rng = np.random.default_rng(0)
    images = rng.random((n, H, W, 3), dtype=np.float32)
    poses = np.stack([synthetic.pose_spherical(360.0 * k / n, -30.0, 4.0).numpy() for k in range(n)]).astype(np.float32)
    return images, poses, np.arange(n)


def trainer(mode, **over):
    kw = dict(dataset_type="blender", basedir="/tmp", expname="b", no_batching=True, datadir="", half_res=False, white_bkgd=True,
              N_importance=128, N_samples=64, use_viewdirs=True, input_dims_embed=3, device="cuda", perturb=1.0, N_rand=a.n_rand)
    if mode != "default":
        kw["device_batches"] = mode
    kw.update(over)
    tr = DepthNetTrainer(**kw)
    tr.H, tr.W, tr.K = H, W, K
    return tr


def emit(**kw):
    print(json.dumps(dict(size=a.size, n_rand=a.n_rand, **kw)), flush=True)


images, poses, i_train = scene(a.images)
poses_t = torch.from_numpy(poses).cuda()

for mode in modes:
    tr = trainer(mode)
    np.random.seed(0)
    ts = []
    for i in range(a.iters + 3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        tr.sample_random_ray_batch(None, None, i_train, images, poses_t, i)
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    ts = ts[3:]
    emit(metric="batch preparation alone", mode=mode, ms_median=1e3 * statistics.median(ts), ms_min=1e3 * min(ts), ms_max=1e3 * max(ts))

if not a.skip_step:
    cfg, params = synthetic.SCENES["lego_synth"], synthetic.make_scene("lego_synth")
    nets = {}
    for which in ("coarse", "fine"):
        n = NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        n.load_state_dict(params[which]); n = n.cuda()
        for p in n.parameters(): p.requires_grad_(False)
        nets[which] = n
    e1, _ = get_embedder(10, 0, 3); e2, _ = get_embedder(4, 0, 3)
    for fused in (False, True):
        for mode in modes:
            dn = DepthNet(hidden_sizes=[256] * 10, cat_hidden_sizes=[256] * 10); dn.load_state_dict(params["depth"]); dn = dn.cuda()
            tr = trainer(mode)
            q = lambda i, v, f: tr.run_network(i, v, f, embed_fn=e1, embeddirs_fn=e2)
            kw = dict(network_query_fn=q, perturb=1.0, N_importance=128, network_fine=nets["fine"], N_samples=64,
                      network_fn=nets["coarse"], use_viewdirs=True, white_bkgd=True, raw_noise_std=0.0, trainer=tr, lindisp=True,
                      depth_network=dn, model_mode="train", near=2.0, far=6.0, ndc=False)
            if fused:
                nerf_utils.standard_query_fn(q)
                kw["fused_step"] = True
            opt = HipAdam(list(dn.parameters()), lr=1e-4)
            np.random.seed(0)
            if mode == "draw":
                run = tr.graphed_optimization_loop(opt, kw, batch_source=tr.draw_source(i_train, images, poses_t, 0))
                it = lambda i: run(None, i, None)
            else:
                run = tr.graphed_optimization_loop(opt, kw)
                def it(i):
                    _, _, rays, tgt = tr.sample_random_ray_batch(None, None, i_train, images, poses_t, i)
                    return run(rays, i, tgt)
            for i in range(5): it(i)
            torch.cuda.synchronize(); ts = []
            for i in range(5, 5 + a.iters):
                t0 = time.perf_counter(); it(i); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
            emit(metric="whole iteration: preparation + graphed DepthNet step", mode=mode, fused_step=fused, dtype=a.dtype,
                 ms_median=1e3 * statistics.median(ts), ms_min=1e3 * min(ts), ms_max=1e3 * max(ts))
            del run, opt, dn

if a.memory_images > 0:
    del images, poses_t
    images, poses, i_train = scene(a.memory_images)
    for mode in [m for m in modes if m != "gather"]:
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        tr = trainer(mode, no_batching=False)
        np.random.seed(0)
        imgs, poses_t, rays_rgb, i_batch = tr.prepare_raybatch_tensor_if_batching_random_rays(poses, images, i_train)
        steps_per_epoch = -(-a.memory_images * H * W // a.n_rand)
        # the last batches of the first epoch: the default path reshuffles rays_rgb there (its second copy)
        i_batch = max(0, (steps_per_epoch - 2) * a.n_rand) if rays_rgb is not None else i_batch
        for i in range(steps_per_epoch - 2, steps_per_epoch + 2):
            rays_rgb, i_batch, rays, tgt = tr.sample_random_ray_batch(rays_rgb, i_batch, i_train, imgs, poses_t, i)
        torch.cuda.synchronize()
        emit(metric="use_batching: peak device memory", mode=mode, images=a.memory_images,
             peak_mib=(torch.cuda.max_memory_allocated() - base) / 2 ** 20)
        del tr, imgs, rays_rgb, rays, tgt
