"""Mirror of the trainer-side operators the render path calls back into.

Reference: nerf_sampling/nerf_pytorch/trainers/Trainer.py (run_network :789-806,
sample_coarse_points :579-649, sample_fine_points :651-710, _sample_points :553-577, train :712-787,
core_optimization_loop :506-544, the two batch samplers :232-269 / :400-475), trainers/Blender.py,
nerf_sampling/trainers/sampling_trainer.py (DepthNetTrainer.raw2outputs :153-230, create_nerf_model :54-122,
save_rays_data :124-138).  ``train`` renders (render_only) or runs the DepthNet optimisation loop on the HIP backward
kernels (autograd.py); wandb / optuna logging is out of scope, and the i_video branch is honoured under
device_video (PNG sequences; the mp4s where imageio is installed).
"""

from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from . import nerf_utils, ops, utils
from .depth_net import DepthNet
from .run_nerf_helpers import Embedder, NeRF


class Trainer:
    """Attribute bag with the reference's constructor arguments and defaults (Trainer.py:19-130).

    Not in the reference: ``hip_graph`` (default on) and, off by default, ``device_batches`` / ``batch_seed`` and the device
    evaluation of held-out views -- ``device_eval`` (psnr.txt scored on the device, i_testset honoured by train()), with it
    ``device_ssim`` (ssim.txt) and ``device_depth`` (depth.txt: per view the MSE of the DepthNet's placed samples and of its
    own depth against the field's max-weight depth, "[TRAIN] Iter: i test depth MSE: x mean MSE: y"; the field's depth maps
    of the i_test views are rendered once while train_depth_net_only keeps the field frozen and the test perturb is 0) and
    ``device_frames`` (NNN.png beside every psnr.txt, quantised on the device and encoded by nerf_utils.FrameWriter's threads)
    and ``device_video`` (i_video honoured by train(): the spiral's rgb and disparity sequences through nerf_utils.write_video).
    All four need device_eval."""

    def __init__(self, dataset_type, basedir, expname, no_batching, datadir, device="cpu", render_test=False,
                 config_path=None, N_rand=32 * 32 * 4, render_only=False, chunk=1024 * 32, render_factor=0,
                 multires=10, i_embed=0, multires_views=4, netchunk=1024 * 64, lrate=5e-4, lrate_decay=250,
                 use_viewdirs=True, N_importance=0, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                 ft_path=None, perturb=1.0, raw_noise_std=0.0, N_samples=64, lindisp=True, precrop_iters=0,
                 precrop_frac=0.5, i_weights=10000, i_testset=100, i_video=5000, i_print=100,
                 input_dims_embed: int = 1, save_train_set_render: bool = True, depth_net_lr: float = 0.0001,
                 train_depth_net_only: bool = False, trial=None, single_image=False, single_ray=False,
                 save_scene_data=False, compare_nerf=False, use_nerf_max_pts=False, use_full_nerf=False,
                 hip_graph: bool = True, device_batches=False, batch_seed: int = 0, device_eval: bool = False,
                 device_ssim: bool = False, device_depth: bool = False, device_cloud: bool = False,
                 cloud_min_weight: float = 0.0, cloud_points: Optional[int] = None, device_frames: bool = False,
                 device_video: bool = False, device_mesh: bool = False, mesh_resolution: int = 256,
                 mesh_threshold: float = 50.0, mesh_bound: float = 1.5, mesh_min_triangles: int = 0,
                 mesh_keep_largest: int = 0, mesh_normals: bool = False, mesh_colour_view: str = "centre",
                 device_mesh_eval: bool = False, mesh_simplify: float = 0):
        for k, v in list(locals().items()):
            if k != "self":
                setattr(self, k, v)
        self.use_batching = not no_batching
        # device_batches (not in the reference; default off): batches come from a dataset resident on the device
        # (ray_batches.DeviceRayDataset).  "gather": the host draws below, uploaded as indices -- the same batch bit for bit;
        # "draw": the kernel draws them with its own generator (seed: batch_seed), which is NOT np.random's stream.
        self.device_batches = device_batches or False
        if self.device_batches not in (False, "gather", "draw"):
            raise ValueError(f"device_batches: False, 'gather' or 'draw', got {device_batches!r}")
        if self.device_batches == "gather" and self.use_batching:
            raise ValueError("device_batches='gather' repeats the no_batching draws; with use_batching choose 'draw'")
        if self.device_batches == "draw" and single_ray:
            raise ValueError("single_ray names its ray on the host: use device_batches='gather'")
        self._ray_dataset = self._draw_source = None
        # device_eval (not in the reference; default off): held-out views are scored on the device (nerf_utils.evaluate_views)
        # -- render(render_test=True) writes its psnr.txt that way, and train() honours i_testset as the reference's
        # Trainer.log does (Trainer.py:289-316).  Off, i_testset stays unused.
        self.device_eval = bool(device_eval)
        if self.device_eval and (compare_nerf or use_nerf_max_pts):
            raise ValueError("device_eval reports a PSNR only: compare_nerf / use_nerf_max_pts report more (render_path)")
        # device_ssim (not in the reference; default off): the device evaluation also reports the SSIM of every view
        # (ns_image_ssim) -- ssim.txt beside each psnr.txt it writes
        self.device_ssim = bool(device_ssim)
        if self.device_ssim and not self.device_eval:
            raise ValueError("device_ssim scores the frames of the device evaluation: it needs device_eval=True")
        # device_depth (not in the reference; default off): the device evaluation also reports, per view, the MSE of the placed
        # samples and of the DepthNet's own depth against the field's max-weight depth (ns_depth_sqerr; the reference's
        # compare_nerf "MSE:", nerf_utils.py:311-317, and depth_net_loss on held-out rays) -- depth.txt beside each psnr.txt.
        # With train_depth_net_only and a test perturb of 0 the field's depth maps of the i_test views cannot change: train()
        # keeps them from its first evaluation (_field_depths); in any other case they are rendered at every evaluation.
        self.device_depth = bool(device_depth)
        if self.device_depth and not self.device_eval:
            raise ValueError("device_depth scores the depths of the device evaluation: it needs device_eval=True")
        self._field_depths = None
        # device_cloud (not in the reference; default off): render() also selects the scene's point cloud of the rendered poses
        # on the device (nerf_utils.scene_cloud, ns_cloud_append) -- scene_cloud.pt and scene_cloud.ply beside the frames: the
        # samples whose weight is at least cloud_min_weight (0.0 is the reference's plot.py:17; raise it), and at most
        # cloud_points of them at random.  The frames and psnr.txt are those of the run without the switch.
        self.device_cloud = bool(device_cloud)
        self.cloud_min_weight = float(cloud_min_weight)
        self.cloud_points = None if cloud_points is None else int(cloud_points)
        if self.cloud_points is not None and self.cloud_points < 0:
            raise ValueError("cloud_points must be >= 0")
        # device_frames (not in the reference; default off): the device evaluation also writes its frames as NNN.png beside
        # psnr.txt -- render_path's files -- through nerf_utils.FrameWriter: quantised on the device (ns_frame_to8b), copied as
        # bytes and encoded off the rendering thread.  render() and evaluate_testset() honour it; the scores keep their bits.
        self.device_frames = bool(device_frames)
        if self.device_frames and not self.device_eval:
            raise ValueError("device_frames writes the frames of the device evaluation: it needs device_eval=True")
        # device_video (not in the reference's form; default off): train() honours i_video as the reference's i_video branch
        # does (Trainer.py:350-376) -- every i_video iterations render_poses, the spiral, goes through nerf_utils.write_video:
        # {expname}_spiral_{i:06d}_rgb/NNN.png and ..._disp/NNN.png (and the two mp4s where imageio is installed), one one-call
        # render per pose, the disparity's maximum kept on the device (ns_map_max, ns_map_to8b).  render() without render_test
        # writes the spiral the same way.  Off, i_video stays unused.
        self.device_video = bool(device_video)
        if self.device_video and not self.device_eval:
            raise ValueError("device_video renders the spiral as the device evaluation renders its views: it needs device_eval=True")
        # device_mesh (not in the reference; default off): render() also extracts the isosurface of the field's density on the
        # device (nerf_utils.scene_mesh, ns_mesh_extract) -- scene_mesh.ply beside the frames: the density of the fine network
        # (the coarse one where there is none) on a mesh_resolution^3 lattice over [-mesh_bound, mesh_bound]^3, cut at
        # mesh_threshold (50 is a starting value, not a property of a scene: lower it where the surface has holes).  The
        # floaters that brings are dropped by the component filter (nerf_utils.mesh_filter, ns_mesh_components; default off):
        # only the connected components of at least mesh_min_triangles triangles stay, and of those only the
        # mesh_keep_largest largest.  The frames and psnr.txt are those of the run without the switch.
        self.device_mesh = bool(device_mesh)
        self.mesh_resolution, self.mesh_threshold, self.mesh_bound = int(mesh_resolution), float(mesh_threshold), float(mesh_bound)
        if self.mesh_resolution < 2 or not self.mesh_bound > 0.0:
            raise ValueError("mesh_resolution must be at least 2 and mesh_bound positive")
        for name in ("mesh_min_triangles", "mesh_keep_largest"):
            value = getattr(self, name)
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0:
                raise ValueError(f"{name} must be a non-negative integer, got {value!r}")
            setattr(self, name, int(value))
        # mesh_normals (default off): scene_mesh.ply also carries per-vertex normals (nerf_utils.scene_mesh_shaded,
        # ns_mesh_normals: the density lattice's gradient at each vertex's lattice edge), so that a viewer shades the surface and
        # not its slivers.  mesh_colour_view: "centre" queries a vertex's colour looking towards the box centre, as ever;
        # "normal" (it needs mesh_normals) looking at the surface along its inward normal.
        if not isinstance(mesh_normals, (bool, np.bool_)):
            raise ValueError(f"mesh_normals must be a bool, got {mesh_normals!r}")
        self.mesh_normals = bool(mesh_normals)
        if mesh_colour_view not in ("centre", "normal"):
            raise ValueError(f"mesh_colour_view: 'centre' or 'normal', got {mesh_colour_view!r}")
        if mesh_colour_view == "normal" and not self.mesh_normals:
            raise ValueError("mesh_colour_view='normal' looks along the vertex normals: it needs mesh_normals=True")
        # device_mesh_eval (default off; it needs device_mesh): after scene_mesh.ply is written, render(render_test=True) rasterises
        # the mesh from the held-out cameras (ns_mesh_raster) and scores it where it is made (nerf_utils.score_mesh_views):
        # mesh_psnr.txt against the photographs, mesh_depth.txt and mesh_iou.txt against the field's own depth and opacity maps
        # -- a number for mesh_threshold and for what the component filter dropped.  Off: no launch, no file, no changed byte.
        if not isinstance(device_mesh_eval, (bool, np.bool_)):
            raise ValueError(f"device_mesh_eval must be a bool, got {device_mesh_eval!r}")
        self.device_mesh_eval = bool(device_mesh_eval)
        if self.device_mesh_eval and not self.device_mesh:
            raise ValueError("device_mesh_eval scores the mesh of device_mesh: it needs device_mesh=True")
        # mesh_simplify (default 0: off, no launch, no changed byte): scene_mesh.ply is the surface simplified by vertex clustering
        # (nerf_utils.scene_mesh_simplified, ns_mesh_simplify) on cluster cells mesh_simplify lattice cells wide -- about
        # mesh_simplify^2 times fewer triangles, every vertex one of the unsimplified surface's; device_mesh_eval scores that mesh.
        if isinstance(mesh_simplify, (bool, np.bool_)) or not isinstance(mesh_simplify, (int, float, np.integer, np.floating)) \
                or not (float(mesh_simplify) >= 0.0 and np.isfinite(float(mesh_simplify))):
            raise ValueError(f"mesh_simplify must be a finite number >= 0, got {mesh_simplify!r}")
        self.mesh_simplify = float(mesh_simplify)
        self.no_reload = False
        self.start = None
        self.K = self.global_step = self.W = self.H = self.c2w = None

    def cast_intrinsics_to_right_types(self, hwf):
        H, W, focal = hwf
        H, W = int(H), int(W)
        if self.K is None:
            self.K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
        self.H, self.W = H, W
        return [H, W, focal]

    # ---- operators called from render_rays / render_rays_test ------------------------------------
    def run_network(self, inputs, viewdirs, fn, embed_fn, embeddirs_fn, netchunk=1024 * 64):
        """Embed + MLP: inputs [R,N,3], viewdirs [R,3] -> [R,N,4]  (Trainer.py:789-806).

        With this package's NeRF module and 10/4-frequency embedders the whole operator is one
        MFMA kernel (no [R*N,90] embedding in memory, no netchunk loop).
        """
        fused = (isinstance(fn, NeRF) and isinstance(embed_fn, Embedder) and embed_fn.num_freqs == 10
                 and embed_fn.input_dims == 3)
        if fused and fn.use_viewdirs:
            fused = (viewdirs is not None and isinstance(embeddirs_fn, Embedder) and embeddirs_fn.num_freqs == 4
                     and embeddirs_fn.input_dims == 3)
        elif fused:                       # output_linear head: the reference feeds the 63 point features only
            fused = viewdirs is None
        if fused:
            if torch.is_grad_enabled() and inputs.requires_grad:   # training: gradient w.r.t. the points only
                from .autograd import NerfInputGrad

                return NerfInputGrad.apply(inputs, viewdirs, fn)
            return ops.nerf_forward(fn.packed(), inputs, viewdirs)
        inputs_flat = torch.reshape(inputs, [-1, inputs.shape[-1]])
        embedded = embed_fn(inputs_flat)
        if viewdirs is not None:
            input_dirs = viewdirs[:, None].expand(inputs.shape)
            embedded = torch.cat([embedded, embeddirs_fn(torch.reshape(input_dirs, [-1, input_dirs.shape[-1]]))], -1)
        outputs_flat = nerf_utils.batchify(fn, netchunk)(embedded)
        return torch.reshape(outputs_flat, list(inputs.shape[:-1]) + [outputs_flat.shape[-1]])

    def _sample_points(self, z_vals_mid, weights, perturb, pytest, rays_d, rays_o, n_importance=None):
        from .run_nerf_helpers import sample_pdf

        if n_importance is None:
            n_importance = self.N_importance
        z_samples = sample_pdf(z_vals_mid, weights[..., 1:-1], n_importance, det=(perturb == 0.0), pytest=pytest)
        z_samples = z_samples.detach()
        return z_samples, ops.points_along_rays(rays_o, rays_d, z_samples)

    def sample_coarse_points(self, near, far, perturb, N_rays, N_samples, viewdirs, network_fn, network_query_fn,
                             rays_o, rays_d, raw_noise_std, white_bkgd, pytest, lindisp, **kwargs):
        """9-tuple in the reference's order (Trainer.py:579-649)."""
        rgb_map = disp_map = acc_map = depth_map = alphas_map = raw = weights = z_vals = None
        if N_samples > 0:
            t_rand = None
            if perturb > 0.0:
                if pytest:
                    np.random.seed(0)
                    t_rand = torch.tensor(np.random.rand(N_rays, N_samples), dtype=torch.float32, device=rays_o.device)
                else:
                    t_rand = torch.rand([N_rays, N_samples], device=rays_o.device)
            z_vals = ops.coarse_z(near, far, N_samples, lindisp, t_rand)
            pts = ops.points_along_rays(rays_o, rays_d, z_vals)
            raw = network_query_fn(pts, viewdirs, network_fn)
            rgb_map, disp_map, acc_map, depth_map, density, alphas, weights = self.raw2outputs(
                raw, z_vals, rays_d, raw_noise_std, white_bkgd, pytest=pytest)
        return rgb_map, disp_map, acc_map, weights, depth_map, z_vals, weights, raw, alphas_map

    def sample_fine_points(self, z_vals, weights, perturb, pytest, rays_d, rays_o, rgb_map, disp_map, acc_map,
                           network_fn, network_fine, network_query_fn, viewdirs, raw_noise_std, white_bkgd):
        """12-tuple in the reference's order (Trainer.py:651-710)."""
        rgb_map_0 = disp_map_0 = acc_map_0 = raw = None
        pts = density = alphas = None
        if self.N_importance > 0:
            rgb_map_0, disp_map_0, acc_map_0 = rgb_map, disp_map, acc_map
            u = None
            if perturb != 0.0:
                if pytest:
                    np.random.seed(0)
                    u = torch.tensor(np.random.rand(z_vals.shape[0], self.N_importance), dtype=torch.float32,
                                     device=z_vals.device)
                else:
                    u = torch.rand([z_vals.shape[0], self.N_importance], device=z_vals.device)
            # z_mid, sample_pdf(weights[1:-1]) and sort(cat[z, samples]) in one kernel
            z_vals = ops.importance_z(z_vals, weights, self.N_importance, u)
            pts = ops.points_along_rays(rays_o, rays_d, z_vals)
            run_fn = network_fn if network_fine is None else network_fine
            raw = network_query_fn(pts, viewdirs, run_fn)
            rgb_map, disp_map, acc_map, depth_map, density, alphas, weights = self.raw2outputs(
                raw, z_vals, rays_d, raw_noise_std, white_bkgd, pytest=pytest)
        return (rgb_map_0, disp_map_0, acc_map_0, rgb_map, disp_map, acc_map, raw, z_vals, pts, density, alphas,
                weights)

    def load_data(self):
        raise NotImplementedError("only the Blender loader is provided (trainers.BlenderTrainer)")

    def render(self, render_test, save_scene_data, images, i_test, render_poses, hwf, render_kwargs_test):
        """renderonly_{test|path}_{step:06d}/ with NNN.png, psnr.txt[, scene_data.pt] -- Trainer.py:181-230
        (no mp4; under device_video without render_test: rgb/NNN.png and disp/NNN.png through nerf_utils.write_video).  Under
        device_cloud also scene_cloud.pt and scene_cloud.ply of the same poses (nerf_utils.scene_cloud); under device_mesh also
        scene_mesh.ply, the isosurface of the field's density (nerf_utils.scene_mesh_shaded), without its small components where
        mesh_min_triangles or mesh_keep_largest is set and with per-vertex normals under mesh_normals."""
        with torch.no_grad():
            images = images[i_test] if render_test else None
            testsavedir = os.path.join(self.basedir, self.expname, "renderonly_{}_{:06d}".format(
                "test" if render_test else "path", self.global_step))
            os.makedirs(testsavedir, exist_ok=True)
            if self.device_cloud:
                H, W = int(hwf[0]), int(hwf[1])
                if self.render_factor != 0:
                    raise ValueError("device_cloud renders whole frames at the dataset's size: render_factor must be 0")
                cloud = nerf_utils.scene_cloud(render_poses, (H, W, hwf[2]), self.K, render_kwargs_test,
                                               min_weight=self.cloud_min_weight, max_points=self.cloud_points,
                                               savedir=testsavedir)
                print(f"scene cloud: {cloud['n_kept']} of {cloud['n_candidates']} samples with weight >= {self.cloud_min_weight}"
                      f", {cloud['pts'].shape[0]} written to {testsavedir}")
            if self.device_mesh:
                fine = render_kwargs_test.get("network_fine")
                mesh = nerf_utils.scene_mesh_simplified(fine if fine is not None else render_kwargs_test["network_fn"],
                                                        bound=self.mesh_bound, resolution=self.mesh_resolution,
                                                        threshold=self.mesh_threshold, savedir=testsavedir,
                                                        min_component_triangles=self.mesh_min_triangles,
                                                        keep_largest=self.mesh_keep_largest, normals=self.mesh_normals,
                                                        colour_view=self.mesh_colour_view, simplify=self.mesh_simplify)
                filtered = ""
                if "n_components" in mesh:
                    filtered = (f"; {mesh['n_kept_components']} of {mesh['n_components']} components kept, "
                                f"{mesh['n_dropped_triangles']} triangles dropped")
                if "normals" in mesh:
                    filtered += f"; normals, {mesh['n_degenerate_normals']} degenerate"
                if "n_clusters" in mesh:
                    filtered += (f"; simplified from {mesh['n_input_faces']} triangles on {mesh['n_input_vertices']} vertices, "
                                 f"{mesh['n_duplicate']} duplicates dropped")
                print(f"scene mesh: {mesh['faces'].shape[0]} triangles on {mesh['vertices'].shape[0]} vertices at density "
                      f"{self.mesh_threshold} ({mesh['n_skipped']} cells skipped{filtered}), written to {testsavedir}")
                if self.device_mesh_eval:
                    if not render_test or self.render_factor != 0:
                        raise ValueError("device_mesh_eval scores the mesh against the held-out photographs at the dataset's "
                                         "size: it needs render_test and render_factor 0")
                    ds, ids = self._ray_dataset, i_test
                    if ds is None:      # called on its own: the test views alone go to the device
                        ds, ids = ops.ray_dataset(np.asarray(images, dtype=np.float32), render_poses, self.K, [0]), range(len(i_test))
                    scored = nerf_utils.score_mesh_views(ds, ids, render_poses, hwf, self.K, mesh,
                                                         float(render_kwargs_test["near"]), render_kwargs=render_kwargs_test,
                                                         savedir=testsavedir,
                                                         background=1.0 if render_kwargs_test["white_bkgd"] else 0.0)
                    print(f"scene mesh from {len(scored['mesh_psnr'])} held-out views: PSNR {scored['avg_mesh_psnr']:.3f} dB, "
                          f"depth MSE against the field {scored['avg_depth_mse']:.3e}, silhouette IoU "
                          f"{scored['avg_silhouette_iou']:.4f}, {sum(scored['n_clipped'])} faces dropped at the near plane")
            if self.device_eval and render_test and self.render_factor == 0:
                ds, ids = self._ray_dataset, i_test
                if ds is None:          # called on its own: the test views alone go to the device
                    ds, ids = ops.ray_dataset(np.asarray(images, dtype=np.float32), render_poses, self.K, [0]), range(len(i_test))
                scores = nerf_utils.evaluate_views(ds, ids, render_poses, hwf, self.K, render_kwargs_test,
                                                   savedir=testsavedir, ssim=self.device_ssim, depth=self.device_depth,
                                                   frames=self.device_frames)
                return scores[1]
            if self.device_eval and self.device_video and not render_test and self.render_factor == 0:
                # the spiral as the i_video branch writes it: rgb/NNN.png and disp/NNN.png under the directory
                nerf_utils.write_video(render_poses, hwf, self.K, render_kwargs_test, os.path.join(testsavedir, ""),
                                       device="cuda" if self.device == "cuda" else self.device)
                return 0.0
            if self.device_eval and self.device_frames and not render_test and self.render_factor == 0:
                # poses without ground truth (the spiral): the same loop without scores; render_path's average is 0 there
                nerf_utils.write_views(render_poses, hwf, self.K, render_kwargs_test, testsavedir,
                                       device="cuda" if self.device == "cuda" else self.device)
                return 0.0
            _, _, avg_test_psnr = nerf_utils.render_path(
                render_poses, hwf, self.K, self.chunk, render_kwargs_test, step=self.global_step,
                save_scene_data=save_scene_data, gt_imgs=images, savedir=testsavedir, render_factor=self.render_factor)
        return avg_test_psnr

    def evaluate_testset(self, i, i_test, test_poses, hwf, render_kwargs_test):
        """device_eval: the i_test views into {basedir}/{expname}/testset_{i:06d}/psnr.txt (Trainer.log, Trainer.py:289-316,
        without its PNGs) -> their average PSNR; under device_ssim ssim.txt too -> (average PSNR, average SSIM); under
        device_depth depth.txt too, and (average sample MSE, average mean MSE) as the last element of the tuple.  While the
        field is frozen and the test perturb is 0 the field's depth maps of the first call serve the later ones."""
        savedir = os.path.join(self.basedir, self.expname, "testset_{:06d}".format(i))
        if not self.device_depth:
            scores = nerf_utils.evaluate_views(self._ray_dataset, i_test, test_poses, hwf, self.K, render_kwargs_test,
                                               savedir=savedir, ssim=self.device_ssim, frames=self.device_frames)
            return (scores[1], scores[3]) if self.device_ssim else scores[1]
        keep = bool(self.train_depth_net_only) and float(render_kwargs_test.get("perturb", 0.0)) == 0.0
        scores = nerf_utils.evaluate_views(self._ray_dataset, i_test, test_poses, hwf, self.K, render_kwargs_test,
                                           savedir=savedir, ssim=self.device_ssim, depth=True,
                                           field_depths=self._field_depths if keep else None, return_depths=keep,
                                           frames=self.device_frames)
        if keep and self._field_depths is None:
            self._field_depths = [max_z for _z, _mean, max_z in scores[-1]]
        averages = scores[1:4 if self.device_ssim else 2:2]           # (PSNR[, SSIM]): every second element is an average
        _sample_mses, avg_sample_mse, _mean_mses, avg_mean_mse = scores[len(averages) * 2:len(averages) * 2 + 4]
        return averages + ((avg_sample_mse, avg_mean_mse),)

    def train(self, N_iters=200000 + 1):
        """Trainer.train (Trainer.py:712-787): load data, build / reload the networks; render_only: render the test
        (or spiral) poses and return the average PSNR; otherwise the DepthNet optimisation loop (random ray batches from
        one image, or -- use_batching -- from the shuffled rays of all training images), checkpoints every i_weights.
        With device_eval the i_test views are scored every i_testset iterations (evaluate_testset); with device_video the
        spiral is written every i_video iterations (nerf_utils.write_video)."""
        hwf, poses, i_test, i_val, i_train, images, render_poses = self.load_data()
        dev = "cuda" if self.device == "cuda" else self.device
        if self.render_test:
            render_poses = torch.tensor(np.array(poses[i_test])).to(dev)
        hwf = self.cast_intrinsics_to_right_types(hwf=hwf)
        test_poses = None
        if self.device_eval and dev == "cuda":
            # all images are in the dataset (device_batches' own, when it uploads one), so the test views are too
            self.ray_dataset(i_train, np.asarray(images, dtype=np.float32), poses)
            test_poses = np.asarray(poses, dtype=np.float32)[np.asarray(i_test)]
        os.makedirs(os.path.join(self.basedir, self.expname), exist_ok=True)
        optimizer, sampling_optimizer, render_kwargs_train, render_kwargs_test = self.create_nerf_model()
        if self.train_depth_net_only:
            for k in ("network_fn", "network_fine"):
                if render_kwargs_train[k] is not None:
                    utils.freeze_model(render_kwargs_train[k])
        if self.render_only:
            return self.render(self.render_test, self.save_scene_data, images, i_test, render_poses, hwf,
                               render_kwargs_test)
        images, poses, rays_rgb, i_batch = self.prepare_raybatch_tensor_if_batching_random_rays(poses, images, i_train)
        psnr = None
        # hip_graph (not in the reference; default on): the step is captured as one hipGraph after two eager steps
        graphed = self.hip_graph and dev == "cuda" and hasattr(sampling_optimizer, "use_device_step")
        # device_batches='draw' under the graphed step: the draw is the first node of the captured graph
        in_graph = graphed and self.device_batches == "draw"
        source = self.draw_source(i_train, images, poses, self.start + 1) if in_graph else None
        step = (self.graphed_optimization_loop(sampling_optimizer, render_kwargs_train, batch_source=source) if graphed
                else lambda rays, it, tgt: self.core_optimization_loop(sampling_optimizer, render_kwargs_train, rays, it, tgt))
        for i in range(self.start + 1, N_iters):
            batch_rays = target_s = None
            if not in_graph:
                rays_rgb, i_batch, batch_rays, target_s = self.sample_random_ray_batch(rays_rgb, i_batch, i_train, images,
                                                                                       poses, i)
            loss, depth_net_loss, psnr, _ = step(batch_rays, i, target_s)
            self.update_learning_rate(optimizer)
            if i % self.i_print == 0:
                print(f"[TRAIN] Iter: {i} Loss: {float(loss)} depth_net_loss: {float(depth_net_loss)} "
                      f"PSNR: {float(psnr)}")
                # the reference's progress line, appended to {basedir}/{expname}/psnr.txt (Trainer.py:378-392; wandb is
                # out of scope)
                info = f"Iter: {i} Loss: {float(loss)}, Depth Net Loss: {float(depth_net_loss)}, PSNR: {float(psnr):.5f}"
                with open(os.path.join(self.basedir, self.expname, "psnr.txt"), "a") as file:
                    file.write(f"{info}\n")
            if test_poses is not None and self.i_testset and i % self.i_testset == 0 and i > 0:
                with torch.no_grad():
                    avg = self.evaluate_testset(i, i_test, test_poses, hwf, render_kwargs_test)
                if self.device_depth:
                    avg, (avg_sample_mse, avg_mean_mse) = avg[:-1], avg[-1]
                    avg = avg if self.device_ssim else avg[0]
                    print(f"[TRAIN] Iter: {i} test depth MSE: {avg_sample_mse} mean MSE: {avg_mean_mse}")
                if self.device_ssim:
                    avg, avg_ssim = avg
                    print(f"[TRAIN] Iter: {i} test SSIM: {avg_ssim}")
                print(f"[TRAIN] Iter: {i} test PSNR: {avg}")
            if self.device_video and dev == "cuda" and self.i_video and i % self.i_video == 0 and i > 0:
                moviebase = os.path.join(self.basedir, self.expname, "{}_spiral_{:06d}_".format(self.expname, i))
                video = nerf_utils.write_video(render_poses, hwf, self.K, render_kwargs_test, moviebase, device=dev)
                print(f"[TRAIN] Iter: {i} spiral of {video['n_views']} views written to {moviebase}rgb/ and {moviebase}disp/ "
                      f"(max disparity {video['disp_max']}{', NaN pixels written as 0' if video['has_nan'] else ''})")
            if i % self.i_weights == 0:
                path = os.path.join(self.basedir, self.expname, "{:06d}.tar".format(i))
                utils.save_state(self.global_step, render_kwargs_train["network_fn"],
                                 render_kwargs_train["network_fine"], optimizer, render_kwargs_train["depth_network"],
                                 sampling_optimizer, path)
            self.global_step += 1
        return psnr

    def update_learning_rate(self, optimizer):
        """Trainer.py:546-551 (decays the NeRF optimiser's lr, which never steps when train_depth_net_only)."""
        new_lrate = self.lrate * (0.1 ** (self.global_step / (self.lrate_decay * 1000)))
        for param_group in optimizer.param_groups:
            param_group["lr"] = new_lrate

    def prepare_raybatch_tensor_if_batching_random_rays(self, poses, images, i_train):
        """(images, poses, rays_rgb, i_batch) -- Trainer.py:232-269.  With use_batching the rays of every TRAINING image
        are generated once (ns_get_rays, on the device), joined with their pixel colours into rays_rgb
        [(n_train H W), ro+rd+rgb, 3] and shuffled with numpy's generator: the reference calls np.random.shuffle on the
        array itself, which draws the same permutation as shuffling an index vector of that length."""
        dev = "cuda" if self.device == "cuda" else self.device
        poses_t = torch.tensor(np.asarray(poses), dtype=torch.float32).to(dev)
        if not self.use_batching:
            return images, poses_t, None, None
        if self.device_batches == "draw":         # the draw kernel walks the epoch itself: no rays_rgb, no permutation
            return images, poses_t, None, 0
        rows = []
        for img_i in i_train:
            o, d, _ = ops.get_rays(self.H, self.W, self.K, poses_t[img_i, :3, :4], device=dev)
            rgb = torch.tensor(np.asarray(images[img_i]), dtype=torch.float32, device=o.device).reshape(-1, 3)
            rows.append(torch.stack([o, d, rgb[:, :3]], 1))            # [H*W, 3, 3]
        rays_rgb = torch.cat(rows, 0)
        perm = np.arange(rays_rgb.shape[0])
        np.random.shuffle(perm)
        rays_rgb = rays_rgb[torch.from_numpy(perm).to(rays_rgb.device)]
        images = torch.tensor(np.asarray(images), dtype=torch.float32).to(dev)
        return images, poses_t, rays_rgb, 0

    def sample_random_ray_batch(self, rays_rgb, i_batch, i_train, images, poses, i):
        """use_batching: the next N_rand rows of the shuffled rays_rgb, reshuffled (torch.randperm, as the reference)
        after an epoch; otherwise N_rand random pixels of one random training image -- Trainer.py:400-475.  With
        device_batches the batch comes from the device-resident dataset (see _device_batch)."""
        if self.device_batches:
            return (rays_rgb, i_batch) + self._device_batch(i_train, images, poses, i)
        if self.use_batching:
            batch = torch.transpose(rays_rgb[i_batch : i_batch + self.N_rand], 0, 1)     # [ro+rd+rgb, B, 3]
            batch_rays, target_s = batch[:2], batch[2]
            i_batch += self.N_rand
            if i_batch >= rays_rgb.shape[0]:
                print("Shuffle data after an epoch!")
                rays_rgb = rays_rgb[torch.randperm(rays_rgb.shape[0], device=rays_rgb.device)]
                i_batch = 0
            return rays_rgb, i_batch, batch_rays, target_s
        img_i = 42 if self.single_image else np.random.choice(i_train)
        target = torch.tensor(np.asarray(images[img_i]), dtype=torch.float32)
        pose = poses[img_i, :3, :4]
        self.c2w = pose.clone().detach()
        rays_o, rays_d, _ = ops.get_rays(self.H, self.W, self.K, self.c2w)     # [H*W, 3]
        if i < self.precrop_iters:
            dH, dW = int(self.H // 2 * self.precrop_frac), int(self.W // 2 * self.precrop_frac)
            rows = torch.arange(self.H // 2 - dH, self.H // 2 + dH)
            cols = torch.arange(self.W // 2 - dW, self.W // 2 + dW)
        else:
            rows, cols = torch.arange(self.H), torch.arange(self.W)
        coords = torch.stack(torch.meshgrid(rows, cols, indexing="ij"), -1).reshape(-1, 2)
        if self.single_ray:
            select = np.array([91])
        else:
            select = np.random.choice(coords.shape[0], size=[self.N_rand], replace=False)
        sel = coords[select].long()
        flat = (sel[:, 0] * self.W + sel[:, 1]).to(rays_o.device)
        batch_rays = torch.stack([rays_o[flat], rays_d[flat]], 0)
        target_s = target[sel[:, 0], sel[:, 1]].to(rays_o.device)
        return rays_rgb, i_batch, batch_rays, target_s

    def ray_dataset(self, i_train, images, poses):
        """The device-resident dataset of device_batches, uploaded at the first call."""
        if self._ray_dataset is None:
            from .ray_batches import DeviceRayDataset

            self._ray_dataset = DeviceRayDataset(images, poses, self.K, i_train, white_bkgd=False)
        return self._ray_dataset

    def draw_source(self, i_train, images, poses, first_step):
        """device_batches='draw': the batch source of this run (ray_batches.DrawBatchSource).  Its step counter lives on the
        device, starts at ``first_step`` and advances by one per batch; the pre-crop is its window, use_batching its scope."""
        if self._draw_source is None:
            from .ray_batches import DrawBatchSource, precrop_window

            ds = self.ray_dataset(i_train, images, poses)
            crop = precrop_window(self.H, self.W, self.precrop_frac)
            self._draw_source = DrawBatchSource(
                ds, self.N_rand, scope="all_images" if self.use_batching else "per_image", seed=self.batch_seed,
                first_step=first_step, window_fn=lambda it: crop if it < self.precrop_iters else None,
                train_idx=[42] if (self.single_image and not self.use_batching) else i_train)
        return self._draw_source

    def _device_batch(self, i_train, images, poses, i):
        """(batch_rays, target_s) of iteration ``i`` under device_batches.  'gather' makes the np.random.choice calls of the
        default path in the same order, maps the drawn window positions to full-frame pixels on the host and uploads only
        those indices: the default path's batch bit for bit.  'draw' asks the draw source."""
        if self.device_batches == "draw":
            return self.draw_source(i_train, images, poses, i)(i)
        from .ray_batches import full_window, precrop_window

        ds = self.ray_dataset(i_train, images, poses)
        img_i = 42 if self.single_image else np.random.choice(i_train)
        self.c2w = poses[img_i, :3, :4].clone().detach()
        r0, r1, c0, c1 = (precrop_window(self.H, self.W, self.precrop_frac) if i < self.precrop_iters
                          else full_window(self.H, self.W))
        cols = c1 - c0
        if self.single_ray:
            select = np.array([91])
        else:
            select = np.random.choice((r1 - r0) * cols, size=[self.N_rand], replace=False)
        return ds.gather(int(img_i), (r0 + select // cols) * self.W + c0 + select % cols)

    def _optimization_step(self, sampling_optimizer, render_kwargs_train, batch_rays, i, target_s, **render_extra):
        """forward + two losses + backward + update; (img_loss, depth_net_loss) as device scalars."""
        from .run_nerf_helpers import img2mse

        rgb, _disp, extras = nerf_utils.render(self.H, self.W, self.K, chunk=self.chunk, rays=batch_rays,
                                               verbose=i < 10, retraw=True, **render_kwargs_train, **render_extra)
        sampling_optimizer.zero_grad()
        img_loss = img2mse(rgb, target_s)
        depth_net_loss = torch.nn.functional.mse_loss(extras["depth_net_z_vals"], extras["max_z_vals"])
        (depth_net_loss + img_loss).backward()
        sampling_optimizer.step()
        return img_loss.detach(), depth_net_loss.detach()

    def core_optimization_loop(self, sampling_optimizer, render_kwargs_train, batch_rays, i, target_s):
        """One DepthNet update: (loss, depth_net_loss, psnr, psnr0) -- Trainer.py:506-544.  The two backward
        calls of the reference accumulate into the same .grad; one backward of the sum is identical."""
        from .run_nerf_helpers import mse2psnr

        img_loss, depth_net_loss = self._optimization_step(sampling_optimizer, render_kwargs_train, batch_rays, i, target_s)
        psnr = mse2psnr(img_loss)
        render_kwargs_train["depth_network"].repack()
        return img_loss, depth_net_loss, psnr, None

    def graphed_optimization_loop(self, sampling_optimizer, render_kwargs_train, batch_source=None):
        """core_optimization_loop as ONE hipGraph replay per step (see GraphedDepthNetStep): same arguments after the
        first two, same return value, same updates bit for bit.  ``batch_source``: a ray_batches.DrawBatchSource whose draw
        becomes part of the graph."""
        return GraphedDepthNetStep(self, sampling_optimizer, render_kwargs_train, batch_source=batch_source)


class GraphedDepthNetStep:
    """Trainer.core_optimization_loop (Trainer.py:506-544) captured as one hipGraph.

    A training step at the reference's batch size (N_rand = 1024 rays) is ~450 small kernels: the frozen field's
    64 + 128 vanilla pass, the DepthNet forward / backward layer by layer, the NeRF input gradient, 82 Adam updates.
    Eagerly the step is bound by the host side of those launches; captured once (torch.cuda.CUDAGraph = hipGraph on
    ROCm) and replayed, the host issues ONE launch per step.  What makes the step capturable: HipAdam's device-resident
    step counter / learning rate (ns_adam_step_dev), render_rays without its three host copies (nothing in the step
    reads them), and fixed batch shapes.  With ``fused_step`` in the render kwargs the step's two one-call renderers work in
    workspaces this object owns and on f16x3 streams it keeps alive.  The first ``warmup`` calls run eagerly (they are real steps and warm every
    lazily-built cache); the next call captures and replays.  A batch of another shape runs eagerly.

    Call: ``step(batch_rays, i, target_s) -> (img_loss, depth_net_loss, psnr, None)`` like core_optimization_loop.

    ``batch_source`` (a ray_batches.DrawBatchSource, optional): the batches are drawn on the device and ``batch_rays`` /
    ``target_s`` of the call are ignored (pass None).  Eager steps draw one batch each; the capture records the draw launch and
    its counter increment in front of the step, writing into the graph's own ray and target buffers, so a replay copies nothing
    in.  The host only rewrites the source's window when it changes (``batch_source.begin(i)``)."""

    def __init__(self, trainer, sampling_optimizer, render_kwargs_train, warmup: int = 2, batch_source=None):
        self.tr, self.opt, self.kw, self.warmup = trainer, sampling_optimizer, render_kwargs_train, warmup
        self.source = batch_source
        self.calls, self.graph, self.shape = 0, None, None
        self.opt.use_device_step()
        # everything the captured kernels point into must outlive the graph: packed weight streams of the frozen networks
        nets = [n for n in (render_kwargs_train.get("network_fn"), render_kwargs_train.get("network_fine")) if n is not None]
        self._keep = [n.packed() for n in nets]
        self._extra = {"_skip_host_copies": True}
        if render_kwargs_train.get("fused_step", False):
            # the fused step's two one-call renderers: their f16x3 streams, and workspaces of this object's own (the module's
            # shared one may be regrown, i.e. freed, by any other render call between two replays)
            field = nerf_utils._fused_step_field(nets[-1], render_kwargs_train.get("network_query_fn"), trainer, True)
            if field is not None:
                self._keep.append(field)
            self._extra["_workspaces"] = {"vanilla": ops.RenderWorkspace(), "tangent": ops.RenderWorkspace()}

    def _eager(self, batch_rays, i, target_s):
        from .run_nerf_helpers import mse2psnr

        img_loss, dn_loss = self.tr._optimization_step(self.opt, self.kw, batch_rays, i, target_s, **self._extra)
        self.kw["depth_network"].repack()
        return img_loss, dn_loss, mse2psnr(img_loss), None

    def _capture(self, batch_rays, target_s):
        if self.source is not None:
            self.rays, self.target = self.source.empty_batch()
        else:
            self.rays, self.target = batch_rays.clone(), target_s.clone()
        self.shape = (tuple(self.rays.shape), tuple(self.target.shape))
        self.opt.zero_grad(set_to_none=True)           # backward inside the capture allocates the grads in the graph's pool
        # an evaluation since the last step (evaluate_testset) has packed the DepthNet again: the training forward drops that
        # stream, and freeing device memory inside a capture invalidates it -- drop it here
        self.kw["depth_network"].repack()
        torch.cuda.synchronize()
        self.opt.claim_capture_table()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            if self.source is not None:
                self.source.launch(self.rays, self.target)
            self.img_loss, self.dn_loss = self.tr._optimization_step(self.opt, self.kw, self.rays, 1 << 30, self.target,
                                                                     **self._extra)

    def __call__(self, batch_rays, i, target_s):
        from .run_nerf_helpers import mse2psnr

        self.calls += 1
        if self.source is not None:
            if self.calls <= self.warmup:
                batch_rays, target_s = self.source(i)
                return self._eager(batch_rays, i, target_s)
            self.source.begin(i)
        elif self.calls <= self.warmup or (self.shape is not None and
                                           self.shape != (tuple(batch_rays.shape), tuple(target_s.shape))):
            return self._eager(batch_rays, i, target_s)
        if self.graph is None:
            self._capture(batch_rays, target_s)        # records, does not execute
        if self.source is None:
            self.rays.copy_(batch_rays)
            self.target.copy_(target_s)
        self.opt.sync_device_lr()
        self.graph.replay()
        self.opt.note_replayed_step()
        self.kw["depth_network"].repack()
        return self.img_loss, self.dn_loss, mse2psnr(self.img_loss), None


class FieldFitter:
    """Fit the radiance field itself on the HIP kernels: the vanilla objective the reference's forward implies
    (sample_as_in_NeRF, nerf_utils.py:497-611) -- coarse depths, coarse field, compositing, importance sampling on the detached
    weights, fine field on the Nc + Nf depths, compositing, loss = img2mse(rgb) + img2mse(rgb0) -- with the weight gradients of
    autograd.NerfFunction (ns_gemm_wgrad), autograd.Composite and HipAdam over both networks' parameters.

    ``network_fine=None``: the coarse-only objective when N_importance == 0, else the coarse network runs both passes (as
    sample_fine_points does).  One module passed as both networks accumulates both passes' gradients into the same tensors.
    ``near`` / ``far``: the ray bounds (Blender's 2 / 6).  ``gemm_engine``: "tile" runs the layer forwards and the grad-input
    products of both passes on ns_gemm_fused, "tall" on ns_gemm_tall (autograd.nerf_forward_train's ``engine``)."""

    def __init__(self, network_fn, network_fine=None, N_samples=64, N_importance=128, lrate=5e-4, lrate_decay=250,
                 white_bkgd=True, raw_noise_std=0.0, perturb=1.0, lindisp=False, near=2.0, far=6.0, gemm_engine="tile"):
        from .autograd import GEMM_ENGINES, HipAdam

        if gemm_engine not in GEMM_ENGINES:
            raise ValueError(f"gemm_engine must be one of {GEMM_ENGINES}, got {gemm_engine!r}")
        self.gemm_engine = gemm_engine
        self.network_fn, self.network_fine = network_fn, network_fine
        self.N_samples, self.N_importance = int(N_samples), int(N_importance)
        self.lrate, self.lrate_decay = float(lrate), lrate_decay
        self.white_bkgd, self.raw_noise_std = bool(white_bkgd), float(raw_noise_std)
        self.perturb, self.lindisp = float(perturb), bool(lindisp)
        self.near, self.far = float(near), float(far)
        params, seen = [], set()
        for net in (network_fn, network_fine):
            for p in ([] if net is None else net.parameters()):
                if id(p) not in seen:
                    seen.add(id(p))
                    params.append(p)
        self.optimizer = HipAdam(params=params, lr=self.lrate, betas=(0.9, 0.999))
        self.optimizer.use_device_step()           # one launch for all parameter tensors
        self.global_step = 0

    def _noise(self, shape, device):
        if self.raw_noise_std > 0.0:
            return torch.randn(shape, device=device) * self.raw_noise_std
        return None

    def forward_loss(self, batch_rays, target, t_rand=None, u=None):
        """(loss, info) of one batch: batch_rays [2,B,3] (origins, directions), target [B,3].  info: img_loss / img_loss0 (the
        fine / coarse image losses, detached), rgb / rgb0, z0 [B,Nc] and z [B,Nc+Nf].  ``t_rand`` [B,Nc] / ``u`` [B,Nf]: the
        stratified and importance draws (drawn here when perturb > 0 and not given)."""
        from .autograd import composite, nerf_forward_train
        from .run_nerf_helpers import img2mse

        o, d = ops._dev(batch_rays[0], "rays_o"), ops._dev(batch_rays[1], "rays_d")
        target = ops._dev(target, "target")
        B, dev = o.shape[0], o.device
        viewdirs = d / torch.norm(d, dim=-1, keepdim=True)
        near = torch.full((B,), self.near, dtype=torch.float32, device=dev)
        far = torch.full((B,), self.far, dtype=torch.float32, device=dev)
        if t_rand is None and self.perturb > 0.0:
            t_rand = torch.rand((B, self.N_samples), device=dev)
        z0 = ops.coarse_z(near, far, self.N_samples, self.lindisp, t_rand)
        raw0 = nerf_forward_train(self.network_fn, ops.points_along_rays(o, d, z0), viewdirs, engine=self.gemm_engine)
        rgb0, _, _, _, _, w0 = composite(raw0, z0, d, self._noise(z0.shape, dev), self.white_bkgd)
        img_loss0 = img2mse(rgb0, target)
        info = dict(z0=z0, rgb0=rgb0, img_loss0=img_loss0.detach())
        if self.N_importance <= 0:
            info.update(z=z0, rgb=rgb0, img_loss=img_loss0.detach())
            return img_loss0, info
        if u is None and self.perturb > 0.0:
            u = torch.rand((B, self.N_importance), device=dev)
        z = ops.importance_z(z0, w0.detach(), self.N_importance, u)       # the reference detaches z_samples (Trainer.py:572)
        fine = self.network_fn if self.network_fine is None else self.network_fine
        raw = nerf_forward_train(fine, ops.points_along_rays(o, d, z), viewdirs, engine=self.gemm_engine)
        rgb, _, _, _, _, _ = composite(raw, z, d, self._noise(z.shape, dev), self.white_bkgd)
        img_loss = img2mse(rgb, target)
        info.update(z=z, rgb=rgb, img_loss=img_loss.detach())
        return img_loss + img_loss0, info

    def step(self, batch_rays, target):
        """One update of both networks: (loss, psnr, psnr0) as device scalars (psnr0: the coarse pass's, None without a fine
        pass), then the reference's learning-rate decay (Trainer.py:546-551)."""
        from .run_nerf_helpers import mse2psnr

        loss, info = self.forward_loss(batch_rays, target)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        new_lrate = self.lrate * (0.1 ** (self.global_step / (self.lrate_decay * 1000)))
        for group in self.optimizer.param_groups:
            group["lr"] = new_lrate
        self.global_step += 1
        psnr0 = mse2psnr(info["img_loss0"]) if self.N_importance > 0 else None
        return loss.detach(), mse2psnr(info["img_loss"]), psnr0

    def repack(self):
        """Drop the packed inference streams of both networks: the next render packs the fitted weights."""
        for net in (self.network_fn, self.network_fine):
            if net is not None:
                net.repack()

    def save(self, path):
        """A checkpoint in the reference's .tar layout (utils.save_state): network_fn_state_dict, network_fine_state_dict,
        optimizer_state_dict, global_step."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        utils.save_state(self.global_step, self.network_fn, self.network_fine, self.optimizer, None, None, path)

    def _blender_source(self, split, N_rand, device_batches=False, batch_seed=0, want_dataset=False):
        """Batches of N_rand rays of a Blender split as Trainer.sample_random_ray_batch draws them (one random training image
        per batch).  ``split``: load_blender_data's (images, poses, render_poses, hwf, i_split), or a dict with images
        [n,H,W,3|4], poses, hwf and i_train.  ``device_batches``: Trainer's option -- the images (all their channels) and poses
        go to the device once, and the background blend happens per drawn pixel in the batch kernel.  ``want_dataset``: upload
        that dataset whatever makes the batches (fit's held-out evaluation scores against it); the returned callable carries
        it and what an evaluation needs beside it as ``dataset`` / ``poses`` / ``hwf`` / ``K`` / ``i_test``."""
        if isinstance(split, dict):
            images, poses, hwf, i_train = split["images"], split["poses"], split["hwf"], split["i_train"]
            i_test = split.get("i_test")
        else:
            images, poses, _render_poses, hwf, i_split = split
            i_train, i_test = i_split[0], i_split[2]
        images = np.asarray(images)
        tr = Trainer(dataset_type="blender", basedir="", expname="", no_batching=True, datadir="", N_rand=N_rand, device="cuda",
                     device_batches=device_batches, batch_seed=batch_seed)
        tr.cast_intrinsics_to_right_types(hwf)
        poses_t = torch.tensor(np.asarray(poses), dtype=torch.float32).to("cuda")
        dataset = None
        if device_batches or want_dataset:
            from .ray_batches import DeviceRayDataset

            dataset = DeviceRayDataset(images.astype(np.float32, copy=False), poses_t, tr.K, i_train,
                                       white_bkgd=self.white_bkgd)
        if device_batches:
            tr._ray_dataset = dataset
        elif images.shape[-1] == 4:
            images = (images[..., :3] * images[..., -1:] + (1.0 - images[..., -1:])) if self.white_bkgd else images[..., :3]

        def draw(i):
            _, _, batch_rays, target = tr.sample_random_ray_batch(None, None, i_train, images, poses_t, i)
            return batch_rays, target

        draw.dataset, draw.poses, draw.hwf, draw.K, draw.i_test = dataset, np.asarray(poses, dtype=np.float32), hwf, tr.K, i_test
        return draw

    def evaluate_views(self, dataset, image_ids, poses, hwf, K, savedir=None, return_frames=False, ssim=False,
                       frames=False):
        """The PSNR of held-out views on the device (nerf_utils.score_views): every view through the hierarchical renderer in
        one call, with this fitter's N_samples / N_importance, white_bkgd / lindisp / bounds and perturb 0, scored against
        ``dataset``'s images.  Call repack() first if the weights have moved.  -> (psnr per view, their mean[, frames]); with
        ``ssim`` (psnr per view, their mean, ssim per view, their mean[, frames]) and ssim.txt beside psnr.txt.  ``frames``
        (needs ``savedir``): the views also as NNN.png beside psnr.txt (nerf_utils.FrameWriter)."""
        render_frame = nerf_utils.hierarchical_frame_renderer(
            self.network_fn, self.network_fine, int(hwf[0]), int(hwf[1]), K, self.N_samples, self.N_importance, self.lindisp,
            self.white_bkgd, self.near, self.far, perturb=0.0, device=dataset.device)
        return nerf_utils.score_views(dataset, image_ids, poses, render_frame, savedir=savedir, return_frames=return_frames,
                                      ssim=ssim, frames=frames)

    def fit(self, rays_source, n_iters, N_rand=1024, basedir=None, expname="field", i_weights=10000, i_print=100,
            evaluate=None, device_batches=False, batch_seed=0, i_testset=0, test_ids=None, test_ssim=False,
            test_frames=False):
        """``n_iters`` steps on batches from ``rays_source``: a loaded Blender split (see _blender_source) or a callable
        returning (batch_rays [2,B,3], target [B,3]).  With ``basedir`` a checkpoint {basedir}/{expname}/{step:06d}.tar is written
        every ``i_weights`` steps and at the end.  ``evaluate(fitter)``, if given, runs at every ``i_print`` steps after repack().
        Both networks are repacked before the call returns.  ``device_batches`` / ``batch_seed``: how a Blender split's batches
        are made (_blender_source).  ``i_testset`` > 0 (a Blender split only): every ``i_testset`` steps and at the end the views
        ``test_ids`` (default: the split's i_test) are scored on the device (``evaluate_views``), "[FIT] Iter: .. test PSNR:
        .." is printed and, with ``basedir``, {basedir}/{expname}/testset_{step:06d}/psnr.txt written; ``test_ssim`` adds
        " SSIM: .." to that line and ssim.txt to that directory, ``test_frames`` (needs ``basedir``) the views as NNN.png.
        Returns the last (loss, psnr, psnr0)."""
        i_testset = int(i_testset or 0)
        if test_frames and i_testset > 0 and basedir is None:
            raise ValueError("test_frames writes the test views under basedir: basedir is required")
        if callable(rays_source):
            if device_batches:
                raise ValueError("device_batches applies to a Blender split, not to a callable ray source")
            if i_testset > 0:
                raise ValueError("i_testset scores a Blender split's held-out views, a callable ray source has none")
            draw = lambda i: rays_source()  # noqa: E731
        else:
            draw = self._blender_source(rays_source, N_rand, device_batches=device_batches, batch_seed=batch_seed,
                                        want_dataset=i_testset > 0)
        if i_testset > 0:
            test_ids = draw.i_test if test_ids is None else test_ids
            if test_ids is None or len(test_ids) == 0:
                raise ValueError("i_testset: the split names no test views (i_test) and test_ids is not given")
            test_ids = np.asarray(test_ids, dtype=np.int64).reshape(-1)

        def score():
            self.repack()
            savedir = None if basedir is None else os.path.join(basedir, expname, "testset_{:06d}".format(self.global_step))
            scores = self.evaluate_views(draw.dataset, test_ids, draw.poses[test_ids], draw.hwf, draw.K, savedir=savedir,
                                         ssim=bool(test_ssim), frames=bool(test_frames))
            print(f"[FIT] Iter: {self.global_step} test PSNR: {scores[1]}" + (f" SSIM: {scores[3]}" if test_ssim else ""))

        out = None
        for i in range(1, int(n_iters) + 1):
            batch_rays, target = draw(i)
            out = self.step(batch_rays, target)
            if i_testset > 0 and (i % i_testset == 0 or i == int(n_iters)):
                score()
            if i_print and i % i_print == 0:
                print(f"[FIT] Iter: {self.global_step} Loss: {float(out[0])} PSNR: {float(out[1])}")
                if evaluate is not None:
                    self.repack()
                    evaluate(self)
            if basedir is not None and (i % i_weights == 0 or i == int(n_iters)):
                self.save(os.path.join(basedir, expname, "{:06d}.tar".format(self.global_step)))
        self.repack()
        return out


class BlenderTrainer(Trainer):
    def __init__(self, half_res, white_bkgd, testskip=8, near=2.0, far=6.0, **kwargs):
        self.half_res, self.testskip, self.white_bkgd = half_res, testskip, white_bkgd
        self.near, self.far = near, far
        super().__init__(**kwargs)

    def load_data(self):
        """trainers/Blender.py:19-32."""
        from .load_blender import load_blender_data

        images, poses, render_poses, hwf, i_split = load_blender_data(self.datadir, self.half_res, self.testskip)
        i_train, i_val, i_test = i_split
        if self.white_bkgd:
            images = images[..., :3] * images[..., -1:] + (1.0 - images[..., -1:])
        else:
            images = images[..., :3]
        return hwf, poses, i_test, i_val, i_train, images, render_poses.clone().detach()


class DepthNetTrainer(BlenderTrainer):
    """Constructor and operator signatures of sampling_trainer.py:17-52,153-230."""

    def __init__(self, distance=None, sampling_mode=None, n_depth_samples=None,
                 depth_net_path: Optional[str] = None, n_layers: int = 6, layer_width: int = 256,
                 sphere_radius: float = 2.0, fused_step: bool = False, **kwargs):
        # fused_step (not in the reference; default off): render_rays runs the DepthNet branch of the training step as one
        # kernel and the target pass as one call (nerf_utils.render_rays)
        self.fused_step = bool(fused_step)
        self.n_layers, self.layer_width = n_layers, layer_width
        self.depth_net_path, self.sphere_radius = depth_net_path, sphere_radius
        self.distance, self.n_depth_samples, self.sampling_mode = distance, n_depth_samples, sampling_mode
        super().__init__(**kwargs)

    def create_nerf_model(self):
        """(optimizer, sampling_optimizer, render_kwargs_train, render_kwargs_test) -- sampling_trainer.py:54-122.

        Checkpoints in the reference's .tar format are read with torch.load(weights_only=True).
        """
        render_kwargs_train, render_kwargs_test, start, grad_vars, optimizer = nerf_utils.create_nerf(self, NeRF)
        bds = {"near": self.near, "far": self.far}
        render_kwargs_train.update(bds)
        render_kwargs_test.update(bds)
        sizes = [self.layer_width for _ in range(self.n_layers)]
        dev = "cuda" if self.device == "cuda" else self.device
        depth_network = DepthNet(hidden_sizes=sizes, cat_hidden_sizes=list(sizes), sphere_radius=self.sphere_radius).to(dev)
        from .autograd import HipAdam

        sampling_optimizer = HipAdam(params=list(depth_network.parameters()), lr=self.depth_net_lr)
        ckpts = []
        if self.depth_net_path is not None and self.depth_net_path != "None":
            ckpts = [self.depth_net_path]
        elif os.path.isdir(os.path.join(self.basedir, self.expname)):
            d = os.path.join(self.basedir, self.expname)
            ckpts = [os.path.join(d, f) for f in sorted(os.listdir(d)) if "tar" in f]
        start = None
        if len(ckpts) > 0 and not self.no_reload:
            ckpt = torch.load(ckpts[-1], weights_only=True, map_location=dev)
            start = ckpt["global_step"]
            utils.load_depth_network(depth_network, sampling_optimizer, ckpt)
        self.global_step = self.start = start if start is not None else 0
        for kw, mode in ((render_kwargs_train, "train"), (render_kwargs_test, "test")):
            kw["depth_network"] = depth_network
            kw["model_mode"] = mode
        if self.fused_step:
            render_kwargs_train["fused_step"] = True
        return optimizer, sampling_optimizer, render_kwargs_train, render_kwargs_test

    def save_rays_data(self, rays_o, pts, alpha):
        """{basedir}/{expname}/{expname}_{global_step}.safetensors holding origins / pts / alpha, the dump
        experiments/plot.py reads for its point-cloud plots (sampling_trainer.py:124-138)."""
        from safetensors.torch import save_file

        os.makedirs(os.path.join(self.basedir, self.expname), exist_ok=True)
        filename = os.path.join(self.basedir, self.expname, f"{self.expname}_{self.global_step}.safetensors")
        save_file({"origins": rays_o.detach().contiguous(), "pts": pts.detach().contiguous(),
                   "alpha": alpha.detach().contiguous()}, filename)
        return filename

    def raw2outputs(self, raw, z_vals, rays_d, raw_noise_std=0, white_bkgd=True, pytest=False, **kwargs):
        """7-tuple (rgb_map, disp_map, acc_map, depth_map, density, alphas, weights).

        Unknown keyword arguments are swallowed exactly like the reference does (its DepthNet-path
        callers pass the misspelled raw_noise= / white_bkdg=, nerf_utils.py:712-713,862-863).
        """
        noise = None
        if raw_noise_std > 0.0:
            if pytest:
                np.random.seed(0)
                noise = torch.tensor(np.random.rand(*list(raw[..., 3].shape)) * raw_noise_std, dtype=torch.float32,
                                     device=raw.device)
            else:
                noise = torch.randn(raw[..., 3].shape, device=raw.device) * raw_noise_std
        density = raw[..., 3]
        if z_vals.shape[-1] == 0:  # sampling_trainer.py:219-220
            R = raw.shape[0]
            zeros = torch.zeros((R,), device=raw.device)
            return (torch.zeros((R, 3), device=raw.device), torch.full((R,), 1e10, device=raw.device), zeros,
                    zeros.clone(), density, raw[..., 3].clone(), raw[..., 3].clone())
        if torch.is_grad_enabled() and (raw.requires_grad or z_vals.requires_grad or rays_d.requires_grad):
            if z_vals.shape[-1] == 1 and noise is None:      # the training step's operator (nerf_utils.py:692-715)
                from .autograd import SingleSampleComposite

                rgb_map, disp_map, acc_map, depth_map, alphas, weights = SingleSampleComposite.apply(
                    raw, z_vals, rays_d, bool(white_bkgd))
            else:                                            # any N, with or without noise: ns_raw2outputs_backward
                from .autograd import composite

                rgb_map, disp_map, acc_map, depth_map, alphas, weights = composite(raw, z_vals, rays_d, noise, white_bkgd)
            return rgb_map, disp_map, acc_map, depth_map, density, alphas, weights
        rgb_map, disp_map, acc_map, depth_map, alphas, weights = ops.raw2outputs(raw, z_vals, rays_d, noise, white_bkgd)
        return rgb_map, disp_map, acc_map, depth_map, density, alphas, weights
