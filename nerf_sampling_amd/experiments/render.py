"""Counterpart of nerf_sampling/experiments/render.py: same flags, same yaml -> trainer -> train() flow,
rendering through the HIP path.  wandb is out of scope (the -w flag is accepted and ignored).

    python -m nerf_sampling_amd.experiments.render -d lego [-nf | -nm | -nc] [-e] [--dtype bf16]
"""

import os

import click
import torch
import yaml

from nerf_sampling_amd import ops
from nerf_sampling_amd.utils import load_obj_from_config, override_config, set_global_device

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@click.command()
@click.option("-c", "--config", help="Path to configuration file.", type=str,
              default=f"{ROOT_DIR}/experiments/configs/lego.yaml", show_default=True)
@click.option("-dp", "--dataset_path", help="Path to dataset folder.", type=str, show_default=True)
@click.option("-d", "--dataset", help="Name of the dataset to render.", type=str, show_default=True)
@click.option("-m", "--model", help="Model type.", type=str, default="lego_depth_net_module", show_default=True)
@click.option("-w", "--wandb", default="disabled", help="Ignored (wandb logging is out of scope).", show_default=True)
@click.option("-si", "--single_image", is_flag=True, default=False, show_default=True)
@click.option("-sr", "--single_ray", is_flag=True, default=False, show_default=True)
@click.option("-rt", "--render_test", is_flag=True, default=False, help="Perform render test", show_default=True)
@click.option("-ssd", "--save_scene_data", is_flag=True, default=False, show_default=True)
@click.option("-nc", "--nerf_compare", is_flag=True, default=False,
              help="Compare depth network predictions to the original NeRF most important samples.", show_default=True)
@click.option("-nm", "--nerf_max", is_flag=True, default=False, help="Use nerf max points to render", show_default=True)
@click.option("-nf", "--nerf_full", is_flag=True, default=False, help="Use full nerf to render", show_default=True)
@click.option("-e", "--experiments", is_flag=True, default=False, help="Use automatic experiments.", show_default=True)
@click.option("-tmp", "--temporary", is_flag=True, default=False, help="Use temporary folder for experiment.",
              show_default=True)
@click.option("-ip", "--i_print", default=1000, help="Frequency of log printing.", show_default=True)
@click.option("--dtype", default="bf16", type=click.Choice(["bf16", "f16", "f32", "f16x3"]), show_default=True,
              help="MFMA operand precision of the HIP kernels (not in the reference).")
@click.option("--psnr-guard/--no-psnr-guard", "psnr_guard", default=True, show_default=True,
              help="(not in the reference) This CLI's deliverable is a PSNR file: with a 16-bit --dtype the DepthNet and the "
                   "last sample of a ray whose density there is near zero -- the one composited with dist = 1e10 -- run on "
                   "fp32-grade split-fp16 operands (ops.set_psnr_guard; ~4.5 % of the frame).  Per-image PSNR then stays within "
                   "0.03 dB of the fp32 arithmetic on a 28-30 dB scene; without it the 16-bit paths sit at 0.03-0.26 dB "
                   "(tools/guard_experiment.py).")
@click.option("--device-psnr", "device_psnr", is_flag=True, default=False,
              help="(not in the reference) Score the test views on the device (Trainer(device_eval=True), "
                   "nerf_utils.evaluate_views): the same psnr.txt, no frame copied to the host and no PNG written.  Serves "
                   "single runs and the -e sweep; not with -nc / -nm.")
@click.option("--device-ssim", "device_ssim", is_flag=True, default=False,
              help="(not in the reference) --device-psnr, and the SSIM of every test view beside it (ns_image_ssim, "
                   "Trainer(device_ssim=True)): ssim.txt next to psnr.txt.")
@click.option("--device-depth", "device_depth", is_flag=True, default=False,
              help="(not in the reference) --device-psnr, and per test view the MSE of the DepthNet's placed samples and of its "
                   "own depth against the field's max-weight depth (ns_depth_sqerr, Trainer(device_depth=True)): -nc's MSE "
                   "without its host copies, in depth.txt next to psnr.txt.  Not with -nf.")
@click.option("--device-frames", "device_frames", is_flag=True, default=False,
              help="(not in the reference) --device-psnr, and the frames as NNN.png beside psnr.txt after all: quantised on the "
                   "device (ns_frame_to8b, to8b's bits), copied as bytes and encoded by nerf_utils.FrameWriter's threads while "
                   "the next view renders (Trainer(device_frames=True)).")
@click.option("--device-video", "device_video", is_flag=True, default=False,
              help="(not in the reference) --device-psnr, and instead of the test views the spiral render_poses, as the "
                   "training's i_video branch writes it: renderonly_path_*/rgb/NNN.png and disp/NNN.png (rgb.mp4 / disp.mp4 too "
                   "where imageio is installed) through nerf_utils.write_video -- one render per pose, the disparity divided by "
                   "its maximum over all frames, which stays on the device (ns_map_max, ns_map_to8b; "
                   "Trainer(device_video=True)).  There is no ground truth on the spiral: the PSNR printed is 0.")
@click.option("--device-cloud", "device_cloud", is_flag=True, default=False,
              help="(not in the reference) Also select the scene's point cloud of the rendered views on the device "
                   "(ns_cloud_append, Trainer(device_cloud=True), nerf_utils.scene_cloud): scene_cloud.pt and scene_cloud.ply "
                   "beside the frames, what -ssd's scene_data.pt gives after experiments/plot.py's threshold, without its "
                   "per-sample host copies.  With -nm / -nf the field's samples.")
@click.option("--cloud-min-weight", "cloud_min_weight", default=0.0, type=float, show_default=True,
              help="(not in the reference) --device-cloud keeps the samples whose weight is at least this.  0.0 is the "
                   "reference's own (plot.py:17) and keeps every sample: raise it (0.05 - 0.5) for a cloud of the surfaces.")
@click.option("--cloud-points", "cloud_points", default=None, type=int, show_default=True,
              help="(not in the reference) --device-cloud writes at most this many of the kept samples, drawn uniformly "
                   "(plot.py draws 5e4).")
@click.option("--device-mesh", "device_mesh", is_flag=True, default=False,
              help="(not in the reference) Also extract a triangle mesh of the field's density on the device (ns_mesh_extract, "
                   "Trainer(device_mesh=True), nerf_utils.scene_mesh): scene_mesh.ply beside the frames -- marching tetrahedra "
                   "on a lattice of the fine network's density, a closed surface facing outwards, coloured by the field.")
@click.option("--mesh-resolution", "mesh_resolution", default=256, type=int, show_default=True,
              help="(not in the reference) --device-mesh samples the density at this many lattice points per axis.")
@click.option("--mesh-threshold", "mesh_threshold", default=50.0, type=float, show_default=True,
              help="(not in the reference) --device-mesh cuts the density at this value.  50 is a starting value, not a "
                   "property of a scene: lower it where the surface has holes; rather than raise it where it carries floaters, drop them "
                   "with --mesh-keep-largest or --mesh-min-triangles.")
@click.option("--mesh-bound", "mesh_bound", default=1.5, type=float, show_default=True,
              help="(not in the reference) --device-mesh covers the cube [-bound, bound]^3 of scene coordinates.")
@click.option("--mesh-min-triangles", "mesh_min_triangles", default=0, type=click.IntRange(min=0), show_default=True,
              help="(not in the reference) --device-mesh keeps only the connected components of its surface with at least this "
                   "many triangles (ns_mesh_components, nerf_utils.mesh_filter): floaters, the small closed blobs of stray "
                   "density around the object, leave scene_mesh.ply.  0: no filter.")
@click.option("--mesh-keep-largest", "mesh_keep_largest", default=0, type=click.IntRange(min=0), show_default=True,
              help="(not in the reference) --device-mesh keeps only this many of its surface's connected components, those with "
                   "the most triangles (among those --mesh-min-triangles leaves).  0: no filter.")
@click.option("--mesh-normals", "mesh_normals", is_flag=True, default=False,
              help="(not in the reference) --device-mesh also writes per-vertex normals nx ny nz into scene_mesh.ply "
                   "(ns_mesh_normals, nerf_utils.scene_mesh_shaded): the density lattice's gradient at each vertex, so that a "
                   "viewer shades the surface and not its triangles.")
@click.option("--mesh-colour-view", "mesh_colour_view", default="centre", type=click.Choice(["centre", "normal"]),
              show_default=True,
              help="(not in the reference) --device-mesh queries a vertex's colour looking towards the box centre, or with "
                   "'normal' (it needs --mesh-normals) looking at the surface along its inward normal.")
@click.option("--mesh-simplify", "mesh_simplify", default=0.0, type=click.FloatRange(min=0.0), show_default=True,
              help="(not in the reference) --device-mesh simplifies its surface by vertex clustering before it is coloured and "
                   "written (ns_mesh_simplify, nerf_utils.scene_mesh_simplified): the vertices within a cluster cell this many "
                   "lattice cells wide collapse onto the one of them nearest their centroid -- about K^2 times fewer "
                   "triangles, every vertex one of the unsimplified surface's.  0: off.")
@click.option("--device-mesh-eval", "device_mesh_eval", is_flag=True, default=False,
              help="(not in the reference) --device-mesh also rasterises scene_mesh.ply's mesh from the held-out cameras "
                   "(ns_mesh_raster) and scores it on the device (nerf_utils.score_mesh_views): mesh_psnr.txt against the "
                   "photographs, mesh_depth.txt and mesh_iou.txt against the field's depth and opacity, and mesh_rgb/ and "
                   "mesh_depth/ PNGs -- a number for --mesh-threshold.")
@click.option("--root", default=os.getcwd(), show_default=True,
              help="Directory holding dataset/ pretrained/ logs/ (the reference uses its package directory).")
def main(**kw):
    """Render with a pretrained NeRF + DepthNet (reference flow: render.py:135-272)."""
    with open(kw["config"], "r") as fin:
        config = yaml.safe_load(fin)[kw["model"]]
    k = config["kwargs"]
    k.update(single_image=kw["single_image"], single_ray=kw["single_ray"], save_scene_data=kw["save_scene_data"],
             i_print=kw["i_print"], compare_nerf=kw["nerf_compare"], use_nerf_max_pts=kw["nerf_max"],
             use_full_nerf=kw["nerf_full"], render_only=True, render_test=True)
    if kw["device_psnr"] or kw["device_ssim"] or kw["device_depth"] or kw["device_frames"] or kw["device_video"]:
        k["device_eval"] = True
    if kw["device_video"]:
        k.update(device_video=True, render_test=False)
    if kw["device_frames"]:
        k["device_frames"] = True
    if kw["device_ssim"]:
        k["device_ssim"] = True
    if kw["device_depth"]:
        k["device_depth"] = True
    if kw["device_cloud"]:
        k.update(device_cloud=True, cloud_min_weight=kw["cloud_min_weight"], cloud_points=kw["cloud_points"])
    if kw["device_mesh"]:
        k.update(device_mesh=True, mesh_resolution=kw["mesh_resolution"], mesh_threshold=kw["mesh_threshold"],
                 mesh_bound=kw["mesh_bound"], mesh_min_triangles=kw["mesh_min_triangles"],
                 mesh_keep_largest=kw["mesh_keep_largest"], mesh_normals=kw["mesh_normals"],
                 mesh_colour_view=kw["mesh_colour_view"])
        if kw["mesh_simplify"]:
            k["mesh_simplify"] = kw["mesh_simplify"]
    if kw["device_mesh_eval"]:
        if not kw["device_mesh"]:
            raise click.UsageError("--device-mesh-eval scores the mesh of --device-mesh")
        k["device_mesh_eval"] = True
    root = kw["root"]
    datadir, ft_path, depth_net_path = kw["dataset_path"], None, None
    dataset_name = kw["dataset"]
    if dataset_name is not None:
        datadir = f"{root}/dataset/{dataset_name}"
        ft_path = f"{root}/pretrained/nerf/{dataset_name}/200000.tar"
        depth_net_path = f"{root}/pretrained/depth_net/{dataset_name}/files/sampler_experiment/200000.tar"
    if datadir is None:
        print("Please specify the name of the dataset or provide the path to the folder")
        return
    basedir = f"{root}/logs/{dataset_name}"
    set_global_device(k["device"])
    ops.set_compute_dtype(kw["dtype"])
    ops.set_psnr_guard(kw["psnr_guard"])
    override_config(config=k, update={"depth_net_lr": 1e-4, "n_layers": 10, "layer_width": 256,
                                      "train_depth_net_only": True, "sphere_radius": 2})
    torch.manual_seed(42)
    k.update(datadir=datadir, basedir=basedir, ft_path=ft_path, depth_net_path=depth_net_path)
    n_samples, distance, sampling_mode = 2, 0.01, "uniform"   # the reference's in-source defaults (render.py:208-212)

    def expname(ns, dist, mode):
        if kw["temporary"]:
            return "tmp"
        if kw["nerf_compare"]:
            return f"{dataset_name}_depth_net_render_mse"
        if kw["nerf_max"]:
            return f"{dataset_name}_nerf_max_render"
        if kw["nerf_full"]:
            return f"{dataset_name}_nerf_full_render"
        return f"{dataset_name}_depth_net_render_n_samples_{ns}_distance_{dist}_sampling_mode_{mode}"

    if kw["experiments"]:  # the -e sweep of render.py:232-261
        basedir = f"{root}/logs/{dataset_name}/experiments"
        os.makedirs(basedir, exist_ok=True)
        f = os.path.join(basedir, "experiments_results.txt")
        with open(f, "w") as file:
            file.write("Experiments")
        for sampling_mode in ["uniform", "gaussian"]:
            k["basedir"] = os.path.join(basedir, sampling_mode)
            with open(f, "a") as file:
                file.write(f"\n\nSampling mode: {sampling_mode}\n\n")
            for n_samples in [2, 32, 64, 128]:
                with open(f, "a") as file:
                    file.write(f"N_samples: {n_samples}:\n")
                for distance in [0.1, 0.3, 0.5, 1]:
                    k.update(expname=f"{dataset_name}_depth_net_render_n_samples_{n_samples}_distance_{distance}"
                                     f"_sampling_mode_{sampling_mode}",
                             n_depth_samples=n_samples, distance=distance, sampling_mode=sampling_mode)
                    psnr = load_obj_from_config(cfg=config).train()
                    with open(f, "a") as file:
                        file.write(f"    Distance: {distance}, PSNR: {psnr:.2f}\n")
        return
    k.update(expname=expname(n_samples, distance, sampling_mode), n_depth_samples=n_samples, distance=distance,
             sampling_mode=sampling_mode)
    psnr = load_obj_from_config(cfg=config).train()
    print(f"Final psnr: {psnr}")


if __name__ == "__main__":
    main()
