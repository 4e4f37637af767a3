"""Counterpart of nerf_sampling/experiments/run.py: train the DepthNet against a frozen pretrained NeRF.

    python -m nerf_sampling_amd.experiments.run -d lego [--iters 100000]

Same flags and overrides as the reference (run.py:16-113); wandb is out of scope (-w accepted, ignored).
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
@click.option("-d", "--dataset", help="Name of the dataset to train on.", type=str, show_default=True)
@click.option("-m", "--model", help="Model type.", type=str, default="lego_depth_net_module", show_default=True)
@click.option("-w", "--wandb", type=click.Choice(["online", "offline", "disabled"], case_sensitive=False),
              default="disabled", help="Ignored (wandb logging is out of scope).", show_default=True)
@click.option("-si", "--single_image", is_flag=True, default=False, help="Train sampling network on single image.")
@click.option("-sr", "--single_ray", is_flag=True, default=False, help="Train sampling network on single ray.")
@click.option("-ip", "--i_print", default=1000, help="Frequency of log printing.", show_default=True)
@click.option("--iters", default=100_000, show_default=True, help="Training iterations (EPOCHS in the reference).")
@click.option("--dtype", default="f32", type=click.Choice(["bf16", "f16", "f32", "f16x3"]), show_default=True,
              help="MFMA operand precision of the frozen-NeRF forward kernels (not in the reference).")
@click.option("--fused-step", "fused_step", is_flag=True, default=False,
              help="Run the DepthNet branch of the training step as one kernel and the target pass as one call (not in the "
                   "reference; DepthNetTrainer(fused_step=True)).")
@click.option("--fit-field", "fit_field", is_flag=True, default=False,
              help="Fit the radiance field itself (trainers.FieldFitter: both NeRFs' weights on the HIP kernels) instead of "
                   "training the DepthNet; writes {root}/logs/{expname}_field/NNNNNN.tar (not in the reference).")
@click.option("--gemm-engine", "gemm_engine", default="tile", type=click.Choice(["tile", "tall"]), show_default=True,
              help="With --fit-field: the GEMM kernel of the layer forwards and grad-input products (FieldFitter(gemm_engine=...)).")
@click.option("--device-batches", "device_batches", default=None, type=click.Choice(["gather", "draw"]),
              help="Make the training ray batches from a dataset resident on the device (Trainer(device_batches=...), not in the "
                   "reference): 'gather' uploads the host's np.random draws as indices (the same batches), 'draw' draws them "
                   "in the kernel with its own generator (other batches than np.random's).")
@click.option("--device-eval", "device_eval", is_flag=True, default=False,
              help="Score the test views on the device every i_testset iterations (Trainer(device_eval=True), not in the "
                   "reference's form: its Trainer.log renders them to the host); with --fit-field the fit's held-out PSNR "
                   "(FieldFitter.fit(i_testset=...)).")
@click.option("--device-ssim", "device_ssim", is_flag=True, default=False,
              help="--device-eval, and the SSIM of the test views beside their PSNR (ns_image_ssim, Trainer(device_ssim=True) / "
                   "FieldFitter.fit(test_ssim=True)): ssim.txt next to every psnr.txt.")
@click.option("--device-depth", "device_depth", is_flag=True, default=False,
              help="--device-eval, and the MSE of the DepthNet's placed samples and of its own depth against the field's "
                   "max-weight depth on the test views (ns_depth_sqerr, Trainer(device_depth=True)): depth.txt next to every "
                   "psnr.txt.  Not with --fit-field, which has no DepthNet.")
@click.option("--device-frames", "device_frames", is_flag=True, default=False,
              help="--device-eval, and the test views as NNN.png next to every psnr.txt (ns_frame_to8b on the device, "
                   "nerf_utils.FrameWriter's threads for the PNGs; Trainer(device_frames=True) / "
                   "FieldFitter.fit(test_frames=True)).")
@click.option("--device-video", "device_video", is_flag=True, default=False,
              help="--device-eval, and the reference's i_video branch: every i_video iterations the spiral render_poses as "
                   "{expname}_spiral_{i:06d}_rgb/NNN.png and ..._disp/NNN.png (rgb.mp4 / disp.mp4 too where imageio is "
                   "installed) through nerf_utils.write_video -- one render per pose, the disparity's maximum over all frames "
                   "kept on the device (ns_map_max, ns_map_to8b; Trainer(device_video=True)).  Not with --fit-field, which "
                   "renders no spiral.")
@click.option("--mesh-simplify", "mesh_simplify", default=0.0, type=click.FloatRange(min=0.0), show_default=True,
              help="Trainer(mesh_simplify=K), not in the reference: where the configuration sets device_mesh, scene_mesh.ply is "
                   "simplified by vertex clustering on cluster cells K lattice cells wide (ns_mesh_simplify).  0: off.")
@click.option("--root", default=os.getcwd(), show_default=True, help="Directory holding dataset/ pretrained/ logs/.")
def main(**kw):
    """Run sampling-network training with the provided configuration (reference flow: run.py:79-155)."""
    with open(kw["config"], "r") as fin:
        config = yaml.safe_load(fin)[kw["model"]]
    k = config["kwargs"]
    k.update(single_image=kw["single_image"], single_ray=kw["single_ray"], i_print=kw["i_print"])
    root, dataset_name = kw["root"], kw["dataset"]
    datadir, ft_path = kw["dataset_path"], None
    if dataset_name is not None:
        datadir = f"{root}/dataset/{dataset_name}"
        ft_path = f"{root}/pretrained/nerf/{dataset_name}/200000.tar"
    if datadir is None:
        print("Please specify the name of the dataset or provide the path to the folder")
        return
    override_config(config=k, update={"depth_net_lr": 1e-4, "n_layers": 10, "layer_width": 256,
                                      "train_depth_net_only": True, "sphere_radius": 2})
    torch.manual_seed(42)
    set_global_device(k["device"])
    ops.set_compute_dtype(kw["dtype"])
    k.update(ft_path=ft_path, depth_net_path=None, datadir=datadir, basedir=f"{root}/logs")
    if kw["fused_step"]:
        k["fused_step"] = True
    if kw["device_batches"]:
        k["device_batches"] = kw["device_batches"]
    if kw["mesh_simplify"]:
        k["mesh_simplify"] = kw["mesh_simplify"]
    if kw["device_eval"] or kw["device_ssim"] or kw["device_depth"] or kw["device_frames"] or kw["device_video"]:
        k["device_eval"] = True
    if kw["device_video"]:
        k["device_video"] = True
    if kw["device_frames"]:
        k["device_frames"] = True
    if kw["device_ssim"]:
        k["device_ssim"] = True
    if kw["device_depth"]:
        k["device_depth"] = True
    if kw["fit_field"]:
        if kw["device_depth"]:
            raise click.UsageError("--device-depth scores a DepthNet's depth; --fit-field trains none")
        if kw["device_video"]:
            raise click.UsageError("--device-video writes the DepthNet training's spiral; --fit-field renders none")
        k.update(ft_path=None)
        return fit_field(load_obj_from_config(cfg=config), kw["iters"], gemm_engine=kw["gemm_engine"])
    trainer = load_obj_from_config(cfg=config)
    trainer.train(N_iters=kw["iters"] + 1)


def fit_field(trainer, n_iters, gemm_engine="tile"):
    """--fit-field: a FieldFitter built from the trainer's configuration (network shapes, sample counts, learning rate, noise,
    background) on the trainer's dataset; checkpoints load as ft_path of the DepthNet training and of experiments/render.py."""
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.run_nerf_helpers import NeRF
    from nerf_sampling_amd.trainers import FieldFitter
    from nerf_sampling_amd.utils import unfreeze_model

    hwf, poses, i_test, _i_val, i_train, images, _render_poses = trainer.load_data()
    trainer.cast_intrinsics_to_right_types(hwf=hwf)
    trainer.no_reload = True
    kw_train, _kw_test, _start, _grad_vars, _optimizer = nerf_utils.create_nerf(trainer, NeRF)
    for key in ("network_fn", "network_fine"):
        if kw_train[key] is not None:
            unfreeze_model(kw_train[key])
    fitter = FieldFitter(kw_train["network_fn"], kw_train["network_fine"], N_samples=trainer.N_samples,
                         N_importance=trainer.N_importance, lrate=trainer.lrate, lrate_decay=trainer.lrate_decay,
                         white_bkgd=trainer.white_bkgd, raw_noise_std=trainer.raw_noise_std, perturb=trainer.perturb,
                         lindisp=trainer.lindisp, near=trainer.near, far=trainer.far, gemm_engine=gemm_engine)
    split = dict(images=images, poses=poses, hwf=hwf, i_train=i_train, i_test=i_test)
    return fitter.fit(split, n_iters, N_rand=trainer.N_rand, basedir=trainer.basedir, expname=f"{trainer.expname}_field",
                      i_weights=trainer.i_weights, i_print=trainer.i_print, device_batches=trainer.device_batches,
                      batch_seed=trainer.batch_seed, i_testset=trainer.i_testset if trainer.device_eval else 0,
                      test_ssim=trainer.device_ssim, test_frames=trainer.device_frames)


if __name__ == "__main__":
    main()
