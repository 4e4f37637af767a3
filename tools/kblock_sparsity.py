"""How often a K-block (32 hidden units) of a trunk layer's output is all zero for a whole wave of the render kernel, on the CPU
with the fp32 oracle: the table behind the K-block-skipping render kernel.

The frame is a bench frame (default shapes_fit, pose 17, every 80th row, DepthNet placement with 64 samples); a wave is 80
consecutive samples and a group 320, as the five-tile kernel forms them.  The unit order is the one NeRF.packed() applies
(run_nerf_helpers.firing_counts / unit_orders: calibrated on seeded points in a ball, not on the frame); --natural keeps the
trained order.  Per layer: the share of (wave, K-block) pairs that are all zero, the same for whole groups, the share for the
K-blocks the kernel tests (tools/gen_ob16_asm.py KBS_TESTED), and the histogram of the number of dead blocks at the END of a
wave's mask, 0 .. 8 (the order makes dead blocks a suffix).  Last: the chunk steps of a wave pass those blocks stand for -- any
dead tested block (the K-block-skipping kernel) next to the trailing dead tested blocks alone, min(suffix, 4) (the dead-suffix
kernel) -- and, of the waves whose suffix is 4 or longer in some layer, the share whose suffix is 6 or longer in two layers or more.
    python tools/kblock_sparsity.py [--scene shapes_fit] [--pose 17] [--row-step 80] [--natural]"""
import argparse
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from nerf_sampling_amd import run_nerf_helpers as H  # noqa: E402
from nerf_sampling_amd import synthetic  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402

TESTED = (4, 5, 6, 7)
CONSUMER_CHUNKS = {3: 16, 4: 16, 5: 16, 6: 16, 7: 9}      # sub-blocks of the statements fed by layer l (7: sigma + colour)
STEPS_PER_PASS = 1045


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="shapes_fit")
    ap.add_argument("--pose", type=int, default=17)
    ap.add_argument("--row-step", type=int, default=80)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--natural", action="store_true", help="the units in their trained order")
    a = ap.parse_args()
    torch.manual_seed(0)
    params = synthetic.make_scene(a.scene)
    p = {k: v.float() for k, v in params["fine"].items()}
    net = H.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    net.load_state_dict(params["fine"])
    orders = [torch.arange(256)] * 8 if a.natural else H.unit_orders(H.firing_counts(net))
    Hh = Ww = a.size
    _, K = synthetic.blender_intrinsics(Hh, Ww)
    c2w = synthetic.render_poses(40)[a.pose, :3, :4]
    with torch.no_grad():
        o, d = O.camera_rays(Hh, Ww, K, c2w)
        o, d = o[::a.row_step].reshape(-1, 3).float(), d[::a.row_step].reshape(-1, 3).float()
        z = O.depthnet_forward({k: v.float() for k, v in params["depth"].items()}, o, d)
        pts, _ = O.place_samples(o, d, z, a.samples, "uniform", 0.1)
        emb = O.posenc(pts.reshape(-1, 3), 10)
        S = emb.shape[0]
        idx = torch.arange(-(-S // 320) * 320).clamp_(max=S - 1)          # the tail's waves hold copies of the last sample
        h, dead = emb, {}
        for i in range(8):
            h = torch.relu(O._lin(p, f"pts_linears.{i}", h))
            blocks = (h[:, orders[i]] > 0)[idx].reshape(-1, 80, 8, 32).any(3).any(1)      # [waves, 8] live
            dead[i] = ~blocks
            if i == 4:
                h = torch.cat([emb, h], -1)
    print(f"{a.scene} pose {a.pose}, every {a.row_step}th row, {S} samples, {dead[0].shape[0]} waves, "
          f"{'trained' if a.natural else 'firing'} order")
    print("layer | (wave, K-block) dead | whole group dead | tested blocks dead | dead blocks at the end of the mask: 0 1 2 3 4 5 6 7 8")
    steps = steps_suffix = 0.0
    runs = {}
    for i in range(8):
        dw = dead[i]
        dg = dw.reshape(-1, 4, 8).all(1)
        tested = dw[:, list(TESTED)]
        run = torch.zeros(dw.shape[0], dtype=torch.long)
        alive = torch.ones(dw.shape[0], dtype=torch.bool)
        for kb in range(7, -1, -1):
            alive &= dw[:, kb]
            run += alive.long()
        hist = [float((run == k).float().mean()) for k in range(9)]
        runs[i] = run
        print(f"  {i}   | {100 * float(dw.float().mean()):5.1f} % | {100 * float(dg.float().mean()):5.1f} % | "
              f"{100 * float(tested.float().mean()):5.1f} % | " + " ".join(f"{100 * x:5.1f}" for x in hist))
        if i in CONSUMER_CHUNKS:
            steps += CONSUMER_CHUNKS[i] * float(tested.float().sum(1).mean())
            steps_suffix += CONSUMER_CHUNKS[i] * float(run.clamp(max=len(TESTED)).float().mean())
    print(f"chunk steps a wave pass skips (tested blocks {TESTED}, colour statements of every wave counted): "
          f"{steps:.1f} of {STEPS_PER_PASS} ({100 * steps / STEPS_PER_PASS:.1f} %)")
    print(f"... of them by the trailing dead tested blocks alone (one choice per statement): {steps_suffix:.1f} "
          f"({100 * steps_suffix / STEPS_PER_PASS:.1f} % of the pass, {100 * steps_suffix / max(steps, 1e-9):.0f} % of the any-mask figure)")
    long4 = torch.stack([runs[i] >= 4 for i in CONSUMER_CHUNKS]).any(0)
    long6 = torch.stack([runs[i] >= 6 for i in CONSUMER_CHUNKS]).long().sum(0) >= 2
    print(f"waves with a suffix >= 4 in some consumed layer: {100 * float(long4.float().mean()):.1f} %; of them, suffix >= 6 in two or "
          f"more layers: {100 * float((long6 & long4).float().sum() / max(int(long4.sum()), 1)):.1f} %")


if __name__ == "__main__":
    main()
