"""Cost of the depth tangents of the one-kernel renderer (ns_render_rays_fused_tangent) on one MI355X, production network shapes
(lego_synth: NeRF 8 x 256, DepthNet 10 x 256; the field's operand type from --field: f16x3, or bf16 / f16 with approximate=True):
  * an 800 x 800 x 64 frame, forward only (ns_render_rays_fused, the field and an f16x3 DepthNet) against forward + tangents, the two
    alternated on the same box; device events around the MLP kernel and around the whole call;
  * a DepthNet gradient (loss on rgb) at 16 384 and 65 536 rays x 64 samples: time and peak memory through
    autograd.render_depthnet_differentiable and through the autograd chain (PlaceSamples -> NerfInputGrad -> Composite).
Prints one JSON line per measurement."""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nerf_sampling_amd import autograd, ops  # noqa: E402
from nerf_sampling_amd.depth_net import DepthNet  # noqa: E402
from nerf_sampling_amd.run_nerf_helpers import NeRF  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402


def modules(scene):
    """the fine NeRF and the DepthNet of an oracle scene (seeded synthetic weights) on the GPU, frozen"""
    cfg, params = O.SCENES[scene], O.make_scene(scene)
    fine = NeRF(D=cfg["fine"]["D"], W=cfg["fine"]["W"], input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    fine.load_state_dict(params["fine"])
    dn = DepthNet(hidden_sizes=[cfg["depth"]["width"]] * cfg["depth"]["n_layers"],
                  cat_hidden_sizes=[cfg["depth"]["width"]] * cfg["depth"]["n_layers"], sphere_radius=2.0)
    dn.load_state_dict(params["depth"])
    out = {"fine": fine.cuda(), "depth": dn.cuda()}
    for net in out.values():
        for p in net.parameters():
            p.requires_grad_(False)
    return out


def frame(m, reps, field):
    H = W = 800
    _, K = O.blender_intrinsics(H, W)
    c2w = O.pose_spherical(30.0, -30.0, 4.0)[:3, :4]
    dn, nf = m["depth"].packed("f16x3"), m["fine"].packed(field)
    cam = (H, W, K, c2w, 0, H)
    ev = (ops.Event(), ops.Event())
    runs = {
        "forward": lambda: ops.render_rays_depthnet(dn, nf, camera=cam, n_samples=64, mode="uniform", std=0.1, one_kernel=True,
                                                    mlp_events=ev),
        "forward+tangent": lambda: ops.render_rays_depthnet_tangent(dn, nf, camera=cam, n_samples=64, std=0.1, mlp_events=ev,
                                                                    approximate=field != "f16x3"),
    }
    times = {k: {"call": [], "kernel": []} for k in runs}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for k, fn in runs.items():      # alternated
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[k]["call"].append(a.elapsed_time(b))
            times[k]["kernel"].append(ev[0].elapsed_ms(ev[1]))
    for k, t in times.items():
        med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
        print(json.dumps({"what": f"frame 800x800x64 {field}", "run": k, "call_ms_median": round(med["call"], 3),
                          "mlp_kernel_ms_median": round(med["kernel"], 3), "reps": reps}))


def gradient(m, R, reps, field, with_chain=True):
    net = copy.deepcopy(m["depth"])
    for p in net.parameters():
        p.requires_grad_(True)
    params = [p for p in net.parameters() if p.requires_grad]
    nf = m["fine"].packed(field)
    g = torch.Generator().manual_seed(0)
    H = W = 800
    _, K = O.blender_intrinsics(H, W)
    c2w = O.pose_spherical(30.0, -30.0, 4.0)[:3, :4]
    o, d, v = ops.get_rays(H, W, K, c2w)[:3]
    idx = torch.randperm(H * W, generator=g)[:R].cuda()
    o, d, v = o[idx].contiguous(), d[idx].contiguous(), v[idx].contiguous()
    target = torch.rand((R, 3), generator=g).cuda()

    def tangent():
        out = autograd.render_depthnet_differentiable(net, nf, rays=(o, d, v), n_samples=64, std=0.1, chunk=16384,
                                                      approximate=field != "f16x3")
        return torch.autograd.grad(((out["rgb"] - target) ** 2).mean(), params)

    def chain():
        mean = autograd.depthnet_forward_train(net, o, d).reshape(-1)
        pts, z = autograd.place_samples(o, d, mean, 64, "uniform", 0.1)
        raw = autograd.NerfInputGrad.apply(pts, v, m["fine"])
        rgb = autograd.composite(raw, z, d, None, True)[0]
        return torch.autograd.grad(((rgb - target) ** 2).mean(), params)

    for name, fn in (("tangent", tangent), ("chain", chain))[:2 if with_chain else 1]:
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(reps):
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        peak = torch.cuda.max_memory_allocated() - base
        print(json.dumps({"what": "DepthNet gradient, 64 samples", "rays": R, "path": name, "field": field,
                          "ms_median": round(sorted(ts)[len(ts) // 2], 2), "peak_MiB": round(peak / 2**20, 1), "reps": reps}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--field", choices=("f16x3", "bf16", "f16"), default="f16x3")
    ap.add_argument("--no-chain", action="store_true", help="skip the autograd chain's gradient (tens of GB at 65 536 rays)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    m = modules("lego_synth")
    frame(m, args.reps, args.field)
    for R in (16384, 65536):
        gradient(m, R, args.reps, args.field, not args.no_chain)


if __name__ == "__main__":
    main()
