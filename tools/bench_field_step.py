"""Time the field fit on one MI355X.

1. The grad-weight GEMM: ns_gemm_wgrad (autograd.linear_backward_weight_splitk) against the DepthNet step's
   linear_backward_weight (ns_gemm_fused + ns_colsum) at the NeRF's (N, K) shapes and rows = 65 536 and 196 608.  Three
   alternations of the two; each figure is the median of its three, with the spread (max - min) of the baseline's beside it.
2. The layer forward y = relu(x W^T + b) and the grad-input product dx = (dy W) * relu'(y): ns_gemm_tall
   (autograd.linear_forward_tall / linear_backward_input_tall) against ns_gemm_fused at the same rows and (N, K) =
   (out features, in features) of the Linear.  Same alternation and figures.
3. One whole step: trainers.FieldFitter.step at 1024 rays, 64 + 128 samples, two 8x256 networks, with gemm_engine "tile" and
   "tall", beside the torch-autograd step tools/fit_scene.py --engine torch performs at the same shapes (plain-torch twin,
   plain-torch compositing, torch.optim.Adam).

Device events around back-to-back calls after a warm-up; one JSON line per figure.  ``--step-only`` / ``--wgrad-only`` /
``--tall-only`` run one part (a profiler run wants the step alone: rocprofv3 --kernel-trace --stats -- python
tools/bench_field_step.py --step-only)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nerf_sampling_amd import autograd as ag  # noqa: E402

SHAPES = [(256, 256), (256, 319), (128, 283), (3, 128), (1, 256)]
TALL_SHAPES = [(256, 256), (256, 319), (128, 283), (4, 128), (256, 63)]
ROWS = [65_536, 196_608]


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def bench_wgrad():
    g = torch.Generator().manual_seed(0)
    for rows in ROWS:
        for N, K in SHAPES:
            dy, x = torch.randn(rows, N, generator=g).cuda(), torch.randn(rows, K, generator=g).cuda()
            new_W, new_b = ag.linear_backward_weight_splitk(dy, x)
            old_W, old_b = ag.linear_backward_weight(dy, x)
            scale = float(old_W.abs().max())
            diff = float((new_W - old_W).abs().max()) / scale
            base, new = [], []
            for _ in range(3):
                base.append(timed(lambda: ag.linear_backward_weight(dy, x), 5))
                new.append(timed(lambda: ag.linear_backward_weight_splitk(dy, x), 20))
            mb, mn = statistics.median(base), statistics.median(new)
            flops = 2.0 * rows * N * K
            print(json.dumps({"what": "wgrad", "rows": rows, "N": N, "K": K, "gemm_fused_colsum_ms": round(mb, 4),
                              "baseline_spread_ms": round(max(base) - min(base), 4), "gemm_wgrad_ms": round(mn, 4),
                              "wgrad_spread_ms": round(max(new) - min(new), 4), "speedup": round(mb / mn, 2),
                              "wgrad_TFLOPs": round(flops / mn / 1e9, 2), "wgrad_GBps": round(4.0 * rows * (N + K) / mn / 1e6, 1),
                              "max_diff_over_scale": diff}), flush=True)


def bench_tall():
    g = torch.Generator().manual_seed(0)
    for rows in ROWS:
        for N, K in TALL_SHAPES:
            x, W, b = torch.randn(rows, K, generator=g).cuda(), torch.randn(N, K, generator=g).cuda(), torch.randn(N, generator=g).cuda()
            dy, y = torch.randn(rows, N, generator=g).cuda(), torch.randn(rows, K, generator=g).cuda()
            pairs = {
                "forward": (lambda: ag._gemm(x, K, 1, W, K, 1, b, rows, N, K, act=ag.RELU),
                            lambda: ag.linear_forward_tall(x, W, b, ag.RELU)),
                "grad_input": (lambda: ag._gemm(dy, N, 1, W, 1, K, None, rows, K, N, dact=ag.RELU, dact_ref=y),
                               lambda: ag.linear_backward_input_tall(dy, W, dact_ref=y)),
            }
            for what, (old_fn, new_fn) in pairs.items():
                old, new = old_fn(), new_fn()
                diff = float((new - old).abs().max()) / max(float(old.abs().max()), 1e-30)
                base, tall = [], []
                for _ in range(3):
                    base.append(timed(old_fn, 5))
                    tall.append(timed(new_fn, 10))
                mb, mn = statistics.median(base), statistics.median(tall)
                print(json.dumps({"what": what, "rows": rows, "N": N, "K": K, "gemm_fused_ms": round(mb, 4),
                                  "baseline_spread_ms": round(max(base) - min(base), 4), "gemm_tall_ms": round(mn, 4),
                                  "tall_spread_ms": round(max(tall) - min(tall), 4), "speedup": round(mb / mn, 2),
                                  "tall_TFLOPs": round(2.0 * rows * N * K / mn / 1e9, 2),
                                  "tall_GBps": round(4.0 * rows * (N + K) / mn / 1e6, 1), "max_diff_over_scale": diff}), flush=True)


def bench_step(rays, n_coarse, n_fine):
    from nerf_sampling_amd.run_nerf_helpers import NeRF
    from nerf_sampling_amd.trainers import FieldFitter
    from tools.fit_scene import TorchNeRF, composite

    torch.manual_seed(0)
    mk = lambda: NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True).cuda()  # noqa: E731
    ff = FieldFitter(mk(), mk(), N_samples=n_coarse, N_importance=n_fine, perturb=1.0, raw_noise_std=1.0)
    ff_tall = FieldFitter(mk(), mk(), N_samples=n_coarse, N_importance=n_fine, perturb=1.0, raw_noise_std=1.0, gemm_engine="tall")
    o = torch.tensor([0.0, 0.0, 4.0]).expand(rays, 3).contiguous().cuda()
    d = torch.nn.functional.normalize(torch.randn(rays, 3) * 0.2 + torch.tensor([0.0, 0.0, -1.0]), dim=-1).cuda()
    batch, target = torch.stack([o, d], 0), torch.rand(rays, 3).cuda()

    # the torch-autograd step at the same shapes: two twins, coarse on Nc depths, fine on Nc + Nf
    tc, tf = TorchNeRF().cuda(), TorchNeRF().cuda()
    opt = torch.optim.Adam(list(tc.parameters()) + list(tf.parameters()), lr=5e-4)
    view = d / d.norm(dim=-1, keepdim=True)

    def torch_step():
        loss = 0.0
        for net, n in ((tc, n_coarse), (tf, n_coarse + n_fine)):
            z = torch.sort(2.0 + 4.0 * torch.rand(rays, n, device="cuda"), -1).values
            pts = o[:, None] + d[:, None] * z[..., None]
            raw = net(pts.reshape(-1, 3), view[:, None].expand(pts.shape).reshape(-1, 3)).reshape(rays, n, 4)
            rgb, _ = composite(raw, z, d, 1.0)
            loss = loss + ((rgb - target) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    hip, tall, ref = [], [], []
    for _ in range(3):
        ref.append(timed(torch_step, 5))
        hip.append(timed(lambda: ff.step(batch, target), 5))
        tall.append(timed(lambda: ff_tall.step(batch, target), 5))
    print(json.dumps({"what": "step", "rays": rays, "samples": [n_coarse, n_fine], "field_fitter_ms": round(statistics.median(hip), 3),
                      "field_fitter_spread_ms": round(max(hip) - min(hip), 3),
                      "field_fitter_tall_ms": round(statistics.median(tall), 3),
                      "field_fitter_tall_spread_ms": round(max(tall) - min(tall), 3),
                      "torch_autograd_ms": round(statistics.median(ref), 3),
                      "torch_spread_ms": round(max(ref) - min(ref), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wgrad-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--tall-only", action="store_true")
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--samples", type=int, nargs=2, default=[64, 128])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    only = args.wgrad_only or args.step_only or args.tall_only
    if args.wgrad_only or not only:
        bench_wgrad()
    if args.tall_only or not only:
        bench_tall()
    if args.step_only or not only:
        bench_step(args.rays, *args.samples)


if __name__ == "__main__":
    main()
