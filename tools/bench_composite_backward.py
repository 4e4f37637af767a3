"""Time the compositing backward (ns_raw2outputs_backward: d_raw, d_z and d_rays_d from every upstream gradient but alphas)
against the forward (raw2outputs_kernel through ns_raw2outputs, all six outputs) on one MI355X, at the training batch
(1024 rays x {2, 64, 128} samples) and a frame's worth of rays (640 000 x 64).  Device events around `reps` back-to-back
launches after a warm-up; prints one JSON line per shape and the bytes each moves at the least."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nerf_sampling_amd import ops  # noqa: E402

SHAPES = [(1024, 2), (1024, 64), (1024, 128), (640_000, 64)]


def inputs(R, N, g):
    raw = torch.randn(R, N, 4, generator=g)
    z = 2.0 + torch.cumsum(torch.rand(R, N, generator=g) * (4.0 / N), -1)
    d = torch.randn(R, 3, generator=g)
    return raw.cuda(), z.cuda(), d.cuda()


def timed(fn, reps):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    g = torch.Generator().manual_seed(0)
    for R, N in SHAPES:
        raw, z, d = inputs(R, N, g)
        grads = [torch.randn(R, 3, generator=g).cuda(), torch.randn(R, generator=g).cuda() * 1e-3,
                 torch.randn(R, generator=g).cuda(), torch.randn(R, generator=g).cuda(), None,
                 torch.randn(R, N, generator=g).cuda()]
        reps = 200 if R * N < 1_000_000 else 20
        fwd = timed(lambda: ops.raw2outputs(raw, z, d, None, True), reps)
        bwd = timed(lambda: ops.raw2outputs_backward(raw, z, d, None, True, grads), reps)
        # least traffic: forward reads raw + z (20 B / sample), writes alphas + weights (8 B); backward reads raw, z and the
        # weights' gradient (24 B / sample), writes d_raw and d_z (20 B)
        print(json.dumps({"rays": R, "samples": N, "forward_ms": round(fwd, 4), "backward_ms": round(bwd, 4),
                          "ratio": round(bwd / fwd, 2), "forward_bytes": 28 * R * N, "backward_bytes": 44 * R * N,
                          "backward_GBps": round(44 * R * N / bwd / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
