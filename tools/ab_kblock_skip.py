"""Same-box, same-process A/B of the K-block-skipping render kernel (--switch kblock_skip, the default) or of the dead-suffix
render kernel (--switch kblock_suffix; --on-value 2, the default there, takes unit-ordered handles only, so input (c) shows that the
render kernel runs: its counter reads 0) against the render kernel, through ns_debug_set: whole 800 x 800 x 64 bf16 frames, the switch alternating after a warm-up, as tools/ab_colour_skip.py
does for the colour skip (a side of a pair is --frames consecutive spiral poses timed between two synchronisations; both sides
see the same poses).  Three inputs: (a) the bench scene (shapes_fit) packed with the unit order, (b) lego_synth (seeded random
weights) packed with the unit order, (c) the bench scene packed in its own order -- next to nothing skips there, so the pair shows
the new kernel's overhead (mask ORs, tests and branches).  Prints per-pair times, the share of chunk steps skipped (the device
counter, read on an untimed frame), the spread of each side and the verdict of the acceptance rule.
    python tools/ab_kblock_skip.py [--switch kblock_skip|kblock_suffix] [--on-value V] [--pairs 6] [--frames 40] [--size 800]"""
import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import bench  # noqa: E402
from nerf_sampling_amd import ops, synthetic  # noqa: E402
from nerf_sampling_amd.parallel import FrameRenderer, hip_row_renderer  # noqa: E402

STEPS_PER_PASS = 1045            # chunk steps of one wave pass (67 slabs less the pad steps): the denominator of the skipped share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=40, help="frames (consecutive poses) per side of a pair; 40 = the whole spiral")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--switch", default="kblock_skip", choices=["kblock_skip", "kblock_suffix"], help="the switch that alternates")
    ap.add_argument("--on-value", type=int, default=None, help="its value on the 'on' side (default: 1 for kblock_skip, 2 for kblock_suffix)")
    a = ap.parse_args()
    assert a.pairs >= 6, "at least six pairs"
    on_value = a.on_value if a.on_value is not None else {"kblock_skip": 1, "kblock_suffix": 2}[a.switch]
    counter = {"kblock_skip": ops.kblock_skip_count, "kblock_suffix": ops.kblock_suffix_count}[a.switch]
    dev = torch.device("cuda", 0)
    H = W = a.size
    _, K = synthetic.blender_intrinsics(H, W)
    poses = synthetic.render_poses(40)[:, :3, :4]
    inputs = []
    for label, scene, ordered in (("a shapes_fit, unit order", "shapes_fit", True), ("b lego_synth, unit order", "lego_synth", True),
                                  ("c shapes_fit, own order (overhead)", "shapes_fit", False)):
        _c, fine, dn, _p = bench.build_modules(scene, dev)
        if not ordered:
            fine = copy.deepcopy(fine)
            fine.unit_order = False
        inputs.append((label, fine.packed(a.dtype), dn.packed(ops.depthnet_dtype_for(a.dtype))))
    waves = 4 * -(-(H * W * a.samples) // 320)
    verdicts = {}
    for label, nw, dw in inputs:
        fr = FrameRenderer(H, W, hip_row_renderer(dw, nw, H, W, K, a.samples, "uniform", 0.1, device=dev, events=None), dev)

        def frame(first, off):
            with ops.debug_switch(**{a.switch: 0 if off else on_value}):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(a.frames):
                    fr.render(poses[(first + k) % 40])
                fr.finish()
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0) / a.frames

        for i in range(a.warmup):
            frame(i, False)
            frame(i, True)
        with ops.debug_switch(count_colour_skips=1, **{a.switch: on_value}):
            fr.render(poses[a.warmup % 40])
            fr.finish()
            share = counter() / (waves * STEPS_PER_PASS)
            colour = ops.colour_skip_count() / waves
        on, off = [], []
        for i in range(a.pairs):
            pose = (a.warmup + i * a.frames) % 40
            order = (False, True) if i % 2 == 0 else (True, False)      # alternate which side goes first
            t = {o: frame(pose, o) for o in order}
            on.append(t[False])
            off.append(t[True])
            print(f"{label}: pair {i}: skip on {t[False]:.3f} ms, off {t[True]:.3f} ms, gain {t[True] - t[False]:+.3f} ms", flush=True)
        med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])   # noqa: E731
        gains = [b - c for b, c in zip(off, on)]
        spread = max(max(on) - min(on), max(off) - min(off))
        res = {"switch": a.switch, "on_value": on_value, "input": label, "pairs": a.pairs, "frames_per_side": a.frames, "steps_skipped": round(share, 4), "waves_skipping_colour": round(colour, 4),
               "median_on_ms": round(med(on), 3), "median_off_ms": round(med(off), 3), "median_gain_ms": round(med(gains), 3),
               "spread_on_ms": round(max(on) - min(on), 3), "spread_off_ms": round(max(off) - min(off), 3),
               "every_pair_favours_skip": all(g > 0 for g in gains), "gain_over_3x_spread": med(gains) >= 3 * spread,
               "not_slower_than_spread": med(gains) >= -spread}
        verdicts[label[0]] = res
        print(json.dumps(res), flush=True)
    ok = verdicts["a"]["every_pair_favours_skip"] and verdicts["a"]["gain_over_3x_spread"] and verdicts["c"]["not_slower_than_spread"]
    print(json.dumps({"accept": bool(ok), "rule": "(a): every pair favours the change and the median gain >= 3 x the larger max - min "
                      "spread of the two sides; (c): not slower than that spread"}))


if __name__ == "__main__":
    main()
