"""Cost of the PSNR guard on rays of several 64-sample chunks in the one-kernel renderer, on one MI355X, production network shapes
(lego_synth: NeRF 8 x 256, DepthNet 10 x 256 on f16x3 operands in every variant, so that the guard's own cost is what differs):
  * a 1600 x 1600 x 192 f16 frame and an 800 x 800 x 128 bf16 frame, each unguarded, guarded every-ray and guarded selective
    (ops.render_rays_depthnet(guard_long_rays="selective")) at threshold 16: one process, the variants alternated, three rounds,
    a round's figure the median of --reps frames; every frame is waited for under its own time limit;
  * with --parent-lib PATH (a libnerf_sampling_hip.so built from the parent commit): the unguarded frames of both shapes on that
    library and on this one, alternated, three rounds, one child process per library and round (a process loads one library),
    each under its own time limit.
Prints one JSON line per shape: the medians over the rounds, every-ray and selective as a percentage over the unguarded frame,
the spread (max - min over the rounds) of each, and the flagged share of rays; then the parent / this comparison."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("1600x1600x192 f16", 1600, 192, "f16"), ("800x800x128 bf16", 800, 128, "bf16"))
ROUNDS = 3
THRESHOLD = 16.0


def median(v):
    return sorted(v)[len(v) // 2]


def modules(scene):
    """the fine NeRF and the DepthNet of an oracle scene (seeded synthetic weights) on the GPU, frozen"""
    from nerf_sampling_amd.depth_net import DepthNet
    from nerf_sampling_amd.run_nerf_helpers import NeRF
    from oracle import nerf_oracle as O

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


def timed(fn, limit_s):
    """one frame between two device events; the wait for it ends the process when it outlasts limit_s"""
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    deadline = time.monotonic() + limit_s
    while not b.query():
        if time.monotonic() > deadline:
            print(json.dumps({"error": f"a frame did not finish within {limit_s} s"}), flush=True)
            os._exit(3)
        time.sleep(0.0005)
    return a.elapsed_time(b), out


def variants_of(m, size, n, dtype, guarded):
    import torch

    from nerf_sampling_amd import ops
    from oracle import nerf_oracle as O

    _, K = O.blender_intrinsics(size, size)
    cam = (size, size, K, O.pose_spherical(30.0, -30.0, 4.0)[:3, :4], 0, size)
    dn, nf, gw = m["depth"].packed("f16x3"), m["fine"].packed(dtype), m["fine"].packed("f16x3")
    ws = ops.RenderWorkspace()
    shard = torch.empty((size * size, 4), dtype=torch.float32, device="cuda")
    kw = dict(camera=cam, n_samples=n, mode="uniform", std=0.1, one_kernel=True, workspace=ws, shard=shard)
    runs = {"unguarded": lambda: ops.render_rays_depthnet(dn, nf, **kw)}
    if guarded:
        runs["every"] = lambda: ops.render_rays_depthnet(dn, nf, guard=gw, guard_threshold=THRESHOLD, guard_long_rays="every", **kw)
        runs["selective"] = lambda: ops.render_rays_depthnet(dn, nf, guard=gw, guard_threshold=THRESHOLD,
                                                             guard_long_rays="selective", extras=("guard_count",), **kw)
    return runs


def measure(m, reps, limit_s, guarded):
    """{shape: {variant: [one figure per round]}}, and the flagged share per shape"""
    import torch

    res, share = {}, {}
    for name, size, n, dtype in SHAPES:
        runs = variants_of(m, size, n, dtype, guarded)
        for fn in runs.values():                         # warm-up: workspaces, packings, code objects
            timed(fn, limit_s)
        rounds = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for k, fn in runs.items():                   # alternated
                ts = []
                for _ in range(reps):
                    t, out = timed(fn, limit_s)
                    ts.append(t)
                rounds[k].append(median(ts))
                if k == "selective":
                    share[name] = int(out["guard_count"]) / float(size * size)
        res[name] = rounds
        torch.cuda.empty_cache()
    return res, share


def child(reps, limit_s):
    import torch

    torch.cuda.set_device(0)
    res, _ = measure(modules("lego_synth"), reps, limit_s, guarded=False)
    print(json.dumps({name: r["unguarded"] for name, r in res.items()}))


def against_parent(parent_lib, reps, limit_s):
    """the unguarded frames on the parent's library and on this one: a child per library and round, alternated"""
    got = {"parent": {}, "this": {}}
    for _ in range(ROUNDS):
        for who, lib in (("parent", parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("NS_LIB_PATH", None)
            if lib:
                env["NS_LIB_PATH"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps), "--limit", str(limit_s)],
                               env=env, capture_output=True, text=True, timeout=120 + 40 * limit_s)
            if r.returncode != 0:
                print(json.dumps({"error": f"{who}: child exited with {r.returncode}", "tail": (r.stdout + r.stderr)[-400:]}))
                return 1                                  # nothing more is started on the GPU
            for name, rounds in json.loads(r.stdout.strip().splitlines()[-1]).items():
                got[who].setdefault(name, []).append(median(rounds))
    for name in got["this"]:
        p, t = got["parent"][name], got["this"][name]
        print(json.dumps({"what": f"unguarded frame {name}, parent against this commit", "parent_ms": [round(x, 3) for x in p],
                          "this_ms": [round(x, 3) for x in t], "parent_median_ms": round(median(p), 3),
                          "this_median_ms": round(median(t), 3), "parent_spread_ms": round(max(p) - min(p), 3),
                          "this_over_parent_pct": round(100.0 * (median(t) / median(p) - 1.0), 2)}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="frames per variant and round (the round's figure is their median)")
    ap.add_argument("--limit", type=float, default=30.0, help="seconds a single frame may take")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libnerf_sampling_hip.so: also compare the unguarded frames")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.reps, args.limit)
    import torch

    torch.cuda.set_device(0)
    res, share = measure(modules("lego_synth"), args.reps, args.limit, guarded=True)
    for name, rounds in res.items():
        med = {k: median(v) for k, v in rounds.items()}
        spread = {k: max(v) - min(v) for k, v in rounds.items()}
        print(json.dumps({"what": f"frame {name}, guard threshold {THRESHOLD}", "unguarded_ms": round(med["unguarded"], 3),
                          "every_ms": round(med["every"], 3), "selective_ms": round(med["selective"], 3),
                          "every_over_unguarded_pct": round(100.0 * (med["every"] / med["unguarded"] - 1.0), 2),
                          "selective_over_unguarded_pct": round(100.0 * (med["selective"] / med["unguarded"] - 1.0), 2),
                          "spread_ms": {k: round(v, 3) for k, v in spread.items()},
                          "rounds_ms": {k: [round(x, 3) for x in v] for k, v in rounds.items()},
                          "flagged_share": round(share[name], 4), "rounds": ROUNDS, "reps": args.reps}), flush=True)
    if args.parent_lib:
        del res
        torch.cuda.empty_cache()
        return against_parent(args.parent_lib, args.reps, args.limit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
