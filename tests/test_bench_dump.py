"""bench.py --dump-outputs: the frame of the last timed step as .npy files, so that two builds can be compared output for
output.  The writer and the flags are checked on the CPU; one GPU test runs bench.py with the flag and compares the files
with a direct render of the same pose."""

import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _frame(H, W):
    """rgb / disp whose values name their pixel: rgb[..., c] = 3 * pixel + c, disp = pixel."""
    pix = np.arange(H * W, dtype=np.float32).reshape(H, W)
    return np.stack([3 * pix, 3 * pix + 1, 3 * pix + 2], -1), pix


def test_flags(bench):
    a = bench.parse_args(["--steps", "7", "--warmup", "2", "--dump-outputs", "out"])
    assert a.steps == 7 and a.warmup == 2 and a.dump_outputs == "out"
    assert bench.parse_args([]).dump_outputs is None
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_whole_frame(bench, tmp_path):
    rgb, disp = _frame(6, 5)
    info = bench.dump_outputs(str(tmp_path), rgb.astype(np.float64), disp)
    got_rgb, got_disp = np.load(tmp_path / "rgb.npy"), np.load(tmp_path / "disp.npy")
    assert got_rgb.dtype == got_disp.dtype == np.float32
    np.testing.assert_array_equal(got_rgb, rgb)
    np.testing.assert_array_equal(got_disp, disp)
    assert info["files"] == {"rgb": [6, 5, 3], "disp": [6, 5]} and info["pixels"] == info["of_pixels"] == 30


def test_dump_samples_a_large_frame_under_the_budget(bench, tmp_path):
    """A 2048 x 2048 frame is 67 MB: cut to one fixed sample of pixels, the same in both files and from run to run."""
    rgb, disp = _frame(2048, 2048)
    infos = [bench.dump_outputs(str(tmp_path / d), rgb, disp) for d in ("a", "b")]
    sizes = [os.path.getsize(tmp_path / "a" / f) for f in ("rgb.npy", "disp.npy")]
    assert sum(sizes) <= 64_000_000 and sum(sizes) > 63_000_000
    a_rgb, a_disp = np.load(tmp_path / "a" / "rgb.npy"), np.load(tmp_path / "a" / "disp.npy")
    assert a_rgb.shape == (infos[0]["pixels"], 3) and infos[0]["of_pixels"] == 2048 * 2048
    assert (np.diff(a_disp) > 0).all()                             # distinct pixels, row-major order
    np.testing.assert_array_equal(a_rgb, rgb.reshape(-1, 3)[a_disp.astype(np.int64)])
    np.testing.assert_array_equal(a_rgb, np.load(tmp_path / "b" / "rgb.npy"))
    np.testing.assert_array_equal(a_disp, np.load(tmp_path / "b" / "disp.npy"))


@pytest.mark.gpu
def test_bench_dumps_its_last_timed_frame(bench, tmp_path):
    """bench.py --steps 3 --warmup 2 --dump-outputs DIR: the JSON line carries steps / ms_per_step, and DIR holds the frame
    of pose (2 + 3 - 1) -- bit for bit what the one-kernel renderer gives for that pose with the same weights."""
    import torch

    from nerf_sampling_amd import ops, synthetic

    size, out_dir = 64, str(tmp_path / "dump")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", str(size), "--steps", "3",
                        "--warmup", "2", "--no-cpu-baseline", "--dump-outputs", out_dir], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["dumped_outputs"]["pose"] == 4
    got_rgb, got_disp = np.load(os.path.join(out_dir, "rgb.npy")), np.load(os.path.join(out_dir, "disp.npy"))
    assert got_rgb.shape == (size, size, 3) and got_disp.shape == (size, size)

    torch.cuda.set_device(0)
    _, fine, dn, _ = bench.build_modules("shapes_fit", torch.device("cuda", 0))
    ops.set_compute_dtype("bf16")
    nerf_w, depth_w = fine.packed("bf16"), dn.packed()
    ops.set_compute_dtype("f32")
    _, K = synthetic.blender_intrinsics(size, size)
    c2w = synthetic.render_poses(40)[4, :3, :4]
    exp = ops.render_rays_depthnet(depth_w, nerf_w, camera=(size, size, K, c2w, 0, size), n_samples=64, mode="uniform",
                                   std=0.1, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got_rgb.reshape(-1, 3), exp["rgb"].cpu().numpy())
    np.testing.assert_array_equal(got_disp.reshape(-1), exp["disp"].cpu().numpy())
