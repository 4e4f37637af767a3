"""bench.py --full: a plain run sets up, warms up, times its steps and prints the line; the CPU baseline, the accuracy and
scene-PSNR checks, the other configs and the API path run only with --full."""

import importlib.util
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("psnr_vs_oracle_db", "abs_err_vs_oracle", "scene_psnr", "other_configs", "api_path")


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "64", *args], env=env,
                       capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), wall


def test_full_flag(bench):
    assert bench.parse_args([]).full is False
    a = bench.parse_args(["--full", "--no-api-path"])
    assert a.full and not a.api_path and a.other_configs and not a.no_cpu_baseline


@pytest.mark.gpu
def test_plain_run_stops_at_the_line():
    """No leg beyond the timed steps, and at most 30 s of the whole process outside them."""
    out, wall = _run("--steps", "2", "--warmup", "1")
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["roofline"]["kernel_ms"] > 0
    assert out["cpu_baseline"] is None and not any(k in out for k in FULL_ONLY), sorted(out)
    assert wall - 3 * out["ms_per_step"] * 1e-3 < 30.0, wall


@pytest.mark.gpu
def test_full_run_carries_every_leg():
    out, _ = _run("--steps", "2", "--warmup", "1", "--full")
    assert out["cpu_baseline"]["value"] > 0 and all(k in out for k in FULL_ONLY), sorted(out)
    assert out["scene_psnr"]["rays"] > 0 and out["api_path"]["async_pinned"]["rays_per_s"] > 0
    assert {c["config"].split(" ")[0] for c in out["other_configs"]} == {"configs[1]", "configs[2]", "configs[4]"}
