"""bench.py as a command: a plain run times the headline only, --dump-outputs writes what the
last timed frame computed, as finite values.  One tiny run (cornell 64x64x8) in a process of
its own."""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rtref

NAME, W, H, S = "cornell", 64, 64, 8


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(rtref.ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    env = dict(os.environ, RT_SCENE_DIR=str(d / "scenes"))
    p = subprocess.run([sys.executable, os.path.join(rtref.ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--scene", NAME, "--width", str(W), "--height", str(H), "--spp", str(S),
                        "--dump-outputs", str(d / "out")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), d / "out"


def test_finite_sums_keeps_finite_values_and_names_the_rest(bench):
    s = np.arange(4 * 5 * 3, dtype=np.float32).reshape(4, 5, 3) - 7.5
    s[0, 1, 0], s[1, 2, 1], s[2, 3, 2] = np.nan, np.inf, -np.inf
    s[3, 4] = [-np.inf, np.nan, np.inf]
    s[3, 0, 1] = np.float32(3.4e38)
    out, klass = bench.finite_sums(s)
    assert out.dtype == klass.dtype == np.float32 and out.shape == s.shape and klass.shape == s.shape[:2]
    assert np.isfinite(out).all() and np.isfinite(klass).all()
    fin = np.isfinite(s)
    assert np.array_equal(rtref.bits(out[fin]), rtref.bits(s[fin])) and (out[~fin] == 0).all()
    want = np.zeros((4, 5), np.float32)
    want[0, 1], want[1, 2], want[2, 3], want[3, 4] = 1, 2 * 4, 3 * 16, 3 + 1 * 4 + 2 * 16
    assert np.array_equal(klass, want)


@pytest.mark.gpu
def test_plain_line_has_the_headline_only(plain_run):
    line, _ = plain_run
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    # value = rays of the timed frames / their wall time
    rays = line["config"]["rays_per_frame"]
    assert line["value"] == pytest.approx(rays / line["ms_per_step"] / 1e3, rel=1e-3)
    assert line["natural_order"] is None and line["fast_mode"] is None and line["cpu_baseline"] is None


@pytest.mark.gpu
def test_dumped_outputs_are_the_reference_frame(rt, bench, plain_run):
    line, out = plain_run
    assert sorted(os.listdir(out)) == ["frame.npy", "sums.npy", "sums_nonfinite.npy"]
    frame, sums, klass = (np.load(out / f"{n}.npy") for n in ("frame", "sums", "sums_nonfinite"))
    assert frame.dtype == np.float32 and frame.shape == (H, W, 3)
    assert sums.dtype == np.float32 and sums.shape == (H, W, 3)
    assert klass.dtype == np.float32 and klass.shape == (H, W)
    assert np.isfinite(frame).all() and np.isfinite(sums).all() and np.isfinite(klass).all()
    g = rtref.golden(f"{NAME}_sums_{W}x{H}x{S}.rtd")
    ref, ref_klass = bench.finite_sums(g["sums"].reshape(H, W, 3))
    assert np.array_equal(rtref.bits(sums), rtref.bits(ref)) and np.array_equal(klass, ref_klass)
    assert int(g["counters"][0]) == line["config"]["rays_per_frame"]
    u8 = frame.astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), frame)
    assert hashlib.sha1(u8.tobytes()).hexdigest()[:16] == line["config"]["frame_sha1"]
    assert np.array_equal(rt.tonemap(g["sums"].reshape(H, W, 3), S), u8)
