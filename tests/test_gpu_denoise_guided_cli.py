"""RT_DENOISE_GUIDED of the drop-in CLI (raytracing-hw_amd/csrc/rt_main.cpp) end to end on the GPU:
the one-shot frame and the last frame of a run in passes are the host function's guided frame
finished at spp 1; setting it together with RT_DENOISE is refused before anything is rendered; and
with neither set the bytes are the unfiltered frame's."""
import os
import subprocess

import numpy as np
import pytest

from test_dropin_cli import SOLUTION
from test_gpu_accum import gpu   # noqa: F401  (fixture)
import rtref

pytestmark = pytest.mark.gpu
NAME, W, H, S, K = "cornell", 33, 17, 4, 5
VARS = ("RT_PASS_SPP", "RT_CHECKPOINT", "RT_ADAPT", "RT_FAST", "RT_DENOISE", "RT_DENOISE_GUIDED", "RT_AOV_OUT")


def solution(tmp_path, out, samples=S, **env_more):
    env = dict(os.environ, RT_GPUS="1", **env_more)
    for k in VARS:
        if k not in env_more:
            env.pop(k, None)
    return subprocess.run([SOLUTION, rtref.scene_path(NAME), str(W), str(H), str(samples), str(tmp_path / out)], env=env,
                          capture_output=True, text=True, timeout=120)


def run(tmp_path, out, **env_more):
    r = solution(tmp_path, out, **env_more)
    assert r.returncode == 0, r.stderr
    data = (tmp_path / out).read_bytes()
    header = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(header)
    return np.frombuffer(data[len(header):], np.uint8).reshape(H, W, 3)


@pytest.fixture(scope="module")
def expected(gpu):
    scene = gpu.Scene.load(rtref.scene_path(NAME), W, H, S)
    g = scene.gbuffer()
    sums, _ = scene.render_sums(S)
    return (gpu.tonemap(gpu.denoise_guided(sums, S, g, iterations=K), 1), gpu.tonemap(gpu.denoise(sums, S, g, iterations=K), 1),
            gpu.tonemap(sums, S))


def test_one_shot_frame_is_guided(tmp_path, expected):
    want, plain, raw = expected
    got = run(tmp_path, "a.ppm", RT_DENOISE_GUIDED=str(K))
    assert np.array_equal(got, want) and (want != raw).any() and (want != plain).any()


def test_last_frame_of_a_run_in_passes_is_guided(tmp_path, expected):
    want, _, _ = expected
    assert np.array_equal(run(tmp_path, "b.ppm", RT_DENOISE_GUIDED=str(K), RT_PASS_SPP="3"), want)


def test_both_filters_are_refused_before_rendering(tmp_path):
    for more in ({}, {"RT_PASS_SPP": "2"}):
        r = solution(tmp_path, "c.ppm", RT_DENOISE="3", RT_DENOISE_GUIDED="3", **more)
        assert r.returncode == 1 and "RT_DENOISE and RT_DENOISE_GUIDED" in r.stderr
        assert "Frame drawn" not in r.stdout and "Progress" not in r.stdout and not (tmp_path / "c.ppm").exists()
    r = solution(tmp_path, "c.ppm", RT_DENOISE_GUIDED="7")
    assert r.returncode == 1 and "RT_DENOISE_GUIDED must be 1..6" in r.stderr and not (tmp_path / "c.ppm").exists()


def test_unset_the_bytes_are_unfiltered(tmp_path, expected):
    _, _, raw = expected
    assert np.array_equal(run(tmp_path, "d.ppm"), raw)
    assert np.array_equal(run(tmp_path, "e.ppm", RT_DENOISE_GUIDED=""), raw)
