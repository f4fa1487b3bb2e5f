"""RT_DENOISE and RT_AOV_OUT of the drop-in CLI (raytracing-hw_amd/csrc/rt_main.cpp) end to end on
the GPU: the one-shot frame and the frame in passes are the host filter's frame finished at spp 1,
and the feature images are the G-buffer's.  (With both unset the CLI's bytes are the reference's:
tests/test_dropin_cli.py.)"""
import os
import subprocess

import numpy as np
import pytest

from test_dropin_cli import SOLUTION
from test_gpu_accum import gpu   # noqa: F401  (fixture)
import rtref

pytestmark = pytest.mark.gpu
NAME, W, H, S, K = "cornell", 33, 17, 4, 3


def run(tmp_path, out, **env_more):
    env = dict(os.environ, RT_GPUS="1", **env_more)
    for k in ("RT_PASS_SPP", "RT_CHECKPOINT", "RT_ADAPT", "RT_FAST", "RT_DENOISE", "RT_AOV_OUT"):
        if k not in env_more:
            env.pop(k, None)
    r = subprocess.run([SOLUTION, rtref.scene_path(NAME), str(W), str(H), str(S), str(tmp_path / out)], env=env,
                       capture_output=True, text=True, timeout=120)
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
    return g, gpu.tonemap(gpu.denoise(sums, S, g, iterations=K), 1), gpu.tonemap(sums, S)


def test_one_shot_frame_is_denoised(tmp_path, expected):
    g, want, raw = expected
    got = run(tmp_path, "a.ppm", RT_DENOISE=str(K), RT_AOV_OUT=str(tmp_path / "aov"))
    assert np.array_equal(got, want) and (want != raw).any()
    normal = (tmp_path / "aov.normal.ppm").read_bytes()
    header = f"P6\n{W} {H}\n255\n".encode()
    assert normal.startswith(header)
    n = np.clip(g["normal"] * np.float32(0.5) + np.float32(0.5), 0, 1)
    want_n = (n * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    assert np.array_equal(np.frombuffer(normal[len(header):], np.uint8).reshape(H, W, 3), want_n)
    assert (tmp_path / "aov.albedo.ppm").read_bytes().startswith(header)
    depth = (tmp_path / "aov.depth.pgm").read_bytes()
    dh = f"P5\n{W} {H}\n65535\n".encode()
    assert depth.startswith(dh) and len(depth) == len(dh) + W * H * 2
    d = np.frombuffer(depth[len(dh):], ">u2").reshape(H, W)
    assert d.max() == 65535 and ((d == 0) == (g["depth"] == 0)).all()


def test_frame_in_passes_is_denoised(tmp_path, expected):
    _, want, _ = expected
    assert np.array_equal(run(tmp_path, "b.ppm", RT_DENOISE=str(K), RT_PASS_SPP="3"), want)


def test_bad_value_is_refused(tmp_path):
    env = dict(os.environ, RT_DENOISE="9")
    r = subprocess.run([SOLUTION, rtref.scene_path(NAME), str(W), str(H), "1", str(tmp_path / "c.ppm")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "RT_DENOISE must be 1..6" in r.stderr
