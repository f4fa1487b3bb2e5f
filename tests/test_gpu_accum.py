"""Progressive rendering on the GPU (include/rt_hw.h rt_accum_*, Scene.accumulator): passes
of any sizes, on every schedule, must leave the bits of the one-shot render of their total —
the reference's own sums (tests/golden) — and every pixel's record at the samples done."""
import os
import subprocess

import numpy as np
import pytest

import rtref
from test_gpu_parity import CASES

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_LIMIT = -1, -5
SCHEDULES = {"default": {}, "no_runahead": dict(runahead=False), "heavy": dict(heavy_order=True),
             "natural": dict(natural_order=True)}
SOLUTION = os.path.join(rtref.ROOT, "raytracing-hw_amd", "rt_solution")


@pytest.fixture(scope="module")
def gpu(rt):
    import torch   # initialises the HIP runtime librt_hw_amd.so shares (see test_gpu_parity.py)
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    if rt.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return rt


_cache = {}


def _ref_scene(gpu, name, w, h, s):
    """(scene on the reference's own flattened arrays, those arrays, golden sums), made once."""
    key = (name, w, h, s)
    if key not in _cache:
        arrays = rtref.ref_arrays(gpu, name, w, h, s)
        want = rtref.golden(f"{name}_sums_{w}x{h}x{s}.rtd")["sums"].reshape(h, w, 3)
        _cache[key] = (gpu.Scene.from_view(arrays), arrays, want)
    return _cache[key]


def _splits(s):
    out = {"ones": (1,) * s, "first": (1, s - 1)}
    if s > 2:
        out["last"] = (s - 1, 1)
    return out


def _run_passes(acc, passes):
    """Adds the passes; after each, every pixel's record must stand at the samples done."""
    done, stats = acc.samples, []
    for n in passes:
        stats.append(acc.add(n))
        done += n
        assert acc.samples == done
        nxt = acc.state()[:, 0]
        behind = np.nonzero(nxt != done)[0]
        assert behind.size == 0, f"{behind.size} records not at sample {done} (first: pixel {behind[:4]}, at {nxt[behind[:4]]})"
        assert stats[-1]["samples"] == stats[-1]["pixels"] * n
    return stats


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("name,w,h,s,split", [c + (k,) for c in CASES for k in _splits(c[3])])
def test_passes_match_reference(gpu, name, w, h, s, split, sched):
    scene, _, want = _ref_scene(gpu, name, w, h, s)
    acc = scene.accumulator(**SCHEDULES[sched])
    assert acc.samples == 0 and not acc.sums().any()
    _run_passes(acc, _splits(s)[split])
    got = acc.sums()
    bad = (rtref.bits(got) != rtref.bits(want)).any(2)
    assert bad.sum() == 0, f"{bad.sum()} pixels differ, max |d| {np.abs(got - want).max()}"
    acc.free()


def test_intermediate_passes_are_real_frames(gpu, oracle):
    scene, arrays, want8 = _ref_scene(gpu, "cornell", 64, 64, 8)
    acc = scene.accumulator()
    _run_passes(acc, (3,))
    want3, _, _ = oracle.render(arrays, 3)
    got3 = acc.sums()
    assert np.array_equal(rtref.bits(got3.reshape(-1, 3)), rtref.bits(want3))
    assert np.array_equal(acc.frame(), gpu.tonemap(want3.reshape(64, 64, 3), 3))
    st = acc.state()   # the carried state is not trivial: both cache flags occur, engines have moved
    assert st[:, 2].any() and not st[:, 2].all() and set(np.unique(st[:, 2])) <= {0, 1}
    assert (st[:, 1] != np.maximum(np.arange(64 * 64), 1)).any()
    _run_passes(acc, (5,))
    assert np.array_equal(rtref.bits(acc.sums()), rtref.bits(want8))
    assert acc.device_sums_ptr != 0


def test_runahead_kernel_throughout(gpu):
    """cornell 512x512: 16 + 48 samples against the reference's own row hashes of the 64-spp frame."""
    g = rtref.golden("cornell_512x512x64_rowhash.rtd")
    scene = gpu.Scene.load(rtref.scene_path("cornell"), 512, 512, 64)
    acc = scene.accumulator()
    stats = _run_passes(acc, (16, 48))
    assert [st["schedule"] for st in stats] == [gpu.SCHED_RUNAHEAD] * 2
    out = acc.sums()
    bad = np.nonzero(rtref.row_hash(out) != g["row_fnv1a"])[0]
    assert bad.size == 0, f"rows {bad[:8]} differ"
    assert np.array_equal(rtref.bits(out[g["rows"]]), rtref.bits(g["row_sums"]))


@pytest.fixture(scope="module")
def handoff_ref(gpu, oracle):
    """sponza_mini 1280x720 (the smallest frame the suite uses for the hand-off schedule): the
    one-shot 6-spp frame on the existing path without runahead, and the CPU oracle's sums of 10
    seeded pixels, each made once."""
    scene = gpu.Scene.load(rtref.scene_path("sponza_mini"), 1280, 720, 6)
    want, st = scene.render_sums(6, runahead=False)
    assert st["schedule"] == gpu.SCHED_LANE
    arrays = scene.view()
    pix = np.random.default_rng(17).choice(1280 * 720, 10, replace=False)
    ref = {int(p): oracle.render(arrays, 6, int(p), int(p) + 1, threads=1)[0][0] for p in pix}
    return scene, want, ref


@pytest.mark.parametrize("order", ["natural", "heavy"])
def test_plain_kernel_and_handoff(gpu, handoff_ref, order):
    scene, want, ref = handoff_ref
    acc = scene.accumulator(natural_order=order == "natural", heavy_order=order == "heavy")
    stats = _run_passes(acc, (1, 2, 3))
    assert [st["schedule"] for st in stats] == [gpu.SCHED_LANE | gpu.SCHED_RUNAHEAD] * 3
    got = acc.sums()
    bad = (rtref.bits(got) != rtref.bits(want)).any(2)
    assert bad.sum() == 0, f"{bad.sum()} pixels differ from the one-shot render"
    for p, r in ref.items():
        assert np.array_equal(rtref.bits(got.reshape(-1, 3)[p]), rtref.bits(r)), f"pixel {p}"
    acc.free()


@pytest.mark.parametrize("world", [2, 3])
def test_shards_reassemble(gpu, world):
    scene, _, want = _ref_scene(gpu, "cornell", 33, 17, 3)
    frame = np.zeros((17, 33, 3), np.float32)
    for rank in range(world):
        acc = scene.accumulator(rank=rank, world=world, row_block=4)
        _run_passes(acc, (1, 2))
        rows = gpu.shard_rows(17, rank, world, 4)
        assert np.array_equal(rows, acc.rows)
        frame[rows] = acc.sums()
    assert np.array_equal(rtref.bits(frame), rtref.bits(want))


def test_save_and_load(gpu, tmp_path):
    scene, arrays, want = _ref_scene(gpu, "cornell", 64, 64, 8)
    path = str(tmp_path / "cornell.acc")
    acc = scene.accumulator()
    _run_passes(acc, (3,))
    before = acc.sums()
    acc.save(path)
    acc.free()
    assert os.path.getsize(path) == 128 + 64 * 64 * 32
    acc = gpu.Accumulator.load(scene, path)
    assert acc.samples == 3 and (acc.rank, acc.world, acc.row_block) == (0, 1, 8)
    assert np.array_equal(rtref.bits(acc.sums()), rtref.bits(before))
    _run_passes(acc, (5,))
    assert np.array_equal(rtref.bits(acc.sums()), rtref.bits(want))
    other = gpu.Scene.load(rtref.scene_path("cornell"), 48, 48, 8)
    with pytest.raises(gpu.RtError, match="64 x 64"):
        gpu.Accumulator.load(other, path)
    import ctypes
    h = ctypes.c_void_p()
    assert gpu.lib().rt_accum_load(other.handle, 0, os.fsencode(path), ctypes.byref(h)) == ERR_ARG and not h.value


def test_limits(gpu):
    scene, _, _ = _ref_scene(gpu, "cornell", 33, 17, 3)
    acc = scene.accumulator()
    lib = gpu.lib()
    assert lib.rt_accum_add(acc._h, 0, None, None) == ERR_ARG
    assert lib.rt_accum_add(acc._h, -3, None, None) == ERR_ARG
    assert lib.rt_accum_add(acc._h, 1 << 20, None, None) == ERR_LIMIT   # (refused before any launch)
    assert acc.samples == 0
    acc.add(1)
    assert lib.rt_accum_add(acc._h, (1 << 20) - 1, None, None) == ERR_LIMIT
    assert acc.samples == 1 and (acc.state()[:, 0] == 1).all()
    with pytest.raises(gpu.RtError):
        acc.add(0)


# ---------------------------------------------------------------- CLI
def _cli(out, samples, **env_add):
    env = dict(os.environ)
    for k in ("RT_PASS_SPP", "RT_CHECKPOINT"):
        env.pop(k, None)
    env["RT_GPUS"] = "1"
    env.update(env_add)
    r = subprocess.run([SOLUTION, rtref.scene_path("cornell"), "33", "17", str(samples), out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_passes_write_reference_ppm(tmp_path):
    want = open(os.path.join(rtref.GOLD, "cornell_33x17x3.ppm"), "rb").read()
    out = str(tmp_path / "out.ppm")
    stdout = _cli(out, 3, RT_PASS_SPP="1")
    assert [l for l in stdout.splitlines() if l.startswith("Progress: ")] == [f"Progress: {k} / 3 samples" for k in (1, 2, 3)]
    assert open(out, "rb").read() == want


def test_cli_checkpoint_resumes(tmp_path):
    """The first run is limited to one pass by asking for 1 sample with the prefix; the second
    asks for 3 with the same prefix and resumes from the files of the first."""
    want = open(os.path.join(rtref.GOLD, "cornell_33x17x3.ppm"), "rb").read()
    out, prefix = str(tmp_path / "out.ppm"), str(tmp_path / "ck")
    first = _cli(out, 1, RT_CHECKPOINT=prefix)
    assert "Resumed" not in first and os.path.exists(prefix + ".0of1")
    assert open(out, "rb").read() != want
    second = _cli(out, 3, RT_CHECKPOINT=prefix, RT_PASS_SPP="1")
    assert "Resumed from" in second and "at 1 samples" in second
    assert [l for l in second.splitlines() if l.startswith("Progress: ")] == ["Progress: 2 / 3 samples", "Progress: 3 / 3 samples"]
    assert open(out, "rb").read() == want
