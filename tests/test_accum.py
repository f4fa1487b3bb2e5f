"""Progressive rendering without a GPU: the accumulator's C ABI (include/rt_hw.h rt_accum_*),
its argument and checkpoint-file error paths (all decided before any device call), and the
chain load / store functions of rt_mega.h on the host (tests/native/accum_host.cpp): passes of
any sizes must end in the reference's own sums, bit for bit."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import rtref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the accumulator's entry points, and the harness's options and setters they run with)
SRC = [os.path.join(ROOT, "tests", "native", f) for f in ("accum_host.cpp", "kernel_host.cpp")]
ACCUM_SYMBOLS = ["rt_accum_create", "rt_accum_add", "rt_accum_samples", "rt_accum_sums", "rt_accum_device_sums",
                 "rt_accum_frame_u8", "rt_accum_state", "rt_accum_save", "rt_accum_load", "rt_accum_free"]
ERR_ARG, ERR_IO, ERR_FORMAT = -1, -2, -3


def test_symbols_exported_and_abi_unchanged(rt):
    lib = ctypes.CDLL(rt.LIB_PATH)
    assert [n for n in ACCUM_SYMBOLS if not hasattr(lib, n)] == []
    assert set(ACCUM_SYMBOLS) <= set(rt.ABI)
    assert rt.lib().rt_abi_version() == rt.ABI_VERSION == 6
    assert hasattr(rt.Scene, "accumulator") and hasattr(rt.Accumulator, "load")


@pytest.fixture(scope="module")
def scene(rt):
    return rt.Scene.load(rtref.scene_path("cornell"), 33, 17, 3)


def _create(rt, scene, **kw):
    p = rt.RtParams(0, 0, 1, 8, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    h = ctypes.c_void_p()
    rc = rt.lib().rt_accum_create(scene.handle, ctypes.byref(p), ctypes.byref(h))
    return rc, h.value, rt.lib().rt_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(flags=2), "fast"), (dict(flags=4), "light-split"), (dict(flags=1), "KERNEL_TIMES"),
    (dict(count=1), "count"), (dict(kernel=4), "kernel"), (dict(flags=8 | 32), "exclude"), (dict(flags=64), "unknown flag")])
def test_create_rejects_what_it_cannot_accumulate(rt, scene, kw, word):
    rc, h, msg = _create(rt, scene, **kw)
    assert rc == ERR_ARG and not h
    assert word in msg and msg.startswith("rt_accum_create")


def test_create_needs_an_uploaded_scene(rt, scene):
    rc, h, msg = _create(rt, scene)   # (never uploaded here: no device call is made to find that out)
    assert rc == ERR_ARG and not h and "not uploaded" in msg


def test_add_rejects_a_null_accumulator(rt):
    assert rt.lib().rt_accum_add(None, 1, None, None) == ERR_ARG
    assert rt.lib().rt_accum_samples(None) == 0


# ---------------------------------------------------------------- checkpoint file, from the documented layout
def _header(view, n_pixels, samples, rank=0, world=1, row_block=8, magic=b"RTACCUM\0", version=1, width=None):
    cam = np.concatenate([view["cam_pos"].reshape(-1), view["cam_axes"].reshape(-1), view["tan_half_fov"].reshape(-1)])
    h = magic + struct.pack("<I3i3i3Iq2i", version, width or view["width"], view["height"], view["ray_depth"], rank,
                            world, row_block, len(view["tri"]), len(view["node"]), len(view["light"]), n_pixels,
                            samples, 0)
    h += cam.astype("<f4").tobytes() + b"\0" * 8
    assert len(h) == 128
    return h


def _records(n_pixels, samples):
    rec = np.zeros((n_pixels, 8), "<u4")
    rec[:, 0] = np.arange(n_pixels)
    rec[:, 1] = samples
    rec[:, 2] = np.arange(n_pixels) + 1   # (engine state: any value below 2^31)
    return rec.tobytes()


def _load(rt, scene, path):
    h = ctypes.c_void_p()
    rc = rt.lib().rt_accum_load(scene.handle, 0, os.fsencode(str(path)), ctypes.byref(h))
    return rc, h.value, rt.lib().rt_last_error().decode()


def test_load_error_paths(rt, scene, tmp_path):
    view = scene.view()
    n = 33 * 17
    good = _header(view, n, 2) + _records(n, 2)
    cases = {
        "bad_magic": (_header(view, n, 2, magic=b"RTACCUMX") + _records(n, 2), ERR_FORMAT),
        "bad_version": (_header(view, n, 2, version=2) + _records(n, 2), ERR_FORMAT),
        "one_record_short": (good[:-32], ERR_FORMAT),
        "one_record_long": (good + b"\0" * 32, ERR_FORMAT),
        "header_only_part": (good[:100], ERR_FORMAT),
        "other_width": (_header(view, n, 2, width=34) + _records(n, 2), ERR_ARG),
        "other_rank": (_header(view, n, 2, rank=1) + _records(n, 2), ERR_ARG),
        "other_world": (_header(view, n, 2, world=2) + _records(n, 2), ERR_ARG),
    }
    rc, h, msg = _load(rt, scene, tmp_path / "missing.acc")
    assert rc == ERR_IO and not h and "missing.acc" in msg
    for name, (data, want) in cases.items():
        path = tmp_path / (name + ".acc")
        path.write_bytes(data)
        rc, h, msg = _load(rt, scene, path)
        assert (rc, bool(h)) == (want, False), (name, rc, msg)
        assert msg.startswith("rt_accum_load"), (name, msg)
    # a well-formed file of the 33 x 17 frame, loaded into a 48 x 48 scene
    other = tmp_path / "scene48.acc"
    s48 = rt.Scene.load(rtref.scene_path("cornell"), 48, 48, 3)
    other.write_bytes(good)
    rc, h, msg = _load(rt, s48, other)
    assert rc == ERR_ARG and not h and "33 x 17" in msg


def test_cli_refuses_checkpoints_of_another_scene(rt, scene, tmp_path):
    """RT_CHECKPOINT files that do not fit the scene end the run with the library's message,
    before the GPU is touched (RT_GPUS names the device count, the file is checked first)."""
    exe = os.path.join(ROOT, "raytracing-hw_amd", "rt_solution")
    prefix = str(tmp_path / "ck")
    n = 33 * 17
    with open(prefix + ".0of1", "wb") as f:
        f.write(_header(scene.view(), n, 1) + _records(n, 1))
    env = dict(os.environ, RT_GPUS="1", RT_CHECKPOINT=prefix)
    r = subprocess.run([exe, rtref.scene_path("cornell"), "48", "48", "3", str(tmp_path / "out.ppm")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "rt_accum_load" in r.stderr and "33 x 17" in r.stderr
    assert not os.path.exists(tmp_path / "out.ppm")


# ---------------------------------------------------------------- host emulation of the passes
@pytest.fixture(scope="module")
def ah(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ah") / "libah.so")
    subprocess.run(["g++", "-O2", "-fno-tree-vectorize", "-fno-tree-slp-vectorize", "-ffp-contract=off", "-fopenmp",
                    "-std=c++17", "-shared", "-fPIC", *SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    V, I = ctypes.c_void_p, ctypes.c_int
    lib.kh_accum_init.argtypes = [V, I, I, I, V]
    lib.kh_accum_init.restype = None
    lib.kh_accum_pass.argtypes = [V, I, I, I, I, I, I, I, I, V, V, V]
    lib.kh_accum_pass.restype = I
    lib.kh_set_handoff_spread.argtypes = [I]
    lib.kh_set_handoff_spread.restype = None
    return lib


def _seeds(w, h):
    p = np.arange(w * h, dtype=np.uint32)
    return np.where(p == 0, 1, p).astype(np.uint32)   # (frames below 2^31 - 1 pixels)


PASSES = [("cornell", 33, 17, 3, (1, 1, 1)), ("cornell", 64, 64, 8, (3, 1, 4)), ("sponza_mini", 64, 36, 4, (1, 3))]
# (waves, shade_min, per-pass kernel: 0 plain, 1 runahead, 2 plain + hand-off to runahead)
SCHEDULES = [(3, 16, (0, 0, 0)), (4, 8, (1, 1, 1)), (5, 16, (0, 1, 0)), (3, 16, (2, 2, 2)), (7, 1, (1, 2, 0))]


@pytest.mark.parametrize("waves,shade_min,modes", SCHEDULES)
@pytest.mark.parametrize("name,w,h,s,passes", PASSES)
def test_host_passes_match_reference(rt, ah, name, w, h, s, passes, waves, shade_min, modes):
    _check_passes(rt, ah, name, w, h, s, passes, waves, shade_min, modes)


@pytest.mark.parametrize("spread", [1, 0])
@pytest.mark.parametrize("name,w,h,s,passes", PASSES[:2])
def test_host_handoff_passes_with_and_without_spread(rt, ah, name, w, h, s, passes, spread):
    """The hand-off schedule with the resume launch's spread map (RT_HANDOFF_SPREAD: the parked
    records dealt heaviest first, one per wave) and in park-list slot order: the same sums."""
    ah.kh_set_handoff_spread(spread)
    try:
        _check_passes(rt, ah, name, w, h, s, passes, *SCHEDULES[3])
    finally:
        ah.kh_set_handoff_spread(1)


def _check_passes(rt, ah, name, w, h, s, passes, waves, shade_min, modes):
    want = rtref.golden(f"{name}_sums_{w}x{h}x{s}.rtd")["sums"].reshape(h * w, 3)
    v, keep = rt.make_view(rtref.ref_arrays(rt, name, w, h, s))
    chain = np.zeros((w * h, 8), np.uint32)
    ah.kh_accum_init(ctypes.addressof(v), 0, 1, 8, chain.ctypes.data)
    assert np.array_equal(chain[:, 0], np.arange(w * h)) and not chain[:, 1].any() and not chain[:, 3:].any()
    assert np.array_equal(chain[:, 2], _seeds(w, h))
    out = np.zeros((h * w, 3), np.float32)
    done = 0
    parked_total = 0
    for k, n in enumerate(passes):
        done += n
        parked = ctypes.c_uint64(0)
        rc = ah.kh_accum_pass(ctypes.addressof(v), done, 0, 1, 8, waves, shade_min, modes[k], 56, chain.ctypes.data,
                              out.ctypes.data, ctypes.byref(parked))
        assert rc == 0
        parked_total += parked.value
        assert np.array_equal(chain[:, 1], np.full(w * h, done, np.uint32))   # every record: next sample = samples done
        assert np.array_equal(chain[:, 0], np.arange(w * h))
        assert np.array_equal(chain[:, 4:7], rtref.bits(out))                 # the record's sum is the pixel's
        assert not chain[:, 7].any()
        if name == "cornell" and (w, h) == (64, 64) and k == 0:   # non-vacuity: the carried state is not trivial
            flag = chain[:, 2] >> 31
            assert flag.any() and not flag.all()
            assert ((chain[:, 2] & 0x7fffffff) != _seeds(w, h)).any()
    assert np.array_equal(rtref.bits(out), rtref.bits(want))
    # the hand-off took place: a pass of one sample parks nothing (every pixel ends at its first
    # sample end), one of three or more samples on the hand-off schedule has sparse tail waves
    # whose pixels end their pass in the runahead emulation
    if any(m == 2 and n >= 3 for m, n in zip(modes, passes)):
        assert parked_total > 0


def test_host_passes_shards_reassemble(rt, ah):
    name, w, h, s = "cornell", 33, 17, 3
    want = rtref.golden(f"{name}_sums_{w}x{h}x{s}.rtd")["sums"].reshape(h, w, 3)
    v, keep = rt.make_view(rtref.ref_arrays(rt, name, w, h, s))
    frame = np.zeros((h, w, 3), np.float32)
    for rank in range(3):
        rows = [r for r in range(h) if (r // 4) % 3 == rank]
        n = len(rows) * w
        chain = np.zeros((n, 8), np.uint32)
        out = np.zeros((n, 3), np.float32)
        ah.kh_accum_init(ctypes.addressof(v), rank, 3, 4, chain.ctypes.data)
        for done, mode in ((1, 1), (3, 0)):
            assert ah.kh_accum_pass(ctypes.addressof(v), done, rank, 3, 4, 2, 16, mode, 56, chain.ctypes.data,
                                    out.ctypes.data, None) == 0
        frame[rows] = out.reshape(len(rows), w, 3)
    assert np.array_equal(rtref.bits(frame), rtref.bits(want))
