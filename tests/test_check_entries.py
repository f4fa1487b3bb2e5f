"""The argument and refusal behaviour of the test entries (rt_device_selfcheck, rt_intersect_rays,
rt_intersect_rays_via, rt_sample_frames_via; csrc/rt_check_device.h) on the host: codes, texts and their order, and that
a failing call leaves the caller's `mismatches` word alone.  No GPU is needed: every refusal comes
before any device work, and where no device is visible the device work fails loudly
(RT_ERR_DEVICE) instead of computing anything elsewhere."""
import ctypes

import numpy as np
import pytest

import rtref

RT_OK, RT_ERR_ARG, RT_ERR_DEVICE = 0, -1, -4
_c_i64 = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def scene(rt):
    return rt.Scene.load(rtref.scene_path("cornell"), 8, 8, 1)


def selfcheck(rt, which, out=True):
    """(code, last error, the mismatches word after the call; it is preset to 7)."""
    n = ctypes.c_uint64(7)
    rc = rt.lib().rt_device_selfcheck(which, ctypes.byref(n) if out else None)
    return rc, rt.lib().rt_last_error().decode(), int(n.value)


def rays_via(rt, handle, path, n, org=True, dirs=True):
    """(code, last error) of rt_intersect_rays_via over max(n, 1) rays' worth of buffers."""
    m = max(int(n), 1)
    o = np.zeros((m, 3), np.float32)
    d = np.tile(np.float32([0, 0, -1]), (m, 1))
    f, i = np.zeros((m, 4), np.float32), np.zeros((m, 6), np.int64)
    rc = rt.lib().rt_intersect_rays_via(handle, path, n, o.ctypes.data_as(rt._c_f) if org else None,
                                        d.ctypes.data_as(rt._c_f) if dirs else None, f.ctypes.data_as(rt._c_f),
                                        i.ctypes.data_as(_c_i64))
    return rc, rt.lib().rt_last_error().decode()


@pytest.mark.parametrize("which", [-1, 6])
def test_unknown_check_is_refused(rt, which):
    assert selfcheck(rt, which) == (RT_ERR_ARG, f"rt_device_selfcheck: unknown check {which}", 7)


def test_null_output_is_refused(rt):
    assert selfcheck(rt, 0, out=False)[:2] == (RT_ERR_ARG, "rt_device_selfcheck: null output")


@pytest.mark.parametrize("path,n", [(3, 0), (-1, 4)])
def test_unknown_path_comes_before_the_empty_query(rt, scene, path, n):
    assert rays_via(rt, scene.handle, path, n) == (RT_ERR_ARG, f"rt_intersect_rays_via: unknown path {path}")


@pytest.mark.parametrize("path", [0, 2])
def test_empty_query_needs_no_device(rt, scene, path):
    assert rays_via(rt, scene.handle, path, 0)[0] == RT_OK


@pytest.mark.parametrize("case", ["null scene", "negative n", "null origins"])
def test_bad_argument_is_refused(rt, scene, case):
    handle = None if case == "null scene" else scene.handle
    got = rays_via(rt, handle, 0, -1 if case == "negative n" else 4, org=case != "null origins")
    assert got == (RT_ERR_ARG, "rt_intersect_rays: bad argument")


def frames_via(rt, handle, path, n, seed=1, warm=0, frames=True, bad_row=None):
    """(code, last error, the outputs' first words; they are preset to 7) of rt_sample_frames_via over
    max(n, 1) frames' worth of buffers; bad_row: the only row that holds `seed` and `warm`."""
    m = max(int(n), 1)
    fr = np.tile(np.float32([0, 0, 0, 0, 1, 0, 0, 1, 0, 0.25]), (m, 1))
    sd, wm = np.full(m, 1 if bad_row is not None else seed, np.uint32), np.full(m, 0 if bad_row is not None else warm, np.uint32)
    if bad_row is not None:
        sd[bad_row], wm[bad_row] = seed, warm
    f, i = np.full((m, 6), 7, np.float32), np.full((m, 4), 7, np.int64)
    c_u = ctypes.POINTER(ctypes.c_uint32)
    rc = rt.lib().rt_sample_frames_via(handle, path, n, fr.ctypes.data_as(rt._c_f) if frames else None, sd.ctypes.data_as(c_u),
                                       wm.ctypes.data_as(c_u), f.ctypes.data_as(rt._c_f), i.ctypes.data_as(_c_i64))
    return rc, rt.lib().rt_last_error().decode(), (float(f[0, 0]), int(i[0, 0]))


@pytest.mark.parametrize("case", ["null scene", "negative n", "null frames"])
def test_frames_bad_argument_is_refused(rt, scene, case):
    handle = None if case == "null scene" else scene.handle
    got = frames_via(rt, handle, 0, -1 if case == "negative n" else 4, frames=case != "null frames")
    assert got == (RT_ERR_ARG, "rt_sample_frames_via: bad argument", (7.0, 7))


@pytest.mark.parametrize("path,n", [(2, 0), (-1, 4)])
def test_frames_unknown_path_comes_before_the_empty_query(rt, scene, path, n):
    assert frames_via(rt, scene.handle, path, n)[:2] == (RT_ERR_ARG, f"rt_sample_frames_via: unknown path {path}")


@pytest.mark.parametrize("path", [0, 1])
def test_frames_empty_query_needs_no_device(rt, scene, path):
    assert frames_via(rt, scene.handle, path, 0)[0] == RT_OK


@pytest.mark.parametrize("seed", [0, 2147483647, 0xffffffff])
def test_frames_seed_outside_the_engine_range_is_refused(rt, scene, seed):
    """(on a state of 0 the polar loop would never end: refused on the host, before any device work)"""
    got = frames_via(rt, scene.handle, 1, 5, seed=seed, bad_row=3)
    assert got == (RT_ERR_ARG, "rt_sample_frames_via: seed of frame 3 is outside 1 .. 2147483646", (7.0, 7))


def test_frames_warm_above_one_is_refused(rt, scene):
    got = frames_via(rt, scene.handle, 0, 5, warm=2, bad_row=4)
    assert got == (RT_ERR_ARG, "rt_sample_frames_via: warm of frame 4 is neither 0 nor 1", (7.0, 7))


def test_frames_seed_comes_before_warm_and_path_before_both(rt, scene):
    assert frames_via(rt, scene.handle, 0, 2, seed=0, warm=2, bad_row=1)[1] == "rt_sample_frames_via: seed of frame 1 is outside 1 .. 2147483646"
    assert frames_via(rt, scene.handle, 5, 2, seed=0, warm=2, bad_row=1)[1] == "rt_sample_frames_via: unknown path 5"


def test_frames_query_without_a_device_fails_loudly(rt, scene):
    if rt.device_count() != 0:
        return
    rc, text, first = frames_via(rt, scene.handle, 1, 4)
    assert rc == RT_ERR_DEVICE and text and first == (7.0, 7)


@pytest.mark.parametrize("which", [4, 5])
def test_scene_checks_without_a_scene(rt, which):
    if rt.device_count() != 0:   # (a process with a GPU may hold scenes other tests uploaded)
        return
    assert selfcheck(rt, which) == (RT_ERR_ARG, f"rt_device_selfcheck {which}: no scene is uploaded", 7)


@pytest.mark.parametrize("which", [0, 2])
def test_checks_without_a_device_fail_loudly(rt, which):
    if rt.device_count() != 0:
        return
    rc, text, n = selfcheck(rt, which)
    assert rc == RT_ERR_DEVICE and text and n == 7


def test_query_without_a_device_fails_loudly(rt, scene):
    if rt.device_count() != 0:
        return
    rc, text = rays_via(rt, scene.handle, 1, 4)
    assert rc == RT_ERR_DEVICE and text
