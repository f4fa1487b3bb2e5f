"""Helpers of the moments tests (test_moments.py, test_gpu_moments.py): the CPU ground truth
(tests/native/moments_host.cpp: the fast colour of every sample from the kernels' own source
compiled for the host), the fast fold restated in numpy, and the numpy float32 restatement of
raytracing-hw_amd/csrc/rt_moments.h written from include/rt_hw.h."""
import ctypes
import os
import subprocess

import numpy as np

import rtref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "moments_host.cpp")
GXX = ["g++", "-O2", "-fno-tree-vectorize", "-fno-tree-slp-vectorize", "-ffp-contract=off", "-fopenmp", "-std=c++17"]
f32 = np.float32
MOMENT_MAGIC = b"RTMACCUM"

_twin, _arrays, _colours = {}, {}, {}


def twin(tmp_path_factory):
    """moments_host.cpp as a shared library (built once per session)."""
    if "lib" not in _twin:
        out = str(tmp_path_factory.mktemp("mh") / "libmh.so")
        subprocess.run(GXX + ["-shared", "-fPIC", SRC, "-o", out], check=True)
        lib = ctypes.CDLL(out)
        V, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        lib.mh_colours.argtypes = [V, L, L, I, I, V]
        lib.mh_colours.restype = None
        lib.mh_fold.argtypes = [V, I, I, V, I, V]
        lib.mh_fold.restype = None
        lib.mh_variance_of_mean.argtypes = [I, V, V, V, I]
        lib.mh_variance_of_mean.restype = ctypes.c_float
        lib.mh_relative_error.argtypes = [I, V, V]
        lib.mh_relative_error.restype = ctypes.c_float
        lib.mh_mean_and_variance.argtypes = [I, V, V, V, V]
        lib.mh_mean_and_variance.restype = None
        lib.mh_selected.argtypes = [I, I, I, I, I, ctypes.c_float, I, I, ctypes.c_uint, I, V, V]
        lib.mh_record_words_fit.argtypes = [ctypes.c_uint, I, V]
        _twin["lib"] = lib
    return _twin["lib"]


def arrays_of(rt, name, w, h):
    """The reference's own flattened scene (rtref.ref_arrays), made once per frame size."""
    if (name, w, h) not in _arrays:
        _arrays[name, w, h] = rtref.ref_arrays(rt, name, w, h, 4)
    return _arrays[name, w, h]


def colours(rt, mh, name, w, h, n, arrays=None):
    """The fast colours of samples [0, n) of every frame pixel, (H * W, n, 3) float32: made once
    per frame for the largest n asked so far, never changed."""
    key = (name, w, h)
    have = _colours.get(key)
    if have is None or have.shape[1] < n:
        a = arrays if arrays is not None else arrays_of(rt, name, w, h)
        v, keep = rt.make_view(a)
        out = np.zeros((w * h, n, 3), f32)
        mh.mh_colours(ctypes.addressof(v), 0, w * h, 0, n, out.ctypes.data)
        del keep
        out.setflags(write=False)
        _colours[key] = have = out
    return have[:, :n]


def np_fold(x, n, c):
    """The fast fold of x[:, :n] ((P, >= n, 3) float32) in chunks of c, vectorised over the
    pixels: (total, open, reported), each (P, 3).  Chunk partials in sample order from +0.f, the
    chunk partials in chunk order from +0.f, a ragged last chunk kept apart as `open`."""
    P = x.shape[0]
    total, opn = np.zeros((P, 3), f32), np.zeros((P, 3), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, n - n % c, c):
            part = np.zeros((P, 3), f32)
            for s in range(c0, c0 + c):
                part = part + x[:, s]
            total = total + part
        if n % c == 0:
            return total, opn, total
        for s in range(n - n % c, n):
            opn = opn + x[:, s]
        rep = total + opn
    assert rep.dtype == f32
    return total, opn, rep


def squares(x):
    with np.errstate(invalid="ignore", over="ignore"):
        q = x * x
    assert q.dtype == f32
    return q


def np_mean_and_variance(n, S, Q):
    """Per channel m and vm for n >= 2 (rows with n < 2 hold values nobody may use)."""
    n = np.asarray(n, np.int32)
    safe = np.maximum(n, 2)
    with np.errstate(all="ignore"):
        r = (f32(1) / safe.astype(f32))[..., None]
        r1 = (f32(1) / (safe - 1).astype(f32))[..., None]
        m = S * r
        e2 = Q * r
        v = e2 - m * m
        v = np.where(v > 0, v, f32(0)).astype(f32)
        vm = v * r1
    assert m.dtype == f32 and vm.dtype == f32
    return m, vm


def np_variance(n, S, Q, albedo, hit):
    """variance_of_mean restated: n (P,), S, Q, albedo (P, 3), hit (P,) bool -> (P,) float32."""
    n = np.asarray(n, np.int32)
    _, vm = np_mean_and_variance(n, S, Q)
    with np.errstate(all="ignore"):
        a = np.where(albedo > f32(1e-3), albedo, f32(1e-3)).astype(f32)
        d = vm / (a * a)
        V = (d[..., 0] + d[..., 1]) + d[..., 2]
    assert V.dtype == f32
    V = np.where(np.isfinite(V), V, f32(0))
    return np.where(hit & (n >= 2), V, f32(0)).astype(f32)


def np_relative_error(n, S, Q):
    """relative_error restated, (P,) float32 (rows with n < 2 hold values nobody may use)."""
    m, vm = np_mean_and_variance(n, S, Q)
    with np.errstate(all="ignore"):
        num = (np.sqrt(vm[..., 0]) + np.sqrt(vm[..., 1])) + np.sqrt(vm[..., 2])
        e = num / np.sqrt(((m[..., 0] + m[..., 1]) + m[..., 2]) + f32(1e-4))
    assert e.dtype == f32
    return e


def np_variance_records(n, S, Q, rec):
    """np_variance on first-hit records ((P, 16) float32: albedo words 4-6, triangle id word 7)."""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 16)
    return np_variance(n, S, Q, rec[:, 4:7], rec.view(np.int32)[:, 7] >= 0)


def moment_records(n_pixels, nxt, c):
    """Hand-made moment records (total2 x y z, open2 x y z, 0, 0); open2 only where a chunk is open."""
    rec = np.zeros((n_pixels, 8), "<u4")
    rec[:, 0:3] = rtref.bits(np.full((n_pixels, 3), 2.25, f32))
    is_open = (np.broadcast_to(np.asarray(nxt), (n_pixels,)) % c) != 0
    rec[is_open, 3:6] = rtref.bits(np.full((int(is_open.sum()), 3), 0.0625, f32))
    return rec
