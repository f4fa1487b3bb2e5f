"""Helpers of the feature-buffer and denoiser tests (test_denoise.py, test_gbuffer_host.py,
test_gpu_denoise.py): the host twin of the G-buffer kernel (tests/native/gbuffer_host.cpp), the
synthetic frames, and the numpy float32 restatement of the filter written from include/rt_hw.h."""
import ctypes
import os
import subprocess

import numpy as np

import rtref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "gbuffer_host.cpp")
GXX = ["g++", "-O2", "-fno-tree-vectorize", "-fno-tree-slp-vectorize", "-ffp-contract=off", "-fopenmp", "-std=c++17"]
f32 = np.float32
# (scene, W, H): flat faces; smooth normals; odd textures and a zfar that clips; textured and normal-mapped
FIXTURES = [("cornell", 33, 17), ("cornell_blob", 48, 48), ("texedge", 40, 24), ("sponza_mini", 64, 36)]
DEFAULTS = dict(iterations=5, sigma_color=2.0, sigma_plane=0.02, normal_power_log2=6)   # include/rt_hw.h

_twin = {}
_arrays = {}
_host_g = {}


def twin(tmp_path_factory):
    """gbuffer_host.cpp as a shared library (built once per session)."""
    if "lib" not in _twin:
        out = str(tmp_path_factory.mktemp("gh") / "libgh.so")
        subprocess.run(GXX + ["-shared", "-fPIC", SRC, "-o", out], check=True)
        lib = ctypes.CDLL(out)
        V, I = ctypes.c_void_p, ctypes.c_int
        lib.gh_gbuffer.argtypes = [V, I, I, I, V, V, V, V]
        lib.gh_gbuffer.restype = ctypes.c_longlong
        _twin["lib"] = lib
    return _twin["lib"]


def arrays_of(rt, name, w, h):
    """The reference's own flattened scene (rtref.ref_arrays), made once per frame size."""
    if (name, w, h) not in _arrays:
        _arrays[name, w, h] = rtref.ref_arrays(rt, name, w, h, 1)
    return _arrays[name, w, h]


def host_gbuffer(rt, gh, name, w, h, rank=0, world=1, row_block=8):
    """The twin's records of a shard, (pixels, 16) float32, with the rays it cast: origins and
    directions before normalisation (made once per shard; treat as read-only)."""
    key = (name, w, h, rank, world, row_block)
    if key not in _host_g:
        a = arrays_of(rt, name, w, h)
        v, keep = rt.make_view(a)
        n = len(rt.shard_rows(h, rank, world, row_block)) * w
        rec, org, dirs = np.zeros((n, 16), f32), np.zeros((n, 3), f32), np.zeros((n, 3), f32)
        bad = ctypes.c_longlong(-1)
        got = gh.gh_gbuffer(ctypes.addressof(v), rank, world, row_block, rec.ctypes.data, org.ctypes.data, dirs.ctypes.data,
                            ctypes.addressof(bad))
        del keep
        assert got == n and bad.value == 0, "the twin's exported rays are not the rays it cast"
        _host_g[key] = (rec, org, dirs)
    return _host_g[key]


def synthetic(w, h, seed=1):
    """A generated frame: a back wall (z = 4, facing the camera) over a floor (y = 1) perpendicular to
    it, a slanted plane on the right third, a block of miss pixels, per-pixel counts that include 0,
    one NaN and one inf pixel.  Returns (sums (h, w, 3), counts (h, w), records (h, w, 16), info)."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    d = np.stack([(x + 0.5) / w - 0.5, (y + 0.5) / h - 0.5, np.ones((h, w))], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    face = np.where(x >= (2 * w) // 3, 2, np.where(y >= h // 2 + 2, 1, 0))   # (the floor's rays point down)
    normals = np.array([[0, 0, -1], [0, -1, 0], [-np.sqrt(0.5), 0, -np.sqrt(0.5)]])
    offsets = np.array([-4.0, -1.0, -4.0])   # n . P = offset
    N = normals[face]
    t = offsets[face] / (N * d).sum(-1)
    P = d * t[..., None]
    albedo = np.array([[0.8, 0.7, 0.6], [0.3, 0.5, 0.2], [0.0005, 0.9, 0.4]])[face] * (0.75 + 0.25 * rng.random((h, w, 1)))
    emission = np.zeros((h, w, 3))
    emission[1:3, 2:5] = [3.0, 2.5, 2.0]
    irradiance = np.array([1.0, 0.4, 2.0])[face][..., None] * (1 + 0.6 * rng.standard_normal((h, w, 3)))
    mean = np.abs(irradiance) * albedo + emission
    counts = rng.choice([0, 1, 3, 8, 16], size=(h, w), p=[0.06, 0.2, 0.2, 0.34, 0.2]).astype(np.int32)
    miss = np.zeros((h, w), bool)
    miss[h - 4:h - 1, 1:4] = True
    miss[0, w - 1] = True
    rec = np.zeros((h, w, 16), f32)
    rec[..., 0:3], rec[..., 3], rec[..., 4:7], rec[..., 8:11], rec[..., 12:15] = N, t, albedo, emission, P
    ids = rec.view(np.int32)
    ids[..., 7] = face * 7 + (x + y) % 2
    ids[..., 11] = face
    rec[miss] = 0
    ids[miss, 7] = -1
    ids[miss, 11] = -1
    sums = (mean * counts[..., None]).astype(f32)
    sums[miss] = (f32(0.25) * counts[miss])[..., None]   # (a background the filter must pass through)
    nan_at, inf_at = (h // 3, w // 4), (h - 6, w // 2)
    for at in (nan_at, inf_at):
        assert not miss[at]
        counts[at] = 8
    sums[nan_at] = [1.0, np.nan, 2.0]
    sums[inf_at] = [np.inf, 1.0, 1.0]
    zero_at = (h // 2 - 3, w // 2 - 5)   # a hit without samples well inside the back wall
    counts[zero_at] = 0
    sums[zero_at] = 0
    return sums, counts, rec, dict(face=face, miss=miss, nan_at=nan_at, inf_at=inf_at, zero_at=zero_at)


def np_denoise(sums, counts, spp, records, iterations=5, sigma_color=2.0, sigma_plane=0.02, normal_power_log2=6):
    """The filter restated from include/rt_hw.h in numpy float32: one elementwise operation per
    step, taps in the stated order.  counts None: one spp."""
    h, w = sums.shape[:2]
    S = np.ascontiguousarray(sums, f32)
    n = np.full((h, w), spp, np.int32) if counts is None else np.asarray(counts, np.int32).reshape(h, w)
    rec = np.ascontiguousarray(records, f32).reshape(h, w, 16)
    ids = rec.view(np.int32)
    N, t, al, E, P = rec[..., 0:3], rec[..., 3], rec[..., 4:7], rec[..., 8:11], rec[..., 12:15]
    one, zero = f32(1), f32(0)
    with np.errstate(all="ignore"):
        rn = np.where(n > 0, one / np.maximum(n, 1).astype(f32), zero).astype(f32)
        m = S * rn[..., None]
        if iterations == 0:
            return m
        af = np.where(al > f32(1e-3), al, f32(1e-3)).astype(f32)
        L = (m - E) / af
        fin = np.isfinite(m).all(-1) & np.isfinite(L).all(-1)
        kind = np.where(ids[..., 7] < 0, 0, np.where(n <= 0, 2, np.where(fin, 1, 0)))
        L = np.where((kind == 1)[..., None], L, zero).astype(f32)
        b = [f32(0.375), f32(0.25), f32(0.0625)]
        for k in range(iterations):
            s = 1 << k
            sck = f32(sigma_color) * (one / f32(1 << k))
            c_k = sck * sck
            plane_den = f32(sigma_plane) * t
            sw, sL = np.zeros((h, w), f32), np.zeros((h, w, 3), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ys, xs = np.arange(h) + dy * s, np.arange(w) + dx * s
                    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
                    iy, ix = np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]
                    Lq, Nq, Pq = L[iy, ix], N[iy, ix], P[iy, ix]
                    use = inside & (kind[iy, ix] == 1) & (kind != 0)
                    hw = b[abs(dx)] * b[abs(dy)]
                    nd = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                    nd = np.where(nd > 0, nd, zero)
                    for _ in range(normal_power_log2):
                        nd = nd * nd
                    e = Pq - P
                    pd = (N[..., 0] * e[..., 0] + N[..., 1] * e[..., 1]) + N[..., 2] * e[..., 2]
                    pr = pd / plane_den
                    wp = one / (one + pr * pr)
                    dl = Lq - L
                    d2 = (dl[..., 0] * dl[..., 0] + dl[..., 1] * dl[..., 1]) + dl[..., 2] * dl[..., 2]
                    wc = np.where(kind == 1, one / (one + d2 / c_k), one)
                    wt = ((hw * nd) * wp) * wc
                    assert wt.dtype == f32
                    use = use & (wt > 0)
                    sw = np.where(use, sw + wt, sw)
                    sL = np.where(use[..., None], sL + wt[..., None] * Lq, sL)
            quo = sL / sw[..., None]
            active, some = kind != 0, sw > 0
            good = active & some & np.isfinite(quo).all(-1)
            L = np.where(good[..., None], quo, np.where((active & ~some)[..., None], zero, L)).astype(f32)
            kind = np.where(good, 1, kind)
        out = np.where((kind == 0)[..., None], m, L * af + E)
    assert out.dtype == f32
    return out
