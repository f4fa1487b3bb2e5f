"""Per-sample second moments without a GPU (include/rt_hw.h, "per-sample second moments";
raytracing-hw_amd/csrc/rt_moments.h).  The ground truth is tests/native/moments_host.cpp: the fast
colour of every sample from the kernels' own source compiled for the host, pinned here to the CPU
oracle's fast sums; on it rest the fold of squares, the host variance and relative error against a
numpy float32 restatement, and the bound on the f32 cancellation of E[x^2] - E[x]^2.  Then the
new checkpoint kind's error paths and the new entries' refusals, all before any device call."""
import ctypes
import struct

import numpy as np
import pytest

import rtref
from denoise_util import host_gbuffer, twin as gbuffer_twin
from moments_util import (MOMENT_MAGIC, arrays_of, colours, f32, moment_records, np_fold, np_mean_and_variance,
                          np_relative_error, np_variance, np_variance_records, squares, twin)
from test_accum import _load
from test_fast_accum import fast_header, fast_records

ERR_ARG, ERR_FORMAT, ERR_DEVICE = -1, -3, -4
MOMENT_SYMBOLS = ["rt_accum_create_fast_moments", "rt_accum_has_moments", "rt_accum_moments", "rt_accum_device_moments",
                  "rt_variance_from_moments", "rt_variance_from_moments_device", "rt_accum_variance",
                  "rt_accum_frame_u8_guided_measured", "rt_accum_select_variance"]
bits = rtref.bits


@pytest.fixture(scope="module")
def mh(tmp_path_factory):
    return twin(tmp_path_factory)


# ---------------------------------------------------------------- the harness, pinned to the oracle
@pytest.mark.parametrize("name,w,h,n,c", [("cornell", 33, 17, 5, 2), ("cornell", 33, 17, 7, 3), ("sponza_mini", 64, 36, 4, 2)])
def test_colours_fold_to_the_oracles_fast_sums(rt, oracle, mh, name, w, h, n, c):
    x = colours(rt, mh, name, w, h, n)
    want = oracle.render_fast(arrays_of(rt, name, w, h), n, c)[0]
    got = np_fold(x, n, c)[2]
    assert np.isfinite(want).all() and (want > 0).any()
    assert np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------- the fold of squares
def rec_words(n, total, opn):
    return np.concatenate([[np.uint32(n)], bits(total), bits(opn)]).astype(np.uint32)


@pytest.mark.parametrize("c,passes", [(3, (2, 5, 1, 4)), (1, (2, 5, 1, 4)), (8, (3, 3, 3))])
def test_fold_of_squares_over_passes(rt, mh, c, passes):
    """Pass by pass through the C text (units, `open2` carried, rtfu::fold on rtmo::square) the
    record equals the one-pass numpy fold of the squares, and open2 is zero at boundaries."""
    x = colours(rt, mh, "cornell", 33, 17, 12)
    q = squares(x)
    pixels = range(0, 33 * 17, 7)   # (every 7th pixel: the fold is per pixel)
    recs = {p: rec_words(0, np.zeros(3, f32), np.zeros(3, f32)) for p in pixels}
    n = 0
    some_open = False
    for k in passes:
        total, opn, rep = np_fold(q, n + k, c)
        for p in pixels:
            xs = np.ascontiguousarray(x[p, n:n + k])
            out = np.zeros(3, f32)
            mh.mh_fold(recs[p].ctypes.data, n + k, c, xs.ctypes.data, 1, out.ctypes.data)
            assert np.array_equal(recs[p], rec_words(n + k, total[p], opn[p])), (p, n, k, c)
            assert np.array_equal(bits(out), bits(rep[p]))
            assert (n + k) % c != 0 or not recs[p][4:7].any()
            some_open |= bool(recs[p][4:7].any())
        n += k
    assert some_open == (c != 1)


def test_fold_of_colours_is_the_fast_fold(rt, mh):
    """square = 0: the same text gives the sums' records (what the GPU tests compare sums with)."""
    x = colours(rt, mh, "cornell", 33, 17, 7)
    total, opn, rep = np_fold(x, 7, 3)
    for p in (0, 100, 560):
        rec = rec_words(0, np.zeros(3, f32), np.zeros(3, f32))
        out = np.zeros(3, f32)
        for n0, n1 in ((0, 2), (2, 7)):
            xs = np.ascontiguousarray(x[p, n0:n1])
            mh.mh_fold(rec.ctypes.data, n1, 3, xs.ctypes.data, 0, out.ctypes.data)
        assert np.array_equal(rec, rec_words(7, total[p], opn[p])) and np.array_equal(bits(out), bits(rep[p]))


# ---------------------------------------------------------------- host against numpy
def host_variance(rt, S, Q, counts_or_spp, rec, w, h):
    out = np.zeros(w * h, f32)
    counts = None if np.ndim(counts_or_spp) == 0 else np.ascontiguousarray(counts_or_spp, np.int32)
    F, I = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    S, Q, rec = (np.ascontiguousarray(a, f32) for a in (S, Q, rec))
    rc = rt.lib().rt_variance_from_moments(S.ctypes.data_as(F), Q.ctypes.data_as(F), counts.ctypes.data_as(I) if counts is not None else None,
                                           0 if counts is not None else int(counts_or_spp), w, h, rec.ctypes.data_as(F),
                                           out.ctypes.data_as(F))
    assert rc == 0, rt.lib().rt_last_error().decode()
    return out


def c_relative_error(mh, n, S, Q):
    S, Q = np.ascontiguousarray(S, f32), np.ascontiguousarray(Q, f32)
    return np.array([mh.mh_relative_error(int(n[p]), S[p].ctypes.data, Q[p].ctypes.data) for p in range(len(S))], f32)


@pytest.mark.parametrize("name,w,h,n,c", [("cornell", 33, 17, 7, 3), ("sponza_mini", 64, 36, 4, 2)])
def test_host_variance_and_relative_error_on_rendered_data(rt, mh, tmp_path_factory, name, w, h, n, c):
    x = colours(rt, mh, name, w, h, n)
    S, Q = np_fold(x, n, c)[2], np_fold(squares(x), n, c)[2]
    rec = host_gbuffer(rt, gbuffer_twin(tmp_path_factory), name, w, h)[0]
    want = np_variance_records(np.full(w * h, n), S, Q, rec)
    assert (want > 0).sum() > w * h // 4 and (want == 0).any()
    assert np.array_equal(bits(host_variance(rt, S, Q, n, rec, w, h)), bits(want))
    # counts given: a map of 0, 1, 2 and n samples (the sums and moments of those counts)
    counts = (np.arange(w * h) % 4).astype(np.int32)
    counts[counts == 3] = n
    Sm, Qm = np.zeros_like(S), np.zeros_like(Q)
    for k in (1, 2, n):
        Sm[counts == k], Qm[counts == k] = np_fold(x, k, c)[2][counts == k], np_fold(squares(x), k, c)[2][counts == k]
    want = np_variance_records(counts, Sm, Qm, rec)
    assert not want[counts < 2].any() and (want[counts >= 2] > 0).any()
    assert np.array_equal(bits(host_variance(rt, Sm, Qm, counts, rec, w, h)), bits(want))
    # python's front of the same entry
    got = rt.variance_from_moments(Sm.reshape(h, w, 3), Qm.reshape(h, w, 3), counts.reshape(h, w), rec)
    assert np.array_equal(bits(got.reshape(-1)), bits(want))
    e = c_relative_error(mh, np.full(w * h, n), S, Q)
    assert np.array_equal(bits(e), bits(np_relative_error(np.full(w * h, n), S, Q)))
    assert np.isfinite(e).all() and (e > 0).any()


def test_hand_made_rows(rt, mh):
    """n = 0, 1, 2; a miss; albedo at and below the floor; Q < S^2 / n (clamped to 0); NaN and inf in
    S and Q; V overflow -> 0."""
    nan, inf, big = f32(np.nan), f32(np.inf), f32(3e38)
    rows = [   # n, S, Q, albedo, hit
        (0, [0, 0, 0], [0, 0, 0], [0.5, 0.5, 0.5], True),
        (1, [1, 2, 3], [1, 4, 9], [0.5, 0.5, 0.5], True),
        (2, [1, 2, 3], [1, 4, 9], [0.5, 0.5, 0.5], True),
        (8, [4, 2, 1], [9, 3, 2], [0.5, 0.25, 0.75], False),                 # a miss
        (8, [4, 2, 1], [9, 3, 2], [1e-3, 5e-4, 0.0], True),                  # at and below the floor
        (8, [4, 2, 1], [9, 3, 2], [0.5, 0.25, 0.75], True),
        (4, [4, 4, 4], [3.5, 4, 3.9999], [0.5, 0.5, 0.5], True),             # Q < S^2 / n: clamped to 0
        (8, [nan, 2, 1], [9, 3, 2], [0.5, 0.5, 0.5], True),
        (8, [4, 2, 1], [9, nan, 2], [0.5, 0.5, 0.5], True),
        (8, [inf, 2, 1], [inf, 3, 2], [0.5, 0.5, 0.5], True),
        (8, [4, 2, 1], [inf, 3, 2], [0.5, 0.5, 0.5], True),
        (8, [4, 2, 1], [big, 3, 2], [1e-3, 0.5, 0.5], True),                 # V overflows: 0
        (3, [0, 0, 0], [0, 0, 0], [0.5, 0.5, 0.5], True),
    ]
    n = np.array([r[0] for r in rows], np.int32)
    S, Q, al = (np.array([r[k] for r in rows], f32) for k in (1, 2, 3))
    hit = np.array([r[4] for r in rows])
    want = np_variance(n, S, Q, al, hit)
    got = np.array([mh.mh_variance_of_mean(int(n[k]), S[k].ctypes.data, Q[k].ctypes.data, al[k].ctypes.data, int(hit[k]))
                    for k in range(len(rows))], f32)
    assert np.array_equal(bits(got), bits(want))
    assert np.isfinite(want).all() and (want >= 0).all()
    assert bits(want[[0, 1, 3, 6, 10, 11, 12]]).tolist() == [0] * 7 and want[2] > 0 and want[5] > 0
    # (a NaN channel, or inf - inf, clamps to 0 in that channel alone: the other two still count)
    assert (want[[7, 8, 9]] > 0).all() and (want[[7, 8, 9]] < want[5]).all()
    assert want[4] > want[5]   # (the floor divides by 1e-6)
    # the same rows through the library's host entry (records made of the albedo and a triangle id)
    rec = np.zeros((len(rows), 16), f32)
    rec[:, 4:7] = al
    rec.view(np.int32)[:, 7] = np.where(hit, 5, -1)
    assert np.array_equal(bits(host_variance(rt, S, Q, n, rec, len(rows), 1)), bits(want))
    # relative_error needs n >= 2
    ok = n >= 2
    e = c_relative_error(mh, n[ok], S[ok], Q[ok])
    with np.errstate(all="ignore"):
        want_e = np_relative_error(n[ok], S[ok], Q[ok])
    assert np.array_equal(bits(e), bits(want_e))
    assert np.isnan(e).any() and (e[np.isfinite(e)] >= 0).all()


def test_selection_rule(mh):
    """Steps 1 and 2 as rt_accum_select's, then n_b < 2 -> selected, else the estimate against the
    threshold; a NaN estimate is never selected."""
    S, Q = np.array([4, 2, 1], f32), np.array([9, 3, 2], f32)
    e = mh.mh_relative_error(8, S.ctypes.data, Q.ctypes.data)
    sel = lambda target=12, win=(0, 0, 0, 0), thr=0.0, x=3, y=4, mask=1, n=8, S=S, Q=Q: bool(
        mh.mh_selected(target, *win, thr, x, y, mask, n, S.ctypes.data, Q.ctypes.data))
    assert e > 0
    assert sel() and not sel(target=8) and not sel(mask=0) and not sel(win=(4, 0, 9, 9)) and sel(win=(3, 4, 4, 5))
    assert sel(thr=float(e) * 0.999) and not sel(thr=float(e)) and not sel(thr=float(e) * 1.001)
    assert sel(thr=1e30, n=0) and sel(thr=1e30, n=1) and not sel(thr=1e30, n=2)
    nanS = np.array([np.nan, 2, 1], f32)
    assert not sel(thr=1e-30, S=nanS) and sel(thr=0.0, S=nanS)


# ---------------------------------------------------------------- the cancellation bound
def test_cancellation_bound(rt, mh):
    """vm per channel (f32, from S and Q) against a float64 two-pass variance of the same samples:
    within 4 (n + 2) 2^-24 e2 r1 (each of e2 and m^2 carries at most n + 2 roundings; a factor 2
    of margin)."""
    n, c = 16, 2
    x = colours(rt, mh, "cornell", 32, 32, n)
    S, Q = np_fold(x, n, c)[2], np_fold(squares(x), n, c)[2]
    _, vm = np_mean_and_variance(np.full(len(S), n), S, Q)
    x64 = x.astype(np.float64)
    mean = x64.mean(1, keepdims=True)
    vm64 = ((x64 - mean) ** 2).sum(1) / n / (n - 1)
    e2 = (x64 ** 2).sum(1) / n
    bound = 4 * (n + 2) * 2.0 ** -24 * e2 / (n - 1)
    err = np.abs(vm.astype(np.float64) - vm64)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)
    print(f"cancellation: worst error / bound = {ratio.max():.4f} over {ratio.size} channel values")
    assert (vm64 > 0).sum() > ratio.size // 2
    assert (err <= bound).all(), f"worst error / bound = {ratio.max()}"


# ---------------------------------------------------------------- the C ABI without a device
def test_symbols_exported_and_abi_unchanged(rt):
    lib = ctypes.CDLL(rt.LIB_PATH)
    assert [s for s in MOMENT_SYMBOLS if not hasattr(lib, s)] == []
    assert set(MOMENT_SYMBOLS) <= set(rt.ABI)
    assert rt.lib().rt_abi_version() == rt.ABI_VERSION == 6
    for name in ("has_moments", "moments", "variance", "select_variance"):
        assert hasattr(rt.Accumulator, name)
    assert hasattr(rt, "variance_from_moments")


@pytest.fixture(scope="module")
def scene(rt):
    return rt.Scene.load(rtref.scene_path("cornell"), 33, 17, 3)


def _create(rt, scene, **kw):
    p = rt.RtParams(0, 0, 1, 8, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    h = ctypes.c_void_p()
    rc = rt.lib().rt_accum_create_fast_moments(scene.handle, ctypes.byref(p), ctypes.byref(h))
    return rc, h.value, rt.lib().rt_last_error().decode()


@pytest.mark.parametrize("kw,word", [(dict(count=1), "count"), (dict(kernel=4), "kernel"), (dict(flags=4), "light-split"),
                                     (dict(flags=1), "KERNEL_TIMES"), (dict(fast_chunk=-1), "fast_chunk"),
                                     (dict(flags=64), "unknown flag")])
def test_create_refusals_are_the_fast_ones(rt, scene, kw, word):
    rc, h, msg = _create(rt, scene, **kw)
    assert rc == ERR_ARG and not h
    assert word in msg and msg.startswith("rt_accum_create_fast_moments")


def test_create_without_upload_and_null_arguments(rt, scene):
    rc, h, msg = _create(rt, scene, fast_chunk=3)
    assert rc == ERR_ARG and not h and "not uploaded" in msg and msg.startswith("rt_accum_create_fast_moments")
    lib = rt.lib()
    p = rt.RtParams(0, 0, 1, 8, 0, 0, 0, 0, 0)
    h = ctypes.c_void_p()
    F = ctypes.POINTER(ctypes.c_float)
    buf = np.zeros(64, f32)
    fp = buf.ctypes.data_as(F)
    err = lambda: lib.rt_last_error().decode()
    assert lib.rt_accum_create_fast_moments(None, ctypes.byref(p), ctypes.byref(h)) == ERR_ARG
    assert lib.rt_accum_create_fast_moments(scene.handle, None, ctypes.byref(h)) == ERR_ARG
    assert lib.rt_accum_create_fast_moments(scene.handle, ctypes.byref(p), None) == ERR_ARG
    assert lib.rt_accum_has_moments(None) == 0
    assert lib.rt_accum_moments(None, fp) == ERR_ARG and err().startswith("rt_accum_moments")
    assert not lib.rt_accum_device_moments(None)
    assert lib.rt_accum_variance(None, fp) == ERR_ARG and err().startswith("rt_accum_variance")
    gp = rt.denoise_guided_params()
    out = np.zeros(12, np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert lib.rt_accum_frame_u8_guided_measured(None, ctypes.byref(gp), out) == ERR_ARG
    assert err().startswith("rt_accum_frame_u8_guided_measured")
    sel = rt.RtSelect(4, 0, 0, 0, 0, None, 0.0)
    n = ctypes.c_int64(0)
    assert lib.rt_accum_select_variance(None, ctypes.byref(sel), None, ctypes.byref(n)) == ERR_ARG
    assert err().startswith("rt_accum_select_variance") and "NULL accumulator" in err()
    assert lib.rt_accum_select_variance(None, None, None, ctypes.byref(n)) == ERR_ARG and "NULL selection" in err()
    # the variance from arrays, host and device form: the same checks before anything else
    for entry, tail in ((lib.rt_variance_from_moments, ()), (lib.rt_variance_from_moments_device, (None,))):
        args = lambda **kw: tuple(kw.get(k, d) for k, d in (("sums", fp), ("moments", fp), ("counts", None), ("spp", 2), ("w", 2),
                                                             ("h", 2), ("g", fp), ("out", fp))) + tail
        if tail:   # (ctypes: the device form takes plain pointers)
            conv = lambda a: tuple(ctypes.cast(v, ctypes.c_void_p) if isinstance(v, F) else v for v in a)
        else:
            conv = lambda a: a
        for bad in (dict(sums=None), dict(moments=None), dict(g=None), dict(out=None), dict(w=0), dict(h=-1), dict(spp=0)):
            assert entry(*conv(args(**bad))) == ERR_ARG, bad
            assert err().startswith("rt_variance_from_moments")
        assert entry(*conv(args(w=1 << 16, h=1 << 16))) == -5   # RT_ERR_LIMIT: above 2^31 pixels


# ---------------------------------------------------------------- the checkpoint file
def moment_file(view, n, samples, c, nxt=None, magic=MOMENT_MAGIC, moments=None, header_c=None, **kw):
    nxt = samples if nxt is None else nxt
    mom = moment_records(n, nxt, c) if moments is None else moments
    header = fast_header(view, n, samples, c if header_c is None else header_c, magic=magic, **kw)
    return header + fast_records(n, nxt, c).tobytes() + mom.tobytes()


def test_moment_checkpoint_error_paths(rt, scene, tmp_path):
    view, n = scene.view(), 33 * 17
    good = moment_file(view, n, 4, 3)
    assert len(good) == 128 + 64 * n and good[:8] == MOMENT_MAGIC and struct.unpack("<i", good[120:124]) == (3,)
    assert np.frombuffer(good, "<u4", 8, 128 + 32 * n)[3:6].all()   # (mid-chunk: open2 words set)
    stale = moment_records(n, 6, 3)
    stale[5, 4] = 1    # an open2 word at a chunk boundary
    padded = moment_records(n, 6, 3)
    padded[7, 6] = 1   # a pad word at a chunk boundary
    mixed_next = np.where(np.arange(n) % 3 == 0, 7, 4)
    fine = 0 if rt.device_count() > 0 else ERR_DEVICE   # (past the file checks: the first device call)
    cases = {
        "good": (good, fine),
        "good_on_a_boundary": (moment_file(view, n, 6, 3), fine),
        "per_pixel_counts": (moment_file(view, n, 7, 3, nxt=mixed_next, per_pixel=1), fine),
        "bad_magic": (moment_file(view, n, 4, 3, magic=b"RTMACCUX"), ERR_FORMAT),
        "bad_version": (moment_file(view, n, 4, 3, version=2), ERR_FORMAT),
        "fast_length": (good[:128 + 32 * n], ERR_FORMAT),          # the moment records missing
        "one_record_short": (good[:-32], ERR_FORMAT),
        "one_record_long": (good + b"\0" * 32, ERR_FORMAT),
        "chunk_zero": (moment_file(view, n, 4, 3, header_c=0), ERR_FORMAT),
        "stale_open2_words": (moment_file(view, n, 6, 3, moments=stale), ERR_FORMAT),
        "pad_words_at_a_boundary": (moment_file(view, n, 6, 3, moments=padded), ERR_FORMAT),
        "other_width": (moment_file(view, n, 4, 3, width=34), ERR_ARG),
        "other_world": (moment_file(view, n, 4, 3, world=2), ERR_ARG),
    }
    for name, (data, want) in cases.items():
        path = tmp_path / (name + ".acc")
        path.write_bytes(data)
        rc, h, msg = _load(rt, scene, path)
        assert rc == want and bool(h) == (rc == 0), (name, rc, msg)
        if rc in (ERR_FORMAT, ERR_ARG):
            assert msg.startswith("rt_accum_load"), (name, msg)
        elif rc == 0:
            assert rt.lib().rt_accum_fast_chunk(h) == 3 and rt.lib().rt_accum_has_moments(h) == 1
            rt.lib().rt_accum_free(h)


def test_record_words_rule(mh):
    z = np.zeros(8, np.uint32)
    for word in (3, 4, 5, 6, 7):
        nz = z.copy()
        nz[word] = 1
        assert not mh.mh_record_words_fit(6, 3, nz.ctypes.data) and mh.mh_record_words_fit(7, 3, nz.ctypes.data)
    total_only = z.copy()
    total_only[:3] = 5
    assert mh.mh_record_words_fit(6, 3, z.ctypes.data) and mh.mh_record_words_fit(6, 3, total_only.ctypes.data)
