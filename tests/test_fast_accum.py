"""Fast-mode accumulators without a GPU (include/rt_hw.h rt_accum_create_fast): the unit
arithmetic and the fold of raytracing-hw_amd/csrc/rt_fast_units.h (behind
tests/native/fast_units_host.cpp) against a numpy restatement of the oracle's chunked sum, the
launch plan of a fast pass, and the new entry's refusals and checkpoint-file error paths, all
decided before any device call."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import rtref
from test_accum import _header, _load
from plan_util import PlanIn, PlanOut
from test_launch_plan import PLAIN_BLOCKS, SPEC_BLOCKS, HD, SRC as PLAN_SRC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "fast_units_host.cpp")
GXX = ["g++", "-O2", "-fno-tree-vectorize", "-fno-tree-slp-vectorize", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wextra"]
ERR_ARG, ERR_FORMAT, ERR_DEVICE = -1, -3, -4
SCHED_FAST = 4
F_FAST, F_LSPLIT, F_NATURAL, F_NO_RUNAHEAD, F_HEAVY, F_KERNEL_TIMES = 2, 4, 8, 16, 32, 1
FAST_SYMBOLS = ["rt_accum_create_fast", "rt_accum_fast_chunk"]
FAST_MAGIC = b"RTFACCUM"
f32 = np.float32
CHUNKS = (1, 2, 3, 8)
N_MAX = 20


FuIn = PlanIn   # (one pair of structures for every plan shim: plan_util.py)


@pytest.fixture(scope="module")
def fu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fu") / "libfu.so")
    subprocess.run(GXX + ["-shared", "-fPIC", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    I, V = ctypes.c_int, ctypes.c_void_p
    lib.fu_units_of.argtypes = [I, I, I]
    lib.fu_unit_range.argtypes = [I, I, I, I, V, V]
    lib.fu_unit_range.restype = None
    lib.fu_unit_continues.argtypes = [I, I, I]
    lib.fu_fold.argtypes = [V, I, I, V, V]
    lib.fu_fold.restype = None
    lib.fu_open_words_fit.argtypes = [ctypes.c_uint, I, V]
    lib.fu_plan.argtypes = [ctypes.POINTER(FuIn), ctypes.POINTER(PlanOut)]
    return lib


# ---------------------------------------------------------------- the numpy restatement
def samples():
    """N_MAX synthetic per-sample colours (f32 x 3) with a -0.f and a NaN among them, and values
    whose sums round differently in different association orders."""
    rng = np.random.default_rng(5)
    v = (rng.random((N_MAX, 3)) * 10.0 ** rng.integers(-3, 4, (N_MAX, 3))).astype(f32)
    v[0] = f32(-0.0)            # (a chunk of -0.f alone: its partial is +0.f + -0.f = +0.f)
    v[7, 1] = f32(-0.0)
    v[13, 2] = f32(np.nan)      # (everything from chunk 13 // c on is NaN in that channel)
    return v


def partial(v, s0, s1, start=None):
    """Samples [s0, s1) added in order onto `start` (+0.f), f32."""
    part = np.zeros(3, f32) if start is None else np.array(start, f32)
    with np.errstate(invalid="ignore"):
        for s in range(s0, s1):
            part = (part + v[s]).astype(f32)
    return part


def oracle_record(v, n, c):
    """(total, open, reported) of a pixel with n samples in chunks of c: rt_oracle_render_fast's
    loop (oracle/rt_oracle.cpp render_pixel_fast), keeping the ragged last chunk apart."""
    total = np.zeros(3, f32)
    with np.errstate(invalid="ignore"):
        for c0 in range(0, n - n % c, c):
            total = (total + partial(v, c0, c0 + c)).astype(f32)
        if n % c == 0:
            return total, np.zeros(3, f32), total
        opn = partial(v, n - n % c, n)
        return total, opn, (total + opn).astype(f32)


def rec_words(n, total, opn):
    return np.concatenate([[np.uint32(n)], rtref.bits(total), rtref.bits(opn)]).astype(np.uint32)


def c_pass(fu, v, rec, target, c):
    """One pass [rec.next, target) through the C text: the units' partials as the render kernel
    makes them (unit_range, unit 0 started from `open` where unit_continues says so), then fold.
    Returns (record words, reported sum, the ranges)."""
    nxt = int(rec[0])
    K = fu.fu_units_of(nxt, target, c)
    parts = np.zeros((max(K, 1), 3), f32)
    ranges = []
    for k in range(K):
        s0, s1 = ctypes.c_int(), ctypes.c_int()
        fu.fu_unit_range(nxt, target, c, k, ctypes.addressof(s0), ctypes.addressof(s1))
        ranges.append((s0.value, s1.value))
        start = rec[4:7].view(f32) if fu.fu_unit_continues(nxt, c, k) else None
        parts[k] = partial(v, s0.value, s1.value, start)
    out = rec.copy()
    rep = np.zeros(3, f32)
    fu.fu_fold(out.ctypes.data, target, c, parts.ctypes.data, rep.ctypes.data)
    return out, rep, ranges


@pytest.mark.parametrize("c", CHUNKS)
def test_units_and_fold_match_numpy(fu, c):
    v = samples()
    for nxt in range(N_MAX):
        rec = rec_words(nxt, *oracle_record(v, nxt, c)[:2])
        for target in range(nxt + 1, N_MAX + 1):
            # the chunks [next, target) overlaps, by brute force
            want = [(max(nxt, j * c), min(target, (j + 1) * c)) for j in range(N_MAX // c + 2)
                    if max(nxt, j * c) < min(target, (j + 1) * c)]
            K = fu.fu_units_of(nxt, target, c)
            assert K == len(want) >= 1
            out, rep, ranges = c_pass(fu, v, rec, target, c)
            assert ranges == want
            assert [bool(fu.fu_unit_continues(nxt, c, k)) for k in range(K)] == [nxt % c != 0] + [False] * (K - 1)
            for k in range(K, K + 3):   # empty iff past the pixel's own units
                s0, s1 = ctypes.c_int(), ctypes.c_int()
                fu.fu_unit_range(nxt, target, c, k, ctypes.addressof(s0), ctypes.addressof(s1))
                assert s0.value >= s1.value, (nxt, target, c, k)
            total, opn, reported = oracle_record(v, target, c)
            assert np.array_equal(out, rec_words(target, total, opn)), (nxt, target, c)
            assert np.array_equal(rtref.bits(rep), rtref.bits(reported)), (nxt, target, c)
            assert (target % c != 0) or not out[4:7].any()
    assert fu.fu_units_of(5, 5, c) == 0 and fu.fu_units_of(6, 5, c) == 0
    # (a pass with nothing to render leaves the record as it was)
    rec = rec_words(5, *oracle_record(v, 5, c)[:2])
    out, rep, _ = c_pass(fu, v, rec, 5, c)
    assert np.array_equal(out, rec) and np.array_equal(rtref.bits(rep), rtref.bits(oracle_record(v, 5, c)[2]))


def test_the_restatement_sees_the_special_values():
    """Non-vacuity of the synthetic samples: the NaN reaches the sums from sample 13 on, the -0.f
    chunk folds to +0.f, and the chunk size changes the bits of a finite channel."""
    v = samples()
    assert np.isnan(oracle_record(v, 14, 3)[2][2]) and not np.isnan(oracle_record(v, 13, 3)[2]).any()
    assert rtref.bits(oracle_record(v, 1, 1)[2]).tolist() == [0, 0, 0]
    sums = {c: rtref.bits(oracle_record(v, 12, c)[2][:2]).tolist() for c in CHUNKS}
    assert len({tuple(s) for s in sums.values()}) > 1


@pytest.mark.parametrize("c", CHUNKS)
def test_two_passes_give_the_record_of_one(fu, c):
    v = samples()
    zero = rec_words(0, np.zeros(3, f32), np.zeros(3, f32))
    for n in range(1, N_MAX + 1):
        one, rep1, _ = c_pass(fu, v, zero, n, c)
        for m in range(1, n):
            a, _, _ = c_pass(fu, v, zero, m, c)
            b, rep2, _ = c_pass(fu, v, a, n, c)
            assert np.array_equal(b, one) and np.array_equal(rtref.bits(rep2), rtref.bits(rep1)), (m, n, c)


def test_open_words_rule(fu):
    z, nz = np.zeros(3, np.uint32), np.array([0, 0, 1], np.uint32)
    assert fu.fu_open_words_fit(6, 3, z.ctypes.data) and not fu.fu_open_words_fit(6, 3, nz.ctypes.data)
    assert fu.fu_open_words_fit(7, 3, z.ctypes.data) and fu.fu_open_words_fit(7, 3, nz.ctypes.data)
    assert not fu.fu_open_words_fit(0, 1, nz.ctypes.data)


# ---------------------------------------------------------------- the launch plan
def fu_plan(fu, n_pixels=HD, spp=256, variant_blocks=PLAIN_BLOCKS, **kw):
    i = FuIn(flags=0, kernel=0, count=0, fast_chunk=0, spp=spp, pass_spp=0, n_pixels=n_pixels, ray_depth=8,
             n_nodes=100000, spec_blocks=SPEC_BLOCKS, variant_blocks=variant_blocks, subset_items=0, fast_accum=0,
             fast_units=0)
    for k, val in kw.items():
        setattr(i, k, val)
    o = PlanOut()
    assert fu.fu_plan(ctypes.byref(i), ctypes.byref(o)) == o.err
    return o


def test_fast_pass_keeps_its_chunk_size(fu):
    assert fu.fu_max_chunks() == 128
    one_shot = fu_plan(fu, spp=4096, flags=F_FAST, fast_chunk=2)
    assert (one_shot.cs, one_shot.chunks, one_shot.v_chain) == (32, 128, 0)   # raised: at most 128 units per pixel
    # the last 256 samples of 4096 on an accumulator with c = 2: 128 units of 2
    o = fu_plan(fu, spp=4096, pass_spp=256, fast_chunk=2, fast_accum=1, fast_units=128)
    assert o.err == 0 and o.lane == 1
    assert (o.cs, o.chunks, o.n_items) == (2, 128, HD * 128)
    assert (o.v_count, o.v_fast, o.v_lsplit, o.v_spec, o.v_chain) == (0, 1, 0, 0, 1)
    assert o.sched == SCHED_FAST and (o.handoff, o.ordered, o.blocks2) == (0, 0, 0)
    assert o.stats_spp == 256 and o.blocks == PLAIN_BLOCKS
    # never ordered, whatever the flags; RT_FLAG_FAST set or not
    for flags in (F_FAST, F_HEAVY, F_NATURAL, F_NO_RUNAHEAD, F_FAST | F_HEAVY):
        p = fu_plan(fu, spp=4096, pass_spp=256, fast_chunk=2, fast_accum=1, fast_units=128, flags=flags)
        assert (p.v_fast, p.v_chain, p.v_spec, p.handoff, p.ordered, p.cs, p.sched) == (1, 1, 0, 0, 0, 2, SCHED_FAST)
    # a small shard is not the runahead kernel's either, and a chunk size above the pass stays
    p = fu_plan(fu, n_pixels=33 * 17, spp=3, pass_spp=1, fast_chunk=8, fast_accum=1, fast_units=1)
    assert (p.v_spec, p.handoff, p.cs, p.chunks, p.n_items, p.blocks) == (0, 0, 8, 1, 33 * 17, 3)
    # a subset pass: items x units
    p = fu_plan(fu, spp=9, pass_spp=1, fast_chunk=3, fast_accum=1, fast_units=3, subset_items=1000)
    assert (p.n_items, p.chunks, p.cs, p.ordered, p.v_spec) == (3000, 3, 3, 0, 0)


@pytest.mark.parametrize("kw", [dict(fast_units=0), dict(fast_units=129), dict(fast_chunk=0)])
def test_fast_pass_refuses_what_the_host_never_asks(fu, kw):
    args = dict(spp=300, pass_spp=300, fast_chunk=2, fast_accum=1, fast_units=128)
    args.update(kw)
    o = fu_plan(fu, **args)
    assert o.err == ERR_ARG and o.lane == 0


def test_defaults_give_the_plans_of_before(fu, tmp_path):
    """With the new fields at their defaults every plan equals plan_host.cpp's, which never sets
    them, field by field."""
    out = str(tmp_path / "libph.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-shared", "-fPIC", PLAN_SRC, "-o", out], check=True)
    ph = ctypes.CDLL(out)
    ph.ph_plan.argtypes = [ctypes.POINTER(PlanIn), ctypes.POINTER(PlanOut)]
    n = 0
    for flags in (0, F_FAST, F_LSPLIT, F_NATURAL, F_NO_RUNAHEAD, F_HEAVY, F_NATURAL | F_HEAVY, F_FAST | F_HEAVY):
        for kernel, count in ((0, 0), (0, 1), (4, 0), (3, 0)):
            for spp, pass_spp in ((0, 0), (1, 0), (4, 0), (256, 0), (4096, 0), (1 << 20, 0), (8, 3), (256, 256)):
                for n_pixels in (0, 561, 1024 * 512, HD):
                    for fast_chunk in (0, 2, 7, -1):
                        for vb in (PLAIN_BLOCKS, SPEC_BLOCKS):
                            kw = dict(flags=flags, kernel=kernel, count=count, fast_chunk=fast_chunk, spp=spp,
                                      pass_spp=pass_spp, n_pixels=n_pixels, ray_depth=8, n_nodes=5000,
                                      spec_blocks=SPEC_BLOCKS, variant_blocks=vb)
                            a, b = PlanOut(), PlanOut()
                            ph.ph_plan(ctypes.byref(PlanIn(**kw)), ctypes.byref(a))
                            fu.fu_plan(ctypes.byref(FuIn(subset_items=0, fast_accum=0, fast_units=0, **kw)), ctypes.byref(b))
                            for name, _ in PlanOut._fields_:
                                assert getattr(a, name) == getattr(b, name), (name, kw)
                            n += 1
    assert n == 8 * 4 * 8 * 4 * 4 * 2


# ---------------------------------------------------------------- the C ABI without a device
def test_symbols_exported_and_abi_unchanged(rt):
    lib = ctypes.CDLL(rt.LIB_PATH)
    assert [n for n in FAST_SYMBOLS if not hasattr(lib, n)] == []
    assert set(FAST_SYMBOLS) <= set(rt.ABI)
    assert rt.lib().rt_abi_version() == rt.ABI_VERSION == 6
    assert rt.lib().rt_accum_fast_chunk(None) == 0
    assert hasattr(rt.Accumulator, "fast_chunk")


@pytest.fixture(scope="module")
def scene(rt):
    return rt.Scene.load(rtref.scene_path("cornell"), 33, 17, 3)


def _create_fast(rt, scene, **kw):
    p = rt.RtParams(0, 0, 1, 8, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    h = ctypes.c_void_p()
    rc = rt.lib().rt_accum_create_fast(scene.handle, ctypes.byref(p), ctypes.byref(h))
    return rc, h.value, rt.lib().rt_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(count=1), "count"), (dict(kernel=4), "kernel"), (dict(flags=F_LSPLIT), "light-split"),
    (dict(flags=F_KERNEL_TIMES), "KERNEL_TIMES"), (dict(fast_chunk=-1), "fast_chunk"), (dict(flags=64), "unknown flag"),
    (dict(flags=F_FAST | F_LSPLIT), "light-split")])
def test_create_fast_refusals(rt, scene, kw, word):
    rc, h, msg = _create_fast(rt, scene, **kw)
    assert rc == ERR_ARG and not h
    assert word in msg and msg.startswith("rt_accum_create_fast")


@pytest.mark.parametrize("flags", [0, F_FAST, F_NATURAL | F_HEAVY, F_NO_RUNAHEAD | F_FAST])
def test_create_fast_accepts_the_order_flags(rt, scene, flags):
    """Past the parameter checks (RT_FLAG_FAST set or not, the order flags ignored, even both): the
    next thing it finds is that this scene was never uploaded, without a device call."""
    rc, h, msg = _create_fast(rt, scene, flags=flags, fast_chunk=3)
    assert rc == ERR_ARG and not h and "not uploaded" in msg and msg.startswith("rt_accum_create_fast")


def test_create_keeps_refusing_fast(rt, scene):
    p = rt.RtParams(0, 0, 1, 8, 0, 0, F_FAST, 0, 0)
    h = ctypes.c_void_p()
    assert rt.lib().rt_accum_create(scene.handle, ctypes.byref(p), ctypes.byref(h)) == ERR_ARG and not h.value
    msg = rt.lib().rt_last_error().decode()
    assert msg.startswith("rt_accum_create:") and "fast" in msg and "rt_accum_create_fast" in msg


def fast_header(view, n_pixels, samples, c, magic=FAST_MAGIC, per_pixel=0, **kw):
    """The documented layout: the parity header with the fast magic, the count form in the word
    after `samples done` and c in the first four of the eight trailing bytes."""
    h = _header(view, n_pixels, samples, magic=magic, **kw)
    return h[:60] + struct.pack("<i", per_pixel) + h[64:120] + struct.pack("<i", c) + h[124:]


def fast_records(n_pixels, nxt, c):
    """(pixel, next, total x y z, open x y z); open only where a chunk is open."""
    rec = np.zeros((n_pixels, 8), "<u4")
    rec[:, 0] = np.arange(n_pixels)
    rec[:, 1] = nxt
    rec[:, 2:5] = rtref.bits(np.full((n_pixels, 3), 1.5, f32))
    is_open = (rec[:, 1] % c) != 0
    rec[is_open, 5:8] = rtref.bits(np.full((int(is_open.sum()), 3), 0.25, f32))
    return rec


def test_fast_checkpoint_error_paths(rt, scene, tmp_path):
    view, n = scene.view(), 33 * 17
    good = fast_header(view, n, 4, 3) + fast_records(n, 4, 3).tobytes()
    assert len(good) == 128 + 32 * n and good[:8] == FAST_MAGIC and struct.unpack("<i", good[120:124]) == (3,)
    stale = fast_records(n, 6, 3)
    stale[5, 7] = 1   # an open word at a chunk boundary
    mixed = fast_records(n, np.where(np.arange(n) % 3 == 0, 7, 4), 3)
    fine = 0 if rt.device_count() > 0 else ERR_DEVICE   # (past the file checks: the first device call)
    cases = {
        "good": (good, fine),
        "good_on_a_boundary": (fast_header(view, n, 6, 3) + fast_records(n, 6, 3).tobytes(), fine),
        "per_pixel_counts": (fast_header(view, n, 7, 3, per_pixel=1) + mixed.tobytes(), fine),
        "bad_magic": (fast_header(view, n, 4, 3, magic=b"RTFACCUX") + fast_records(n, 4, 3).tobytes(), ERR_FORMAT),
        "bad_version": (fast_header(view, n, 4, 3, version=2) + fast_records(n, 4, 3).tobytes(), ERR_FORMAT),
        "one_record_short": (good[:-32], ERR_FORMAT),
        "one_record_long": (good + b"\0" * 32, ERR_FORMAT),
        "header_only_part": (good[:100], ERR_FORMAT),
        "chunk_zero": (fast_header(view, n, 4, 0) + fast_records(n, 4, 3).tobytes(), ERR_FORMAT),
        "chunk_negative": (fast_header(view, n, 4, -2) + fast_records(n, 4, 3).tobytes(), ERR_FORMAT),
        "stale_open_words": (fast_header(view, n, 6, 3) + stale.tobytes(), ERR_FORMAT),
        "uniform_with_unequal_records": (fast_header(view, n, 7, 3) + mixed.tobytes(), ERR_FORMAT),
        "record_above_samples": (fast_header(view, n, 6, 3, per_pixel=1) + mixed.tobytes(), ERR_FORMAT),
        "other_width": (fast_header(view, n, 4, 3, width=34) + fast_records(n, 4, 3).tobytes(), ERR_ARG),
        "other_rank": (fast_header(view, n, 4, 3, rank=1) + fast_records(n, 4, 3).tobytes(), ERR_ARG),
        "other_world": (fast_header(view, n, 4, 3, world=2) + fast_records(n, 4, 3).tobytes(), ERR_ARG),
    }
    for name, (data, want) in cases.items():
        path = tmp_path / (name + ".acc")
        path.write_bytes(data)
        rc, h, msg = _load(rt, scene, path)
        assert rc == want and bool(h) == (rc == 0), (name, rc, msg)
        if rc in (ERR_FORMAT, ERR_ARG):
            assert msg.startswith("rt_accum_load"), (name, msg)
        elif rc == 0:
            assert rt.lib().rt_accum_fast_chunk(h) == 3
            rt.lib().rt_accum_free(h)
    s48 = rt.Scene.load(rtref.scene_path("cornell"), 48, 48, 3)
    rc, h, msg = _load(rt, s48, tmp_path / "good.acc")
    assert rc == ERR_ARG and not h and "33 x 17" in msg


def test_a_parity_file_still_loads_as_parity(rt, scene, tmp_path):
    from test_accum import _records
    n = 33 * 17
    path = tmp_path / "parity.acc"
    path.write_bytes(_header(scene.view(), n, 2) + _records(n, 2))
    rc, h, msg = _load(rt, scene, path)
    assert rc == (0 if rt.device_count() > 0 else ERR_DEVICE), msg   # (past every file check)
    if rc == 0:
        assert rt.lib().rt_accum_fast_chunk(h) == 0
        rt.lib().rt_accum_free(h)
