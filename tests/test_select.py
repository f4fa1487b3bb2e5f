"""Per-pixel sample counts without a GPU: the selection rule (raytracing-hw_amd/csrc/rt_select.h
behind tests/native/select_host.cpp) against a numpy restatement on the oracle's sums, its
branches, the count-aware frame finish (rt_tonemap_u8_counts), the new entry points' argument
and checkpoint-file error paths (all decided before any device call) and the launch plan of a
subset pass.  The same harness, built a second time as a stand-alone program under the address
and undefined-behaviour sanitizers, runs once over the same cases.

Without a GPU no accumulator exists, so the argument checks that need one (a window outside the
frame, add_selected without a selection) are made here on the rule's own check function and on
NULL handles, and through the C ABI on a live accumulator in tests/test_gpu_select.py."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import rtref
from test_accum import _header, _load, _records
from plan_util import PlanIn, PlanOut
from test_launch_plan import PLAIN_BLOCKS, SPEC_BLOCKS, HD, SRC as PLAN_SRC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "select_host.cpp")
GXX = ["g++", "-O2", "-fno-tree-vectorize", "-fno-tree-slp-vectorize", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wextra"]
ERR_ARG, ERR_FORMAT, ERR_DEVICE, ERR_LIMIT = -1, -3, -4, -5
LANE, RUNAHEAD = 1, 2
F_NATURAL, F_NO_RUNAHEAD, F_HEAVY = 8, 16, 32
SELECT_SYMBOLS = ["rt_accum_mark", "rt_accum_select", "rt_accum_selection", "rt_accum_add_selected", "rt_accum_counts",
                  "rt_accum_counts_device", "rt_accum_sample_range", "rt_tonemap_u8_counts", "rt_tonemap_u8_counts_device"]
f32 = np.float32


class Rule(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("target", "x0", "y0", "x1", "y1")] + [("threshold", ctypes.c_float)]


SubsetIn, SubsetOut = PlanIn, PlanOut   # (one pair of structures for every plan shim: plan_util.py)


@pytest.fixture(scope="module")
def sh(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sh") / "libsh.so")
    subprocess.run(GXX + ["-shared", "-fPIC", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    V, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.sh_select.argtypes = [ctypes.POINTER(Rule), I, I, I, I, I, L, V, V, V, V, V, V, V, V, V, V]
    lib.sh_select.restype = L
    lib.sh_check_rule.argtypes = [ctypes.POINTER(Rule), I, I]
    lib.sh_count_normalizer.argtypes = [I]
    lib.sh_count_normalizer.restype = ctypes.c_float
    lib.sh_plan.argtypes = [ctypes.POINTER(SubsetIn), ctypes.POINTER(SubsetOut)]
    return lib


def select(sh, w, h, n_b, S_b, n_a, S_a, target, window=(0, 0, 0, 0), mask=None, threshold=0.0, shard=(0, 1, 8)):
    """sh_select over a shard: (list, estimates, samples, next_min, next_max)."""
    n = len(n_b)
    n_b, n_a = np.ascontiguousarray(n_b, np.int32), np.ascontiguousarray(n_a, np.int32)
    S_b, S_a = np.ascontiguousarray(S_b, f32).reshape(n, 3), np.ascontiguousarray(S_a, f32).reshape(n, 3)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(n)
    lst, e = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), f32)
    samples, lo, hi = ctypes.c_uint64(0), ctypes.c_int(0), ctypes.c_int(0)
    r = Rule(target, *window, threshold)
    k = sh.sh_select(ctypes.byref(r), w, h, *shard, n, n_b.ctypes.data, S_b.ctypes.data, n_a.ctypes.data, S_a.ctypes.data,
                     m.ctypes.data if m is not None else None, lst.ctypes.data, e.ctypes.data,
                     ctypes.addressof(samples), ctypes.addressof(lo), ctypes.addressof(hi))
    assert k >= 0
    return lst[:k], e[:n], samples.value, lo.value, hi.value


def np_estimate(S_a, n_a, S_b, n_b):
    """The rule's step 4 restated in numpy f32 from the formula in include/rt_hw.h."""
    S_a, S_b = np.asarray(S_a, f32), np.asarray(S_b, f32)
    ra, rn, rb = f32(1) / f32(n_a), f32(1) / f32(n_b - n_a), f32(1) / f32(n_b)
    with np.errstate(all="ignore"):
        ma, mn, mb = S_a * ra, (S_b - S_a) * rn, S_b * rb
        d = np.abs(mn - ma)
        e = ((d[:, 0] + d[:, 1]) + d[:, 2]) / np.sqrt(((mb[:, 0] + mb[:, 1]) + mb[:, 2]) + f32(1e-4))
    assert e.dtype == f32
    return e


# (scene, W, H, n_a, n_b, pixels threshold 0.5 selects)
RULE_CASES = [("cornell", 64, 64, 4, 8, 2224), ("cornell", 64, 64, 2, 4, 1965), ("sponza_mini", 64, 36, 4, 8, 1600)]
THRESHOLD = 0.5
_sums = {}


def oracle_sums(rt, oracle, name, w, h, n):
    if (name, w, h, n) not in _sums:
        _sums[name, w, h, n] = oracle.render(rtref.ref_arrays(rt, name, w, h, n), n)[0]
    return _sums[name, w, h, n]


def guarded_rule(S_a, n_a, S_b, n_b, threshold):
    """The numpy rule's selection, with the preconditions that keep an exact comparison honest:
    no estimate within 1e-4 relative of the threshold, none non-finite, a share in [0.2, 0.8]."""
    e = np_estimate(S_a, n_a, S_b, n_b)
    assert np.isfinite(e).all()
    assert (np.abs(e - f32(threshold)) > 1e-4 * threshold).all()
    want = np.nonzero(e > f32(threshold))[0]
    assert 0.2 <= len(want) / len(e) <= 0.8
    return want, e


@pytest.mark.parametrize("name,w,h,n_a,n_b,count", RULE_CASES)
def test_rule_matches_numpy_on_oracle_sums(rt, oracle, sh, name, w, h, n_a, n_b, count):
    S_a, S_b = oracle_sums(rt, oracle, name, w, h, n_a), oracle_sums(rt, oracle, name, w, h, n_b)
    want, e = guarded_rule(S_a, n_a, S_b, n_b, THRESHOLD)
    assert len(want) == count
    n = w * h
    got, e_host, samples, lo, hi = select(sh, w, h, np.full(n, n_b), S_b, np.full(n, n_a), S_a, n_b + 4, threshold=THRESHOLD)
    assert np.array_equal(got, want)
    assert np.array_equal(rtref.bits(e_host), rtref.bits(e))   # the estimate itself, bit for bit
    assert samples == 4 * count and (lo, hi) == (n_b, n_b + 4)


def test_rule_branches(sh):
    w, h, n = 8, 4, 32
    S_b = np.tile(np.array([4.0, 2.0, 1.0], f32), (n, 1))
    S_a = np.tile(np.array([1.0, 0.5, 0.25], f32), (n, 1))   # mean since the mark differs a lot: e > 0.5
    n_b, n_a = np.full(n, 4), np.full(n, 2)
    every = np.arange(n)
    sel = lambda **kw: select(sh, w, h, kw.pop("n_b", n_b), kw.pop("S_b", S_b), kw.pop("n_a", n_a), kw.pop("S_a", S_a), **kw)
    assert np.array_equal(sel(target=8, threshold=0.5)[0], every)
    # n_b >= target
    assert len(sel(target=4)[0]) == 0 and len(sel(target=3)[0]) == 0
    nb2 = n_b.copy()
    nb2[::2] = 6
    got, _, samples, lo, hi = sel(target=6, n_b=nb2)
    assert np.array_equal(got, every[1::2]) and samples == 2 * 16 and (lo, hi) == (6, 6)
    # the window is half-open in x and y
    got = sel(target=8, window=(2, 1, 5, 3))[0]
    assert np.array_equal(got, [y * w + x for y in (1, 2) for x in (2, 3, 4)])
    assert len(sel(target=8, window=(3, 1, 3, 2))[0]) == 0   # empty window: nothing
    # mask byte 0
    mask = np.ones(n, np.uint8)
    mask[[0, 7, 31]] = 0
    mask[5] = 200
    assert np.array_equal(sel(target=8, mask=mask)[0], np.setdiff1d(every, [0, 7, 31]))
    # threshold <= 0: no error test (also a negative one)
    flat = sel(target=8, threshold=0.5, S_a=S_b * f32(0.5))   # equal means before and since: e = 0
    assert len(flat[0]) == 0 and not flat[1].any()
    assert np.array_equal(sel(target=8, threshold=0.0, S_a=S_b * f32(0.5))[0], every)
    assert np.array_equal(sel(target=8, threshold=-1.0, S_a=S_b * f32(0.5))[0], every)
    # n_b == 0 and n_a == 0: no estimate yet, selected; n_b == n_a: nothing new, not selected
    z = np.zeros(n, np.int32)
    assert np.array_equal(sel(target=8, threshold=0.5, n_b=z, n_a=z, S_b=S_b * 0, S_a=S_b * 0)[0], every)
    assert np.array_equal(sel(target=8, threshold=0.5, n_a=z, S_a=S_b * f32(0.5))[0], every)
    na2 = n_a.copy()
    na2[10:20] = 4
    assert np.array_equal(sel(target=8, threshold=0.5, n_a=na2)[0], np.setdiff1d(every, np.arange(10, 20)))
    # non-finite sums: never selected under a threshold, selected without one
    bad = S_b.copy()
    bad[3, 1] = np.nan
    bad[9, 0] = np.inf
    got = sel(target=8, threshold=0.5, S_b=bad)
    assert np.array_equal(got[0], np.setdiff1d(every, [3, 9])) and np.isnan(got[1][[3, 9]]).all()
    assert np.array_equal(sel(target=8, S_b=bad)[0], every)
    # ascending, no duplicates, on a shard as well (rank 1 of 2, blocks of 2 rows, of an 8 x 8 frame)
    rng = np.random.default_rng(5)
    nb3 = rng.integers(0, 9, n)
    got, _, samples, lo, hi = select(sh, 8, 8, nb3, S_b, z, S_a, 5, window=(1, 0, 8, 7), shard=(1, 2, 2))
    rows = [y for y in range(8) if (y // 2) % 2 == 1]
    want = [p for p in range(n) if nb3[p] < 5 and p % 8 >= 1 and rows[p // 8] < 7]
    assert np.array_equal(got, want) and (np.diff(got) > 0).all()
    assert samples == sum(5 - nb3[p] for p in want)
    after = np.where(np.isin(every, want), 5, nb3)
    assert (lo, hi) == (after.min(), after.max())


def test_rule_argument_check(sh):
    chk = lambda *a: sh.sh_check_rule(ctypes.byref(Rule(*a)), 33, 17)
    assert chk(1, 0, 0, 0, 0, 0.0) == 0 and chk((1 << 20) - 1, 0, 0, 33, 17, 0.0) == 0 and chk(5, 3, 2, 3, 2, 0.0) == 0
    assert chk(0, 0, 0, 0, 0, 0.0) == 1 and chk(-4, 0, 0, 0, 0, 0.0) == 1
    assert chk(1 << 20, 0, 0, 0, 0, 0.0) == 2
    for window in [(5, 0, 4, 9), (0, 9, 8, 8), (-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 34, 17), (0, 0, 33, 18)]:
        assert chk(4, *window, 0.0) == 1, window


# ---------------------------------------------------------------- the count-aware finish (host)
def test_finish_with_counts(rt, sh):
    g = rtref.golden("finish_37x23x16.rtd")
    sums = np.ascontiguousarray(g["sums"], f32).reshape(23, 37, 3)
    want = open(os.path.join(rtref.GOLD, "finish_37x23x16.ppm"), "rb").read()[len(b"P6\n37 23\n255\n"):]
    assert not np.isfinite(sums).all()   # (the fixture carries the reference's NaN / inf cases)
    assert rt.tonemap_counts(sums, np.full((23, 37), 16, np.int32)).tobytes() == want
    counts = np.array([0, 1, 3, 16], np.int32)[np.random.default_rng(3).integers(0, 4, (23, 37))]
    got = rt.tonemap_counts(sums, counts)
    for c in (1, 3, 16):
        assert np.array_equal(got[counts == c], rt.tonemap(sums, c)[counts == c]), c
    assert (counts == 0).any() and not got[counts == 0].any()
    assert sh.sh_count_normalizer(0) == 0.0 and sh.sh_count_normalizer(3) == f32(1) / f32(3)
    with pytest.raises(ValueError):
        rt.tonemap_counts(sums, counts[:5])


# ---------------------------------------------------------------- ABI and argument errors
def test_symbols_exported_and_abi_unchanged(rt):
    lib = ctypes.CDLL(rt.LIB_PATH)
    assert [n for n in SELECT_SYMBOLS if not hasattr(lib, n)] == []
    assert set(SELECT_SYMBOLS) <= set(rt.ABI)
    assert rt.lib().rt_abi_version() == rt.ABI_VERSION == 6
    for name in ("mark", "select", "selection", "add_selected", "counts", "sample_range"):
        assert hasattr(rt.Accumulator, name), name
    assert hasattr(rt.Scene, "render_adaptive") and hasattr(rt, "tonemap_counts")


def test_argument_errors_before_any_device_call(rt):
    lib = rt.lib()
    n = ctypes.c_int64(7)

    def rc_of(target, window=(0, 0, 0, 0)):
        sel = rt.RtSelect(target, *window, None, 0.0)
        return lib.rt_accum_select(None, ctypes.byref(sel), None, ctypes.byref(n)), lib.rt_last_error().decode()

    assert rc_of(0)[0] == ERR_ARG and "target" in rc_of(0)[1]
    assert rc_of(-1)[0] == ERR_ARG
    rc, msg = rc_of(1 << 20)
    assert rc == ERR_LIMIT and "2^20" in msg
    for window in [(5, 0, 4, 9), (0, 9, 8, 8), (-1, 0, 8, 8)]:
        rc, msg = rc_of(4, window)
        assert rc == ERR_ARG and "window" in msg, window
    rc, msg = rc_of(4)
    assert rc == ERR_ARG and "NULL accumulator" in msg
    assert lib.rt_accum_select(None, None, None, None) == ERR_ARG
    assert n.value == 7
    st = rt.RtStats()
    assert lib.rt_accum_add_selected(None, None, ctypes.byref(st)) == ERR_ARG
    assert lib.rt_accum_mark(None, None) == ERR_ARG
    out = np.zeros(4, np.int32)
    ip = out.ctypes.data_as(rt._c_i)
    assert lib.rt_accum_selection(None, ip) == ERR_ARG and lib.rt_accum_counts(None, ip) == ERR_ARG
    assert lib.rt_accum_counts_device(None, None, None) == ERR_ARG
    assert lib.rt_accum_sample_range(None, ip, ip) == ERR_ARG
    sums, rgb = np.zeros(12, f32), np.zeros(12, np.uint8)
    fp, bp = sums.ctypes.data_as(rt._c_f), rgb.ctypes.data_as(rt._c_b)
    assert lib.rt_tonemap_u8_counts(None, ip, 2, 2, bp) == ERR_ARG
    assert lib.rt_tonemap_u8_counts(fp, None, 2, 2, bp) == ERR_ARG
    assert lib.rt_tonemap_u8_counts(fp, ip, 2, 2, None) == ERR_ARG
    assert lib.rt_tonemap_u8_counts(fp, ip, 0, 2, bp) == ERR_ARG
    assert lib.rt_tonemap_u8_counts_device(None, None, 2, 2, None, None) == ERR_ARG


# ---------------------------------------------------------------- checkpoint files, from the documented layout
def test_checkpoints_with_per_pixel_counts(rt, tmp_path):
    scene = rt.Scene.load(rtref.scene_path("cornell"), 33, 17, 3)
    view, n = scene.view(), 33 * 17
    per_pixel = lambda samples: _header(view, n, samples)[:60] + struct.pack("<i", 1) + _header(view, n, samples)[64:]
    assert struct.unpack("<2i", _header(view, n, 5)[56:64]) == (5, 0)   # (samples done, the count form)
    mixed = np.frombuffer(_records(n, 2), "<u4").reshape(n, 8).copy()
    mixed[::3, 1] = 5
    mixed[1::3, 1] = 0
    fine = 0 if rt.device_count() > 0 else ERR_DEVICE   # (past the file checks: the first device call)
    cases = {
        "per_pixel_ok": (per_pixel(5) + mixed.tobytes(), fine),
        "per_pixel_all_equal": (per_pixel(2) + _records(n, 2), fine),
        "per_pixel_above_samples": (per_pixel(4) + mixed.tobytes(), ERR_FORMAT),
        "uniform_with_unequal_records": (_header(view, n, 5) + mixed.tobytes(), ERR_FORMAT),
        "unknown_count_form": (_header(view, n, 5)[:60] + struct.pack("<i", 2) + _header(view, n, 5)[64:] + _records(n, 5),
                               ERR_FORMAT),
    }
    for name, (data, want) in cases.items():
        path = tmp_path / (name + ".acc")
        path.write_bytes(data)
        rc, h, msg = _load(rt, scene, path)
        assert rc == want, (name, rc, msg)
        if rc:
            assert not h and msg.startswith("rt_accum_load" if want == ERR_FORMAT else "")
        else:
            lo, hi = ctypes.c_int32(), ctypes.c_int32()
            assert rt.lib().rt_accum_sample_range(h, ctypes.byref(lo), ctypes.byref(hi)) == 0
            assert (lo.value, hi.value) == ((0, 5) if name == "per_pixel_ok" else (2, 2))
            rt.lib().rt_accum_free(h)


# ---------------------------------------------------------------- launch plan of a subset pass
@pytest.fixture(scope="module")
def plans(sh, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ph2") / "libph.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", PLAN_SRC, "-o", out], check=True)
    ph = ctypes.CDLL(out)
    ph.ph_plan.argtypes = [ctypes.POINTER(PlanIn), ctypes.POINTER(PlanOut)]

    def plan(subset_items=0, n_pixels=HD, spp=16, pass_spp=8, **kw):
        i = SubsetIn(flags=0, kernel=0, count=0, fast_chunk=0, spp=spp, pass_spp=pass_spp, n_pixels=n_pixels, ray_depth=8,
                     n_nodes=100000, spec_blocks=SPEC_BLOCKS, variant_blocks=0, subset_items=subset_items)
        for k, v in kw.items():
            setattr(i, k, v)
        o = SubsetOut()
        sh.sh_plan(ctypes.byref(i), ctypes.byref(o))
        i.variant_blocks = SPEC_BLOCKS if o.v_spec else PLAIN_BLOCKS
        sh.sh_plan(ctypes.byref(i), ctypes.byref(o))
        return i, o
    plan.ph = ph
    return plan


def test_subset_plan_goes_by_items(plans):
    # 100,000 items of the headline shard: at most two per resident runahead lane, so the runahead kernel
    _, o = plans(100000)
    assert o.err == 0 and (o.v_spec, o.v_chain, o.handoff, o.ordered) == (1, 1, 0, 0)
    assert o.sched == RUNAHEAD and o.n_items == 100000
    assert o.blocks == (100000 + 255) // 256 and o.slots == o.blocks * 256
    _, full = plans(0)
    assert (full.v_spec, full.handoff, full.n_items, full.blocks) == (0, 1, HD, PLAIN_BLOCKS)
    # the boundary is the full pass's, counted in items
    assert plans(SPEC_BLOCKS * 512)[1].v_spec == 1 and plans(SPEC_BLOCKS * 512 + 1)[1].v_spec == 0
    # a large subset: plain kernel with the hand-off, dealt in slot order (nothing is ordered)
    _, o = plans(691200, n_pixels=1280 * 720)
    assert o.sched == LANE | RUNAHEAD and (o.handoff, o.ordered, o.spread2) == (1, 0, 0)
    assert o.n_items == 691200 and o.blocks == PLAIN_BLOCKS and o.blocks2 == SPEC_BLOCKS
    # never ordered: not with RT_FLAG_HEAVY_ORDER, not at 128 samples or more
    assert plans(100000, flags=F_HEAVY)[1].ordered == 0
    assert plans(100000, spp=400, pass_spp=200)[1].ordered == 0 and plans(0, spp=400, pass_spp=200)[1].ordered == 1
    assert plans(HD, flags=F_HEAVY)[1].ordered == 0 and plans(0, flags=F_HEAVY)[1].ordered == 1
    # RT_FLAG_NO_RUNAHEAD still turns the runahead and the hand-off off
    _, o = plans(100000, flags=F_NO_RUNAHEAD)
    assert o.sched == LANE and (o.v_spec, o.handoff) == (0, 0)
    # the field means nothing outside an accumulator's pass
    _, o = plans(100000, pass_spp=0)
    assert o.n_items == HD and o.v_chain == 0


@pytest.mark.parametrize("kw", [
    dict(), dict(n_pixels=HD // 2), dict(n_pixels=HD // 4), dict(n_pixels=1024 * 512), dict(n_pixels=1024 * 513),
    dict(pass_spp=0, spp=256), dict(pass_spp=0, spp=64, flags=F_NATURAL), dict(pass_spp=0, spp=8, flags=F_HEAVY),
    dict(pass_spp=0, spp=256, flags=2, fast_chunk=3), dict(pass_spp=0, spp=256, flags=4), dict(pass_spp=0, spp=4, count=1),
    dict(pass_spp=0, spp=256, flags=F_NO_RUNAHEAD), dict(pass_spp=0, spp=256, kernel=4), dict(n_pixels=33 * 17, n_nodes=100),
    dict(spp=300, pass_spp=200), dict(n_pixels=0), dict(pass_spp=0, spp=1 << 20), dict(pass_spp=0, spp=256, ray_depth=16)])
def test_full_pass_plans_as_before(plans, kw):
    """With the new field 0 the plan is the one plan_host.cpp gives (which never sets the field)."""
    i, o = plans(0, **kw)
    pi = PlanIn(**{n: getattr(i, n) for n, _ in PlanIn._fields_})
    po = PlanOut()
    plans.ph.ph_plan(ctypes.byref(pi), ctypes.byref(po))
    for name, _ in SubsetOut._fields_:
        assert getattr(o, name) == getattr(po, name), name


# ---------------------------------------------------------------- the harness as a sanitized stand-alone program
def test_sanitized_program_over_the_same_cases(rt, oracle, sh, tmp_path):
    exe = str(tmp_path / "select_host")
    # (the sanitizer runtimes linked statically: the program needs nothing from its environment)
    subprocess.run(GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                          "-static-libubsan", "-DSELECT_HOST_MAIN", SRC, "-o", exe], check=True)
    cases = []   # (w, h, shard, target, window, mask, threshold, n_b, S_b, n_a, S_a)
    for name, w, h, n_a, n_b, _ in RULE_CASES:
        S_a, S_b = oracle_sums(rt, oracle, name, w, h, n_a), oracle_sums(rt, oracle, name, w, h, n_b)
        cases.append((w, h, (0, 1, 8), n_b + 4, (0, 0, 0, 0), None, THRESHOLD, np.full(w * h, n_b), S_b, np.full(w * h, n_a), S_a))
    rng = np.random.default_rng(11)
    n = 8 * 4 * 8
    S = rng.random((n, 3), f32)
    S[5, 0], S[17, 2] = np.nan, np.inf
    n_b = rng.integers(0, 9, n)
    n_a = np.minimum(rng.integers(0, 9, n), n_b)
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    cases.append((8, 32, (0, 1, 8), 6, (1, 2, 7, 30), mask, 0.25, n_b, S, n_a, S * f32(0.4)))
    cases.append((8, 64, (1, 2, 4), 9, (0, 0, 0, 0), None, 0.0, n_b, S, n_a, S * f32(0.4)))
    cases.append((8, 32, (0, 1, 8), 1, (3, 3, 3, 3), mask, -1.0, n_b, S, n_a, S))
    blob = struct.pack("<i", len(cases))
    for w, h, shard, target, window, m, thr, nb, Sb, na, Sa in cases:
        blob += struct.pack("<12if", w, h, *shard, target, *window, int(m is not None), len(nb), thr)
        blob += np.asarray(nb, "<i4").tobytes() + np.asarray(Sb, "<f4").tobytes()
        blob += np.asarray(na, "<i4").tobytes() + np.asarray(Sa, "<f4").tobytes()
        if m is not None:
            blob += m.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    out = (tmp_path / "out.bin").read_bytes()
    at = 0
    for w, h, shard, target, window, m, thr, nb, Sb, na, Sa in cases:
        k, samples, lo, hi = struct.unpack_from("<qQii", out, at)
        lst = np.frombuffer(out, "<i4", k, at + 24)
        at += 24 + 4 * k
        want = select(sh, w, h, nb, Sb, na, Sa, target, window, m, thr, shard)
        assert np.array_equal(lst, want[0]) and (samples, lo, hi) == want[2:]
    assert at == len(out)
    assert [struct.unpack_from("<q", out, 0)[0]] == [RULE_CASES[0][5]]
