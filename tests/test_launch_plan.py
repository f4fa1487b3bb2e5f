"""The render's launch plan without a GPU (raytracing-hw_amd/csrc/rt_launch_plan.h behind
tests/native/plan_host.cpp): which kernel instantiation, schedule, work units, pixel order and
grid launch() chooses, and what it refuses.  Resident block counts are inputs: 1280 for the
plain kernel and 1024 for the runahead kernel (256 CUs at 5 and 4 blocks)."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import pytest

from plan_util import PlanIn as In, PlanOut as Out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "plan_host.cpp")
PLAIN_BLOCKS, SPEC_BLOCKS = 1280, 1024
LANE, RUNAHEAD, FAST, LIGHT_SPLIT, WAVEFRONT = 1, 2, 4, 8, 16          # RT_SCHED_*
F_FAST, F_LSPLIT, F_NATURAL, F_NO_RUNAHEAD, F_HEAVY = 2, 4, 8, 16, 32   # RT_FLAG_*
ERR_ARG, ERR_LIMIT = -1, -5
HD = 1920 * 1080


@pytest.fixture(scope="module")
def ph(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ph") / "libph.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-shared", "-fPIC", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.ph_plan.argtypes = [ctypes.POINTER(In), ctypes.POINTER(Out)]
    lib.ph_plan.restype = ctypes.c_int

    def plan(n_pixels=HD, spp=256, variant_blocks=None, **kw):
        i = In(flags=0, kernel=0, count=0, fast_chunk=0, spp=spp, pass_spp=0, n_pixels=n_pixels, ray_depth=8,
               n_nodes=100000, spec_blocks=SPEC_BLOCKS, variant_blocks=0)
        for k, v in kw.items():
            setattr(i, k, v)
        o = Out()
        if variant_blocks is None:   # the chosen kernel's: a first call tells which one that is
            lib.ph_plan(ctypes.byref(i), ctypes.byref(o))
            variant_blocks = SPEC_BLOCKS if o.v_spec else PLAIN_BLOCKS
        i.variant_blocks = variant_blocks
        rc = lib.ph_plan(ctypes.byref(i), ctypes.byref(o))
        assert rc == o.err
        return o
    plan.lib = lib
    return plan


def test_headline_frame_is_plain_kernel_with_handoff(ph):
    o = ph(HD)
    assert HD == 2073600
    assert o.err == 0 and o.lane == 1
    assert (o.v_count, o.v_fast, o.v_lsplit, o.v_spec, o.v_chain) == (0, 0, 0, 0, 0)
    assert o.sched == LANE | RUNAHEAD and o.handoff == 1
    assert (o.blocks, o.slots) == (1280, 327680)
    assert o.ordered == 1 and (o.groups, o.per) == (5120, 64)
    assert (o.cs, o.chunks, o.n_items) == (0, 1, HD)
    assert o.stats_spp == 256


@pytest.mark.parametrize("n_pixels,spec", [
    (HD // 2, False),        # world 2: 1,036,800
    (HD // 4, True),         # world 4: 518,400
    (1024 * 512, True),      # 2 pixels per resident lane of the runahead kernel: the boundary
    (1024 * 513, False)])
def test_runahead_up_to_two_pixels_per_lane_then_handoff(ph, n_pixels, spec):
    o = ph(n_pixels)
    assert o.err == 0 and o.v_spec == int(spec) and o.handoff == int(not spec)
    assert o.sched == (RUNAHEAD if spec else LANE | RUNAHEAD)
    if spec:
        assert o.blocks == 1024 and o.blocks2 == 0
    if n_pixels == HD // 4:
        assert n_pixels == 518400


def test_mode_word_round_trips(ph):
    vals = (0, 1, 56, 100, 255)
    below, pct = ctypes.c_int(-1), ctypes.c_int(-1)
    words = set()
    for b in vals:
        for p in vals:
            mode = ph.lib.ph_mode_pack(b, p)
            ph.lib.ph_mode_unpack(mode, ctypes.byref(below), ctypes.byref(pct))
            assert (below.value, pct.value) == (b, p)
            words.add(mode)
    assert len(words) == len(vals) ** 2 and ph.lib.ph_mode_pack(0, 0) == 0   # (0: the default schedules)


# (slots, pct, waves) -> (dealt, per): the resume launch's deal (rt_launch_plan.h resume_deal),
# worked out by hand, and again below in exact fractions
DEALS = [
    ((327680, 100, 4096), (327680, 64)),   # the headline: 80 a wave, capped at one per lane
    ((25600, 100, 4096), (25600, 7)),      # 6.25 a wave rounds up
    ((768, 100, 4096), (768, 1)),          # fewer slots than waves: 0.19 a wave rounds up
    ((0, 100, 4096), (0, 1)),              # nothing parked: per forced up to 1
    ((100, 0, 4), (0, 1)),                 # nothing dealt: per forced up to 1
    ((192, 100, 3), (192, 64)),            # exactly 64 a wave
    ((193, 100, 3), (193, 64)),            # 64.3 a wave: capped at 64
    ((101, 50, 4), (51, 13)),              # 50.5 rounds up to 51 dealt; 12.75 a wave rounds up
    ((7, 60, 2), (5, 3)),                  # 4.2 rounds up to 5 dealt; 2.5 a wave rounds up
    ((10, 50, 5), (5, 1)),                 # exact: no rounding
    ((1000, 1, 4), (10, 3)),
]


def test_resume_deal_table(ph):
    ph.lib.ph_deal.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong,
                               ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    ph.lib.ph_deal.restype = None
    dealt, per = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
    for (slots, pct, waves), want in DEALS:
        ph.lib.ph_deal(slots, pct, waves, ctypes.byref(dealt), ctypes.byref(per))
        assert (dealt.value, per.value) == want, (slots, pct, waves)
        d = math.ceil(Fraction(slots * pct, 100))
        assert want == (d, min(64, max(1, math.ceil(Fraction(d, waves))))), (slots, pct, waves)
    assert {1, 64} <= {w[1] for _, w in DEALS}   # both clamps are in the table


def test_handoff_relaunch_deal_is_the_kernels_resume_formula(ph):
    # plan_grid deals the main launch's slots over the runahead kernel's resident waves with
    # RT_HANDOFF_PCT 100 (test_resume_deal_table pins the rule itself)
    for blocks in (PLAIN_BLOCKS, 100, 3):
        o = ph(600000, variant_blocks=blocks)
        slots = blocks * 256
        waves = 4 * SPEC_BLOCKS
        assert o.handoff == 1 and (o.blocks, o.slots) == (blocks, slots)
        assert (o.blocks2, o.waves2, o.dealt) == (SPEC_BLOCKS, waves, slots)
        assert o.per2 == min(64, max(1, -(-slots // waves)))
        assert o.spread2 == 1   # ordered, and the order buffer's arrays hold the slots
    assert [ph(600000, variant_blocks=b).per2 for b in (PLAIN_BLOCKS, 100, 3)] == [64, 7, 1]
    assert ph(600000, flags=F_NATURAL).spread2 == 0   # no estimates: slot order


def test_other_schedules(ph):
    for kw in (dict(count=1), dict(flags=F_NO_RUNAHEAD)):
        for n in (HD, HD // 8):
            o = ph(n, **kw)
            assert o.err == 0 and o.sched == LANE and o.handoff == 0 and o.v_spec == 0
            assert o.v_count == kw.get("count", 0)
    for count in (0, 1):
        o = ph(HD, flags=F_LSPLIT, count=count)
        assert o.sched == LIGHT_SPLIT and (o.v_lsplit, o.v_count, o.v_spec, o.handoff) == (1, count, 0, 0)
    o = ph(HD, kernel=4)
    assert o.err == 0 and o.sched == WAVEFRONT and o.lane == 0
    o = ph(0)   # a rank without rows launches nothing
    assert o.err == 0 and o.sched == 0 and o.lane == 0
    o = ph(HD // 8, count=1)
    assert o.blocks == min(PLAIN_BLOCKS, -(-(HD // 8) // 256))


@pytest.mark.parametrize("spp,fast_chunk,cs,chunks", [(256, 0, 2, 128), (1024, 0, 8, 128), (3, 0, 2, 2), (1, 0, 1, 1),
                                                      (256, 16, 16, 16)])
def test_fast_mode_work_units(ph, spp, fast_chunk, cs, chunks):
    for flags in (F_FAST, F_FAST | F_HEAVY, F_FAST | F_LSPLIT):
        o = ph(HD // 8, spp=spp, flags=flags, fast_chunk=fast_chunk)
        assert o.err == 0 and o.sched == FAST and o.ordered == 0
        assert (o.v_fast, o.v_lsplit, o.v_spec, o.handoff) == (1, 0, 0, 0)
        assert (o.cs, o.chunks, o.n_items) == (cs, chunks, (HD // 8) * chunks)
        assert o.blocks == min(PLAIN_BLOCKS, -(-o.n_items // 256))


def test_ordering_rule(ph):
    assert ph(spp=127).ordered == 0 and ph(spp=128).ordered == 1
    assert ph(spp=4, flags=F_HEAVY).ordered == 1
    assert ph(spp=256, flags=F_NATURAL).ordered == 0
    # a pass is ordered by its own samples, and counted by them
    o = ph(spp=256, pass_spp=64)
    assert o.ordered == 0 and o.stats_spp == 64
    o = ph(spp=256, pass_spp=128)
    assert o.ordered == 1 and o.stats_spp == 128


def test_round_min_by_scene_size(ph):
    assert ph(n_nodes=4095).round_min == 4
    assert ph(n_nodes=4096).round_min == 65


def test_pass_variants_keep_the_one_shot_schedule(ph):
    for n in (HD, HD // 8):
        one, p = ph(n), ph(n, pass_spp=8)
        assert p.v_chain == 1 and one.v_chain == 0
        assert (p.v_spec, p.sched, p.handoff, p.blocks, p.slots) == (one.v_spec, one.sched, one.handoff, one.blocks, one.slots)
        assert (p.v_count, p.v_fast, p.v_lsplit) == (0, 0, 0)


@pytest.mark.parametrize("kw,code,text", [
    (dict(kernel=3), ERR_ARG, "rt_render: unknown kernel 3 (0 lane-resident, 4 wavefront)"),
    (dict(spp=0), ERR_ARG, "rt_render: samples per pixel must be >= 1"),
    (dict(spp=1 << 20), ERR_LIMIT, "rt_render: spp must be < 2^20"),
    (dict(ray_depth=0), ERR_LIMIT, "ray_depth must be in [1, 15]"),
    (dict(ray_depth=16), ERR_LIMIT, "ray_depth must be in [1, 15]"),
    (dict(kernel=4, flags=F_FAST), ERR_ARG, "rt_render: fast mode and the light-split kernel run on kernel 0 only"),
    (dict(kernel=4, flags=F_LSPLIT), ERR_ARG, "rt_render: fast mode and the light-split kernel run on kernel 0 only"),
    (dict(fast_chunk=-1), ERR_ARG, "rt_render: fast_chunk must be >= 0"),
    (dict(flags=F_NATURAL | F_HEAVY), ERR_ARG, "rt_render: RT_FLAG_NATURAL_ORDER and RT_FLAG_HEAVY_ORDER exclude each other"),
    (dict(n_pixels=40000 * 256, ray_depth=15, variant_blocks=40000), ERR_LIMIT, "rt_render: vertex records beyond 4 GiB")])
def test_refusals(ph, kw, code, text):
    o = ph(**kw)
    assert o.err == code and o.msg.decode() == text


def test_limits_just_inside(ph):
    assert ph(spp=(1 << 20) - 1).err == 0 and ph(ray_depth=1).err == 0 and ph(ray_depth=15).err == 0
    # 2^32 / (256 * 15 * 32) = 34952.5 blocks
    assert ph(n_pixels=40000 * 256, ray_depth=15, variant_blocks=34952).err == 0
    assert ph(n_pixels=40000 * 256, ray_depth=15, variant_blocks=34953).err == ERR_LIMIT


# ---------------------------------------------------------------- the variant table
# rt_launch_plan.h kVariants, in its order: (count, fast, lsplit, spec, chain, mom)
VARIANTS = [(1, 1, 0, 0, 0, 0), (0, 0, 0, 1, 1, 0), (0, 0, 0, 1, 0, 0), (0, 1, 0, 0, 0, 0), (1, 0, 1, 0, 0, 0), (0, 0, 1, 0, 0, 0),
            (0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 1, 0), (0, 1, 0, 0, 1, 0), (0, 1, 0, 0, 1, 1)]


def sweep():
    """What rt_render* and rt_accum_* admit, on both sides of the runahead boundary."""
    for n_pixels in (1024 * 512, 1024 * 513):
        for flags in (0, F_FAST, F_LSPLIT, F_NO_RUNAHEAD):
            for count in (0, 1):
                yield dict(n_pixels=n_pixels, spp=8, flags=flags, count=count)
        for flags in (0, F_NO_RUNAHEAD):
            for subset_items in (0, 100):
                yield dict(n_pixels=n_pixels, spp=8, pass_spp=4, flags=flags, subset_items=subset_items)
                for moments in (0, 1):
                    yield dict(n_pixels=n_pixels, spp=8, pass_spp=4, flags=flags, subset_items=subset_items, fast_accum=1,
                               fast_chunk=2, fast_units=2, moments=moments)


def test_every_admitted_plan_has_a_kernel_and_every_kernel_a_plan(ph):
    reached, n = set(), 0
    for kw in sweep():
        o = ph(**kw)
        assert o.err == 0 and o.lane == 1 and o.variant_index >= 0, kw
        assert VARIANTS[o.variant_index] == (o.v_count, o.v_fast, o.v_lsplit, o.v_spec, o.v_chain, o.v_mom), kw
        reached.add(o.variant_index)
        n += 1
    assert n == 40 and reached == set(range(11))


def test_mom_only_on_a_fast_accumulators_pass_that_asks(ph):
    for fast_accum in (0, 1):
        for pass_spp in (0, 4):
            for moments in (0, 1):
                for flags in (0, F_FAST):
                    o = ph(spp=8, pass_spp=pass_spp, flags=flags, fast_accum=fast_accum, fast_chunk=2, fast_units=2, moments=moments)
                    assert o.err == 0 and o.v_mom == int(fast_accum and pass_spp > 0 and moments)


def test_mode_words_of_the_launch_and_the_relaunch(ph):
    pack = ph.lib.ph_mode_pack
    o = ph(HD)   # the headline frame: the plain kernel parks below 56, the relaunch deals 100%
    assert o.handoff == 1 and o.mode == pack(56, 0) and o.mode2 == pack(0, 100)
    o = ph(HD // 8)   # an 8-way shard: the runahead kernel, no hand-off
    assert (o.v_spec, o.handoff, o.mode, o.mode2) == (1, 0, 0, 0)
    o = ph(spp=9, pass_spp=1, fast_chunk=3, fast_accum=1, fast_units=3)   # a fast pass: the units per item
    assert (o.v_fast, o.v_chain, o.mode, o.mode2) == (1, 1, 3, 0)

