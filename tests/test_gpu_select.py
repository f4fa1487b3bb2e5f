"""Per-pixel sample counts on the GPU (include/rt_hw.h rt_accum_select / rt_accum_add_selected):
after any sequence of full and subset passes, a pixel that has n samples holds exactly the
reference's sum of that pixel at spp = n, on every schedule; pixels a pass does not list keep
their bits and records; and every selection list is checked (ascending, no duplicates, every
entry below the target) before the pass that renders it is launched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtref
from test_gpu_accum import SCHEDULES, SOLUTION, _ref_scene, gpu, handoff_ref   # noqa: F401  (fixtures)
from test_select import THRESHOLD, guarded_rule

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_LIMIT = -1, -5
# resident blocks of the runahead kernel on the MI355X (256 CUs at 4 blocks, as tests/test_launch_plan.py):
# a pass of more than two items per resident lane runs on the plain kernel and hands its tail off
SPEC_LANES = 1024 * 256

_oracle = {}


def oracle_sums(oracle, arrays, key, n):
    """The CPU oracle's sums of the whole frame at n samples, (H, W, 3), made once per frame."""
    if (key, n) not in _oracle:
        h, w = int(arrays["height"]), int(arrays["width"])
        _oracle[key, n] = oracle.render(arrays, n)[0].reshape(h, w, 3)
    return _oracle[key, n]


def select(acc, target, **kw):
    """select(), with the list checked before anything renders it."""
    before = acc.state()[:, 0].astype(np.int64)
    n = acc.select(target, **kw)
    lst = acc.selection()
    assert len(lst) == n
    assert (np.diff(lst) > 0).all(), "the list must be ascending without duplicates"
    assert n == 0 or (lst[0] >= 0 and lst[-1] < len(before))
    assert (before[lst] < target).all(), "every listed pixel must be below the target"
    return lst, before


def add_selected(acc, lst, before, target):
    """add_selected(), with its stats checked against the list and the records around it."""
    st_before, sums_before = acc.state(), acc.sums().reshape(-1, 3)
    stats = acc.add_selected()
    assert stats["pixels"] == len(lst) and stats["samples"] == int((target - before[lst]).sum())
    assert stats["order_ms"] == 0
    keep = np.ones(len(before), bool)
    keep[lst] = False
    st_after = acc.state()
    assert np.array_equal(st_after[keep], st_before[keep]), "a pixel outside the list changed its record"
    assert np.array_equal(rtref.bits(acc.sums().reshape(-1, 3)[keep]), rtref.bits(sums_before[keep]))
    assert (st_after[lst, 0] == target).all()
    return stats


def check_invariant(acc, want_counts, sums_at, rows=None):
    """counts() is the expected map and, per distinct count n, the pixels at n hold sums_at(n)."""
    counts = acc.counts()
    assert np.array_equal(counts, want_counts)
    assert acc.sample_range == (int(counts.min()), int(counts.max())) and acc.samples == int(counts.max())
    got = acc.sums()
    for n in np.unique(counts):
        at = counts == n
        want = sums_at(int(n)) if n else np.zeros_like(got)
        want = want if rows is None else want[rows]
        bad = (rtref.bits(got[at]) != rtref.bits(want[at])).any(1)
        assert bad.sum() == 0, f"{bad.sum()} of the {at.sum()} pixels at {n} samples differ from the reference"


def run_steps(gpu, oracle, scene, arrays, key, steps, sched=None, rank=0, world=1, row_block=8):
    """add(1), then the subset steps [(target, select arguments)]; the invariant after each."""
    h, w = int(arrays["height"]), int(arrays["width"])
    acc = scene.accumulator(rank=rank, world=world, row_block=row_block, **(sched or {}))
    rows = acc.rows
    ys, xs = np.meshgrid(rows, np.arange(w), indexing="ij")
    sums_at = lambda n: oracle_sums(oracle, arrays, key, n)
    acc.add(1)
    counts = np.ones((len(rows), w), np.int32)
    check_invariant(acc, counts, sums_at, rows)
    all_stats = []
    for target, kw in steps:
        lst, before = select(acc, target, **kw)
        chosen = counts < target
        if "window" in kw:
            x0, y0, x1, y1 = kw["window"]
            chosen &= (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
        if "mask" in kw:
            chosen &= kw["mask"] != 0
        assert np.array_equal(lst, np.nonzero(chosen.reshape(-1))[0])
        starts = set(np.unique(counts[chosen]))
        all_stats.append((add_selected(acc, lst, before, target), starts))
        counts = np.where(chosen, target, counts).astype(np.int32)
        check_invariant(acc, counts, sums_at, rows)
    return acc, counts, all_stats


def cornell_steps(w=64, rows=64):
    even = np.zeros((rows, w), np.uint8)
    even[:, ::2] = 1
    return [(3, dict(mask=even)), (5, dict(window=(10, 20, 40, 50))), (8, dict())]


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_invariant_on_every_schedule(gpu, oracle, sched):
    scene, arrays, want8 = _ref_scene(gpu, "cornell", 64, 64, 8)
    acc, counts, stats = run_steps(gpu, oracle, scene, arrays, "cornell64", cornell_steps(), SCHEDULES[sched])
    assert stats[-1][1] == {1, 3, 5}   # the last pass held pixels starting at three different samples
    print(f"{sched}: schedules {[st['schedule'] for st, _ in stats]}")
    want_sched = gpu.SCHED_LANE if sched == "no_runahead" else gpu.SCHED_RUNAHEAD
    assert [st["schedule"] for st, _ in stats] == [want_sched] * 3
    assert (counts == 8).all() and acc.sample_range == (8, 8)
    assert np.array_equal(rtref.bits(acc.sums()), rtref.bits(want8))
    acc.free()


@pytest.mark.parametrize("world", [2, 3])
def test_invariant_on_shards(gpu, oracle, world):
    """cornell 33 x 17 (odd sizes) as shards of blocks of 4 rows, with a window that crosses shard
    rows; reassembled against the oracle per count and, at the end, the reference's golden."""
    scene, arrays, want3 = _ref_scene(gpu, "cornell", 33, 17, 3)
    frame = np.zeros((17, 33, 3), np.float32)
    for rank in range(world):
        rows = gpu.shard_rows(17, rank, world, 4)
        even = np.zeros((len(rows), 33), np.uint8)
        even[:, ::2] = 1
        steps = [(2, dict(mask=even)), (3, dict(window=(5, 2, 29, 11))), (3, dict())]
        acc, counts, _ = run_steps(gpu, oracle, scene, arrays, "cornell33", steps, rank=rank, world=world, row_block=4)
        assert (counts == 3).all()
        frame[rows] = acc.sums()
        acc.free()
    assert np.array_equal(rtref.bits(frame), rtref.bits(want3))


def test_adaptive_rule_on_the_device(gpu, oracle):
    scene, arrays, _ = _ref_scene(gpu, "cornell", 64, 64, 8)
    sums_at = lambda n: oracle_sums(oracle, arrays, "cornell64", n)
    acc = scene.accumulator()
    acc.add(4)
    acc.mark()
    acc.add(4)
    want, _ = guarded_rule(sums_at(4).reshape(-1, 3), 4, sums_at(8).reshape(-1, 3), 8, THRESHOLD)
    assert len(want) == 2224
    lst, before = select(acc, 12, threshold=THRESHOLD)
    assert np.array_equal(lst, want)
    acc.mark()   # (changes no record: the list stays pending)
    add_selected(acc, lst, before, 12)
    counts = np.full(64 * 64, 8, np.int32)
    counts[lst] = 12
    check_invariant(acc, counts.reshape(64, 64), sums_at)
    again, _ = select(acc, 16, threshold=THRESHOLD)
    assert np.isin(again, lst).all(), "a pixel that was judged converged came back without new samples"
    print(f"second round: {len(again)} of the {len(lst)} refined pixels selected again")
    acc.free()


def test_plain_kernel_and_handoff_with_unequal_starts(gpu, handoff_ref):
    scene, want, ref = handoff_ref
    w, h = 1280, 720
    acc = scene.accumulator()
    acc.add(1)
    even = np.zeros((h, w), np.uint8)
    even[:, ::2] = 1
    lst, before = select(acc, 2, mask=even)
    st = add_selected(acc, lst, before, 2)
    assert len(lst) == w * h // 2 and st["schedule"] == gpu.SCHED_RUNAHEAD
    rows3 = np.zeros((h, w), np.uint8)
    rows3[np.arange(h) % 4 != 0] = 1
    lst, before = select(acc, 6, mask=rows3)
    assert len(lst) == 691200 and set(np.unique(before[lst])) == {1, 2}
    st = add_selected(acc, lst, before, 6)
    assert len(lst) > 2 * SPEC_LANES and st["schedule"] == gpu.SCHED_LANE | gpu.SCHED_RUNAHEAD
    assert acc.sample_range == (1, 6)
    lst, before = select(acc, 6)
    assert len(lst) == w * h - 691200 and len(lst) <= 2 * SPEC_LANES
    st = add_selected(acc, lst, before, 6)
    assert st["schedule"] == gpu.SCHED_RUNAHEAD and acc.sample_range == (6, 6)
    got = acc.sums()
    bad = (rtref.bits(got) != rtref.bits(want)).any(2)
    assert bad.sum() == 0, f"{bad.sum()} pixels differ from the one-shot render"
    for p, r in ref.items():
        assert np.array_equal(rtref.bits(got.reshape(-1, 3)[p]), rtref.bits(r)), f"pixel {p}"
    acc.free()


def test_frame_finish_by_count(gpu, oracle):
    scene, arrays, _ = _ref_scene(gpu, "cornell", 64, 64, 8)
    acc, counts, _ = run_steps(gpu, oracle, scene, arrays, "cornell64", cornell_steps()[:2])
    assert set(np.unique(counts)) == {1, 3, 5}
    frame = acc.frame()
    assert np.array_equal(frame, gpu.tonemap_counts(acc.sums(), acc.counts()))
    for n in (1, 3, 5):
        assert np.array_equal(frame[counts == n], gpu.tonemap(oracle_sums(oracle, arrays, "cornell64", n), n)[counts == n])
    lst, before = select(acc, 5)
    add_selected(acc, lst, before, 5)
    assert acc.sample_range == (5, 5)   # uniform again: the frame is the one it always was
    assert np.array_equal(acc.frame(), gpu.tonemap(oracle_sums(oracle, arrays, "cornell64", 5), 5))
    acc.free()


def test_leveling_and_limits(gpu, oracle):
    scene, arrays, want8 = _ref_scene(gpu, "cornell", 64, 64, 8)
    lib = gpu.lib()
    acc = scene.accumulator()
    st = gpu.RtStats()
    assert lib.rt_accum_add_selected(acc._h, None, ctypes.byref(st)) == ERR_ARG   # nothing selected yet
    assert b"no pending selection" in lib.rt_last_error()
    # arguments are checked before any launch, on the accumulator's frame
    for window in [(0, 0, 65, 64), (0, 0, 64, 65), (10, 0, 9, 5), (-1, 0, 4, 4)]:
        sel = gpu.RtSelect(4, *window, None, 0.0)
        assert lib.rt_accum_select(acc._h, ctypes.byref(sel), None, None) == ERR_ARG, window
    for target, want in ((0, ERR_ARG), (1 << 20, ERR_LIMIT)):
        sel = gpu.RtSelect(target, 0, 0, 0, 0, None, 0.0)
        assert lib.rt_accum_select(acc._h, ctypes.byref(sel), None, None) == want
    assert lib.rt_accum_add_selected(acc._h, None, None) == ERR_ARG   # (a refused select leaves no list)
    acc.add(2)
    lst, before = select(acc, 5, window=(0, 0, 64, 32))
    add_selected(acc, lst, before, 5)
    assert acc.samples == 5 and acc.sample_range == (2, 5)
    with pytest.raises(gpu.RtError, match="level"):
        acc.add(1)
    assert acc.sample_range == (2, 5)
    # an empty selection launches nothing
    assert acc.select(2) == 0 and len(acc.selection()) == 0
    stats = acc.add_selected()
    assert stats["pixels"] == 0 and stats["samples"] == 0 and stats["render_ms"] == 0 and stats["schedule"] == 0
    with pytest.raises(gpu.RtError, match="no pending selection"):
        acc.add_selected()
    # level, then a full pass works again and ends on the reference's golden
    lst, before = select(acc, acc.samples)
    add_selected(acc, lst, before, 5)
    assert acc.sample_range == (5, 5)
    assert acc.select(8) == 64 * 64
    acc.add(3)   # (a full pass drops the pending selection)
    with pytest.raises(gpu.RtError, match="no pending selection"):
        acc.add_selected()
    assert np.array_equal(rtref.bits(acc.sums()), rtref.bits(want8))
    acc.free()


def test_save_and_load_with_unequal_counts(gpu, oracle, tmp_path):
    scene, arrays, want8 = _ref_scene(gpu, "cornell", 64, 64, 8)
    acc, counts, _ = run_steps(gpu, oracle, scene, arrays, "cornell64", cornell_steps()[:2])
    path = str(tmp_path / "mixed.acc")
    sums, state = acc.sums(), acc.state()
    acc.save(path)
    acc.free()
    hdr = np.fromfile(path, np.int32, 16)
    assert (hdr[14], hdr[15]) == (5, 1)   # samples done = the largest count; the count form
    acc = gpu.Accumulator.load(scene, path)
    assert acc.sample_range == (1, 5) and acc.samples == 5
    assert np.array_equal(acc.counts(), counts) and np.array_equal(acc.state(), state)
    assert np.array_equal(rtref.bits(acc.sums()), rtref.bits(sums))
    lst, before = select(acc, 8, threshold=THRESHOLD)   # no mark after a load: every pixel below the target
    assert len(lst) == 64 * 64
    add_selected(acc, lst, before, 8)
    assert np.array_equal(rtref.bits(acc.sums()), rtref.bits(want8))
    acc.free()


def test_render_adaptive(gpu, oracle):
    scene, arrays, _ = _ref_scene(gpu, "cornell", 64, 64, 8)
    sums, counts, frame = scene.render_adaptive(8, 16, 4, THRESHOLD)
    assert counts.min() == 8 and counts.max() <= 16 and set(np.unique(counts)) <= {8, 12, 16}
    assert (counts == 12).sum() + (counts == 16).sum() == 2224
    for n in np.unique(counts):
        at = counts == n
        want = oracle_sums(oracle, arrays, "cornell64", int(n))
        assert np.array_equal(rtref.bits(sums[at]), rtref.bits(want[at]))
    assert np.array_equal(frame, gpu.tonemap_counts(sums, counts))


# ---------------------------------------------------------------- CLI
def _cli(out, samples, **env_add):
    env = dict(os.environ)
    for k in ("RT_PASS_SPP", "RT_CHECKPOINT", "RT_ADAPT", "RT_COUNTS_OUT"):
        env.pop(k, None)
    env["RT_GPUS"] = "1"
    env.update(env_add)
    r = subprocess.run([SOLUTION, rtref.scene_path("cornell"), "33", "17", str(samples), out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _pgm(path, w, h):
    data = open(path, "rb").read()
    header = b"P5\n%d %d\n65535\n" % (w, h)
    assert data.startswith(header) and len(data) == len(header) + 2 * w * h
    return np.frombuffer(data, ">u2", w * h, len(header)).reshape(h, w)


def test_cli_adaptive(tmp_path):
    plain, out, cnt = str(tmp_path / "plain.ppm"), str(tmp_path / "out.ppm"), str(tmp_path / "counts.pgm")
    _cli(plain, 2)
    # a threshold nothing exceeds: two passes of k = 1, then no round; the plain 2-spp frame
    stdout = _cli(out, 3, RT_ADAPT="1e30", RT_PASS_SPP="1", RT_COUNTS_OUT=cnt)
    assert "refined" not in stdout
    assert open(out, "rb").read() == open(plain, "rb").read()
    assert (_pgm(cnt, 33, 17) == 2).all()
    # threshold 0: every round raises every pixel; the reference's 3-spp frame
    stdout = _cli(out, 3, RT_ADAPT="0", RT_PASS_SPP="1", RT_COUNTS_OUT=cnt)
    assert [l for l in stdout.splitlines() if "refined" in l] == [f"Progress: refined {33 * 17} pixels to 3 samples"]
    assert open(out, "rb").read() == open(os.path.join(rtref.GOLD, "cornell_33x17x3.ppm"), "rb").read()
    assert (_pgm(cnt, 33, 17) == 3).all()
    # a threshold in between leaves a mixed map, and the checkpoint of it resumes
    prefix = str(tmp_path / "ck")
    _cli(out, 6, RT_ADAPT="0.5", RT_PASS_SPP="2", RT_COUNTS_OUT=cnt, RT_CHECKPOINT=prefix)
    counts = _pgm(cnt, 33, 17)
    assert set(np.unique(counts)) <= {4, 6} and counts.max() == 6
    first = open(out, "rb").read()
    stdout = _cli(out, 6, RT_ADAPT="0.5", RT_PASS_SPP="2", RT_COUNTS_OUT=cnt, RT_CHECKPOINT=prefix)
    assert "Resumed from" in stdout and "at 6 samples" in stdout and "refined" not in stdout
    assert open(out, "rb").read() == first and np.array_equal(_pgm(cnt, 33, 17), counts)
