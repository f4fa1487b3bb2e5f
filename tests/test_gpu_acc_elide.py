"""The traversal's frame rule on the device (rt_wavefront.h trav_pop ELIDE: a far child that survives
pushes the node's best frame only if the near subtree found a hit).

rt_device_selfcheck 5 runs whole queries through the cooperative step in both forms, with one and two
frames popped per step and with 12 and 4 stack frames in LDS (4 force the scratch path, where a frame
count that is off by one would show), against the per-lane loop that pushes every best frame: eight
launches per uploaded scene, every loop bounded.

Then frames through the plain kernel (the one that takes the rule), through rank 0 of an 8-way split
(the runahead kernel) and through the counting render: cornell 64x64x8 and sponza_mini 64x36x4 against
the reference's committed goldens (row hashes of the sums, and the counters), and sponza_mini 96x54x4,
for which no golden is committed, against the CPU oracle on the same arrays (the oracle is pinned to the
reference by those goldens: tests/test_oracle.py)."""
import numpy as np
import pytest

import rtref
from test_gpu_edges import gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def _counters(st):
    return [st["rays"], st["aabb_tests"], st["tri_tests"], st["light_queries"], st["light_aabb_tests"], st["light_tri_tests"]]


@pytest.mark.parametrize("name", ["cornell", "sponza_mini"])
def test_coop_queries_in_both_forms_match_per_lane_queries(gpu, name):
    scene = gpu.Scene.load(rtref.scene_path(name), 16, 16, 1)
    scene.upload()
    assert gpu.device_selfcheck(5) == 0


_want = {}


def _reference(gpu, oracle, name, w, h, s):
    """(arrays, sums (h, w, 3), counters): the committed golden, or the CPU oracle where none is committed;
    made once per case."""
    key = (name, w, h, s)
    if key not in _want:
        arrays = rtref.ref_arrays(gpu, name, w, h, s)
        if key == ("sponza_mini", 96, 54, 4):
            sums, cnt, _ = oracle.render(arrays, s)
            cnt = [int(c) for c in cnt[:6]]
        else:
            g = rtref.sums_golden(name, w, h, s)
            sums, cnt = g["sums"], [int(c) for c in g["counters"]]
        _want[key] = (arrays, np.asarray(sums, np.float32).reshape(h, w, 3), cnt)
    return _want[key]


@pytest.mark.parametrize("name,w,h,s", [("cornell", 64, 64, 8), ("sponza_mini", 64, 36, 4), ("sponza_mini", 96, 54, 4)])
def test_frames_match_the_reference(gpu, oracle, name, w, h, s):
    arrays, ref, cnt = _reference(gpu, oracle, name, w, h, s)
    assert np.isfinite(ref).all() and ref.max() > 0
    scene = gpu.Scene.from_view(arrays)
    # the plain kernel
    out, st = scene.render_sums(s, runahead=False)
    assert st["schedule"] == gpu.SCHED_LANE
    assert np.array_equal(rtref.row_hash(out), rtref.row_hash(ref))
    # rank 0 of an 8-way split: the runahead kernel
    rows = gpu.shard_rows(h, 0, 8, 8)
    out, st = scene.render_sums(s, rank=0, world=8)
    assert st["schedule"] & gpu.SCHED_RUNAHEAD
    assert np.array_equal(rtref.row_hash(out), rtref.row_hash(ref[rows]))
    # the counting render
    out, st = scene.render_sums(s, count=True)
    assert np.array_equal(rtref.row_hash(out), rtref.row_hash(ref))
    assert _counters(st) == cnt
