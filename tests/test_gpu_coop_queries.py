"""Whole closest-hit queries through the cooperative traversal step on the device
(rt_wavefront.h trav_step_coop, rt_device_selfcheck 5): 16,384 hashed rays per uploaded scene,
in waves that hold the real mix of node, leaf and pop lanes, against the per-lane trav_step loop
in the same kernel; t, triangle, local best and the AABB and triangle counts bit for bit.  One
and two frames popped per step (the plain and the runahead kernel's caps), each with 12 and with
4 stack frames in LDS, so that lanes hold frames in scratch too.  Every query loop is bounded by
4 x (nodes + triangles) + 64 steps and a lane still traversing there is a mismatch, so a
liveness bug fails here instead of hanging.  cornell's tree has 19 nodes: its waves are mostly at
leaves."""
import pytest

import rtref
from test_gpu_edges import gpu  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["cornell", "cornell_blob", "sponza_mini"])
def test_coop_queries_match_per_lane_queries(gpu, name):
    scene = gpu.Scene.load(rtref.scene_path(name), 16, 16, 1)
    scene.upload()
    assert gpu.device_selfcheck(5) == 0
