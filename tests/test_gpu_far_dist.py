"""The root-free cull on the device: far_gt and the squared 1e9 constant against the device's own
sqrtf (rt_device_selfcheck 3), and the stacked-quad scene of tests/test_far_dist.py, whose far
boxes are entered at an entry distance equal to the near subtree's best, against the CPU oracle."""
import numpy as np
import pytest

import rtref
from test_far_dist import stack_rays, stack_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(rt):
    # torch first: it must initialise the HIP runtime it shares with librt_hw_amd.so
    import torch
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    if rt.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return rt


@pytest.fixture(scope="module")
def stack(gpu, tmp_path_factory):
    arrays = stack_scene(gpu, tmp_path_factory.mktemp("stack"))
    return arrays, gpu.Scene.from_view(arrays)


def test_far_gt_is_exact_on_the_device(gpu):
    assert gpu.device_selfcheck(3) == 0


def test_stack_rays_vs_oracle(stack, oracle):
    arrays, scene = stack
    org, dirs = stack_rays()
    f, i = scene.intersect_rays(org, dirs)
    wf, wi = oracle.rays(arrays, org, dirs)
    hit = wi[:, 0].astype(bool)
    assert hit.sum() >= 24 and (~hit).sum() >= 16
    assert np.array_equal(i[:, 0].astype(bool), hit)
    assert np.array_equal(i[hit, 1], wi[hit, 1])
    assert np.array_equal(rtref.bits(f[hit, 0]), rtref.bits(wf[hit, 0]))
    assert np.array_equal(i[:, 2:4], wi[:, 2:4])   # AABB and triangle tests


def test_stack_render_vs_oracle(stack, oracle):
    """The same scene through the kernels whose traversal carries the new frames (counting,
    runahead and plain lane-resident, wavefront): sums and test counts of the oracle."""
    arrays, scene = stack
    s = 4
    ref, cnt, _ = oracle.render(arrays, s)
    assert ref.any()
    out, st = scene.render_sums(s, count=True)
    assert np.array_equal(rtref.bits(out.reshape(-1, 3)), rtref.bits(ref))
    assert [st["rays"], st["aabb_tests"], st["tri_tests"]] == [int(c) for c in cnt[:3]]
    for kw in ({}, {"runahead": False}, {"kernel": 4}):
        out, _ = scene.render_sums(s, **kw)
        assert np.array_equal(rtref.bits(out.reshape(-1, 3)), rtref.bits(ref)), kw
