"""GPU parity of the shading pass with RT_SHADE_CONVERGE (rt_path.h: one ray start per pass for
the bounce and the next sample, the lane's RNG state read where the sampler draws from it) in the
kernel that takes it and, through every schedule, beside the ones that keep the parent form.

As in test_gpu_edges.py, every assertion is bit equality of the float32 sums (and of the six
traversal counters where the schedule counts) against the CPU oracle on the same arrays, through
every schedule (lane-resident, natural order, wavefront, light-split, runahead, 8-way shards).
The cases: the textured fixture, the untextured one, a scene without lights (the mixture then
picks between cosine and VNDF only, and no lane draws a light sample), and a frame of 35 pixels,
whose one wave runs the pass with most lanes idle."""
import numpy as np
import pytest

import rtref
from test_gpu_edges import _changed, _check_variants, cornell_base, gpu, sponza_base  # noqa: F401

pytestmark = pytest.mark.gpu


def test_sponza_mini(gpu, oracle, sponza_base):
    a, ref = sponza_base
    cnt = oracle.render(a, 4)[1]
    _check_variants(gpu, gpu.Scene.from_view(a), 4, ref.reshape(27, 48, 3), cnt, "sponza_mini")


def test_cornell(gpu, oracle, cornell_base):
    a, ref = cornell_base
    cnt = oracle.render(a, 8)[1]
    _check_variants(gpu, gpu.Scene.from_view(a), 8, ref.reshape(17, 33, 3), cnt, "cornell")


def test_without_lights(gpu, oracle, cornell_base):
    """The light list emptied (n_lights == 0): SceneDistribution::sample picks cosine or VNDF
    with one division more, and the pdf has two terms."""
    base, base_ref = cornell_base
    a = dict(base)
    a["light"] = np.zeros((0, 16), np.float32)
    a["light_node"] = np.zeros((0, 8), np.float32)
    ref, cnt, _ = oracle.render(a, 8)
    assert _changed(ref, base_ref) >= 0.10
    _check_variants(gpu, gpu.Scene.from_view(a), 8, ref.reshape(17, 33, 3), cnt, "cornell without lights")


def test_35_pixels(gpu, oracle):
    """7 x 5 pixels: 35 of a wave's 64 lanes ever hold a pixel, and fewer every pass."""
    w, h, s = 7, 5, 16
    a = rtref.ref_arrays(gpu, "sponza_mini", w, h, s)
    ref, cnt, _ = oracle.render(a, s)
    assert np.isfinite(ref).all() and (ref > 0).any()
    _check_variants(gpu, gpu.Scene.from_view(a), s, ref.reshape(h, w, 3), cnt, "sponza_mini 7x5")
