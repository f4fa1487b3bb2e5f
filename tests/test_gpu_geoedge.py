"""The device's end of the geoedge chain: every traversal the kernels run, fed
the caller-made rays of tests/geoedge_util.py, against the reference's own answers to them
(tests/golden/geoedge_rays.rtd; the goldens' reach is shown by tests/test_geoedge.py).

rt_intersect_rays_via path 0 is closest_hit / light_pdf, path 1 the per-lane trav_step and
light_step, path 2 trav_step_coop with the plain kernel's constants.  Comparison: rtref.same,
bit for bit with NaN equal to NaN, every field the entry returns.  Ray i is thread i, so the
shuffled order gives path 2's waves another mix of node, leaf and pop lanes; results are per
ray and must not move.  A loop that reaches its bound reports hit = -2, which equals no golden.
The frame through every schedule is test_gpu_edges.py's test_goldens_every_schedule."""
import numpy as np
import pytest

import geoedge_util as gu
import rtref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(rt):
    import torch   # initialises the HIP runtime librt_hw_amd.so shares (see test_gpu_parity.py)
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    if rt.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return rt


@pytest.fixture(scope="module")
def gold():
    return rtref.golden("geoedge_rays.rtd")


@pytest.fixture(scope="module")
def rays_in():
    return rtref.golden("geoedge_rays_in.rtd")


@pytest.fixture(scope="module")
def scenes(gpu):
    return {"reference arrays": gpu.Scene.from_view(rtref.ref_arrays(gpu, "geoedge", 64, 64, 1)),
            "loader": gpu.Scene.load(rtref.scene_path("geoedge"), 64, 64, 1)}


@pytest.mark.parametrize("order", ["generator", "shuffled"])
@pytest.mark.parametrize("source", ["reference arrays", "loader"])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_rays_match_reference(scenes, gold, rays_in, path, source, order):
    n = len(rays_in["cls"])
    perm = np.arange(n) if order == "generator" else np.random.default_rng(20261022).permutation(n)
    f, i = scenes[source].intersect_rays(rays_in["origin"][perm], rays_in["direction"][perm], path=path)
    out_f, out_i = np.empty_like(f), np.empty_like(i)
    out_f[perm], out_i[perm] = f, i
    unfinished = np.flatnonzero(out_i[:, 0] == -2)
    assert len(unfinished) == 0, f"path {path}, {source}, {order}: rays {unfinished[:8].tolist()} reached the step bound"
    gu.check_rays(rays_in, gold, out_f, out_i, f"path {path}, {source}, {order} order:")


@pytest.fixture(scope="module")
def whole(scenes, rays_in):
    """The whole ray set through each path of the loader scene, once."""
    return {path: scenes["loader"].intersect_rays(rays_in["origin"], rays_in["direction"], path=path) for path in (0, 1, 2)}


@pytest.mark.parametrize("n", [1, 64, 257])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_prefix_equals_whole_set(scenes, rays_in, whole, path, n):
    """The first n rays alone give the first n rows of the whole set: a lone lane, one exactly
    full wave, and a block boundary with one ray in the last block (the threads past n of paths 1
    and 2 take ray 0 and must write nothing)."""
    f, i = scenes["loader"].intersect_rays(rays_in["origin"][:n], rays_in["direction"][:n], path=path)
    assert not (i[:, 0] == -2).any(), f"path {path}, n {n}: a ray reached the step bound"
    assert rtref.same(f, whole[path][0][:n]).all() and np.array_equal(i, whole[path][1][:n])


def test_unknown_path_is_refused(gpu, scenes, rays_in):
    with pytest.raises(gpu.RtError, match="unknown path"):
        scenes["loader"].intersect_rays(rays_in["origin"][:4], rays_in["direction"][:4], path=3)


def test_old_entry_is_path_zero(scenes, rays_in):
    s = scenes["loader"]
    (f0, i0), (f1, i1) = s.intersect_rays(rays_in["origin"], rays_in["direction"]), \
        s.intersect_rays(rays_in["origin"], rays_in["direction"], path=0)
    assert rtref.same(f0, f1).all() and np.array_equal(i0, i1)
