"""The device's end of the shadeedge chain: scene_sample and both compositions of
the pdf as the kernels compile them, fed the caller-made shading frames of tests/shadeedge_util.py,
against the reference's own answers to them (tests/golden/shadeedge_<scene>.rtd; the goldens' reach
is shown by tests/test_shadeedge.py).

rt_sample_frames_via path 0 is scene_sample then scene_pdf<true> over a LocalStack, path 1
scene_sample, the light_step walk and scene_pdf_lp.  Comparison: rtref.same, bit for bit with NaN
equal to NaN, every field the entry returns.  Frame i is thread i, so the shuffled order gives the
waves another mix of samplers and walk lengths; results are per frame and must not move.  A walk that
reaches its bound reports status -2, which no test accepts.  No tolerance anywhere."""
import numpy as np
import pytest

import geoedge_util as gu
import rtref
import shadeedge_util as su

pytestmark = pytest.mark.gpu

SOURCES = su.SCENES + ["cornell through the loader"]


@pytest.fixture(scope="module")
def gpu(rt):
    import torch   # initialises the HIP runtime librt_hw_amd.so shares (see test_gpu_parity.py)
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    if rt.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return rt


def _set(source):
    scene = "cornell" if source == "cornell through the loader" else source
    return rtref.golden(f"shadeedge_{scene}_in.rtd"), rtref.golden(f"shadeedge_{scene}.rtd")


@pytest.fixture(scope="module")
def scenes(gpu):
    s = {name: gpu.Scene.from_view(su.scene_arrays(gpu, name)) for name in su.SCENES}
    s["cornell through the loader"] = gpu.Scene.load(rtref.scene_path("cornell"), 64, 64, 1)
    return s


@pytest.fixture(scope="module")
def whole(scenes):
    """(source, path) -> the whole set through that path in generator order, once."""
    out = {}
    for source in SOURCES:
        fin, _ = _set(source)
        for path in (0, 1):
            out[source, path] = scenes[source].sample_frames(fin["frame"], fin["seed"], fin["warm"], path=path)
    return out


@pytest.mark.parametrize("order", ["generator", "shuffled"])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("path", [0, 1])
def test_frames_match_reference(scenes, whole, path, source, order):
    fin, gold = _set(source)
    if order == "generator":
        out_f, out_i = whole[source, path]
    else:
        n = len(fin["cls"])
        perm = np.random.default_rng(20261104).permutation(n)
        f, i = scenes[source].sample_frames(fin["frame"][perm], fin["seed"][perm], fin["warm"][perm], path=path)
        out_f, out_i = np.empty_like(f), np.empty_like(i)
        out_f[perm], out_i[perm] = f, i
    su.check_frames(fin, gold, out_f, out_i, f"path {path}, {source}, {order} order:")


@pytest.mark.parametrize("source", SOURCES)
def test_both_compositions_agree(whole, source):
    """scene_pdf against light_step + scene_pdf_lp, field by field, status and counts included."""
    (f0, i0), (f1, i1) = whole[source, 0], whole[source, 1]
    for k, name in enumerate(su.FIELDS[:6]):
        bad = np.flatnonzero(~rtref.same(f0[:, k], f1[:, k]))
        assert len(bad) == 0, f"{source} {name}: paths 0 and 1 differ on frames {bad[:8].tolist()}"
    assert np.array_equal(i0, i1), np.flatnonzero((i0 != i1).any(1))[:8].tolist()


@pytest.mark.parametrize("n", [1, 64, 257])
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("source", ["geoedge", "cornell_nolights"])
def test_prefix_equals_whole_set(scenes, whole, source, path, n):
    """The first n frames alone give the first n rows of the whole set: a lone lane, one exactly full
    wave, and a block boundary with one frame in the last block."""
    fin, _ = _set(source)
    f, i = scenes[source].sample_frames(fin["frame"][:n], fin["seed"][:n], fin["warm"][:n], path=path)
    assert rtref.same(f, whole[source, path][0][:n]).all() and np.array_equal(i, whole[source, path][1][:n])


@pytest.mark.parametrize("source", ["cornell", "geoedge", "practice6_1"])
def test_light_pdf_column_against_the_ray_entry(scenes, whole, source):
    """The light pdf column against rt_intersect_rays' light pdf for the ray (point, dir), wherever point
    and dir are finite.  The ray entry builds Ray(point, dir) first, as ref_harness `rays` does, and so
    normalises dir once more; in the reference itself that moves the pdf by an ulp on about a tenth of the
    frames (221 of 2565 finite rows on cornell, 127 of 2565 on geoedge, 288 of 2781 on practice6_1;
    tests/test_shadeedge.py shows it on the goldens).  So the ray entry is held to the reference's own answer for that
    ray on every finite row (`ray_light_pdf`, recorded by samplers_from through Ray::Ray), and to the
    column itself wherever normalising dir is the identity (gu.ray_dir, bit for bit), where both walks
    see the same ray and the same direction.  Both comparisons are exact."""
    fin, gold = _set(source)
    out_f, _ = whole[source, 0]
    point, d = fin["frame"][:, 0:3], out_f[:, 0:3]
    finite = np.isfinite(point).all(1) & np.isfinite(d).all(1)
    rf, _ = scenes[source].intersect_rays(point[finite], d[finite])
    bad = np.flatnonzero(~rtref.same(rf[:, 3], gold["ray_light_pdf"][finite]))
    assert len(bad) == 0, f"{source}: the ray entry differs from the reference on finite rows {bad[:8].tolist()}"
    fixed = np.array([np.array_equal(rtref.bits(gu.ray_dir(v)), rtref.bits(v)) for v in d[finite]])
    assert fixed.sum() >= 0.5 * finite.sum()
    bad = np.flatnonzero(fixed & ~rtref.same(rf[:, 3], out_f[finite, 4]))
    assert len(bad) == 0, f"{source}: the column differs from the ray entry on finite rows {bad[:8].tolist()}"


def test_unknown_path_is_refused(gpu, scenes):
    fin, _ = _set("cornell")
    with pytest.raises(gpu.RtError, match="unknown path"):
        scenes["cornell"].sample_frames(fin["frame"][:4], fin["seed"][:4], fin["warm"][:4], path=2)
