"""The geoedge chain on the CPU: reference -> golden -> oracle, on degenerate
geometry and rays built to sit on the edges (tests/geoedge_util.py).  First the goldens are
shown to reach those edges (the class floors, read from the reference's own answers), then the
oracle is pinned to them with rtref.same (bit for bit, NaN equals NaN).  The device's side of
the chain is tests/test_gpu_geoedge.py."""
import numpy as np
import pytest

import geoedge_util as gu
import rtref

W, H, S = 24, 16, 4


@pytest.fixture(scope="module")
def gold():
    return rtref.golden("geoedge_rays.rtd")


@pytest.fixture(scope="module")
def rays_in():
    return rtref.golden("geoedge_rays_in.rtd")


@pytest.fixture(scope="module")
def arrays(rt):
    return rtref.ref_arrays(rt, "geoedge", 64, 64, 1)


def _cls(rays_in, name):
    return rays_in["cls"] == gu.CLASSES.index(name)


def test_generator_reproduces_the_committed_rays(arrays, rays_in, gold):
    org, dirs, cls = gu.geoedge_rays(arrays)
    assert np.array_equal(rtref.bits(org), rtref.bits(rays_in["origin"]))
    assert np.array_equal(rtref.bits(dirs), rtref.bits(rays_in["direction"]))
    assert np.array_equal(cls, rays_in["cls"])
    # ref_harness rays_from recorded exactly these rays, in this order
    assert np.array_equal(rtref.bits(gold["origin"]), rtref.bits(org))
    assert np.array_equal(rtref.bits(gold["direction"]), rtref.bits(dirs))
    assert 2000 <= len(org) <= 6000
    assert all((cls == k).any() for k in range(len(gu.CLASSES)))


def test_same_rule():
    nan_neg = np.array([0xffc00000], np.uint32).view(np.float32)
    nan_pos = np.array([0x7fc00001], np.uint32).view(np.float32)
    assert rtref.same(nan_neg, nan_pos).all()
    assert not rtref.same(np.float32([0.0]), np.float32([-0.0])).any()
    assert not rtref.same(np.float32([1.0]), np.nextafter(np.float32([1.0]), np.float32(2))).any()
    assert not rtref.same(nan_neg, np.float32([np.inf])).any()
    assert rtref.same(np.int64([3, -1]), np.int32([3, -1])).all()


# ---------------------------------------------------------------- class floors (non-vacuity)
def test_floor_edge(gold, rays_in):
    m = _cls(rays_in, "edge") & gold["hit"].astype(bool)
    u, v = gold["uv"][m, 0], gold["uv"][m, 1]
    on = np.stack([u == 0, v == 0, (u + v).astype(np.float32) == 1], 1)
    assert on.any(1).sum() >= 32, on.any(1).sum()
    assert (on.sum(1) >= 2).sum() >= 8, (on.sum(1) >= 2).sum()


def test_floor_tie(gold, rays_in, arrays):
    m = _cls(rays_in, "tie") & gold["hit"].astype(bool)
    n = np.isin(gold["object_id"][m], gu.partner_triangles(arrays)).sum()
    assert n >= 32, n


def test_floor_t0(gold, rays_in):
    m = _cls(rays_in, "t0")
    hit = gold["hit"].astype(bool)
    zero = (m & hit & (gold["t"] == 0)).sum()
    tested = (m & ~hit & (gold["n_tri"] > 0)).sum()
    assert zero >= 16 and tested >= 16, (zero, tested)


def test_floor_det(rays_in):
    m = _cls(rays_in, "det")
    t = gu.parts()["Lattice"][0]
    det = np.array([gu.det_f32(t[1] - t[0], t[2] - t[0], d) for d in rays_in["direction"][m]], np.float32)
    thr = gu.DET_THRESHOLD
    counts = {(s, side): int(((np.sign(det) == s) & ((np.abs(det) < thr) == (side == "below"))).sum())
              for s in (1, -1) for side in ("below", "above")}
    assert min(counts.values()) >= 16, counts
    assert np.abs(det).min() >= np.float32(0.45e-6) and np.abs(det).max() <= np.float32(2.2e-6)
    # the threshold itself and the float below it, on both signs
    for s in (1, -1):
        assert (det == np.float32(s) * thr).any() and (det == np.float32(s) * gu._step(thr, -1)).any(), s


def test_det_class_straddles_the_reference_threshold(gold, rays_in):
    """The reference tests the grazed triangle and takes it on one side of 1e-6 only."""
    m = _cls(rays_in, "det")
    t = gu.parts()["Lattice"][0]
    det = np.array([gu.det_f32(t[1] - t[0], t[2] - t[0], d) for d in rays_in["direction"][m]], np.float32)
    uv = gold["uv"][m]
    grazed = gold["hit"][m].astype(bool) & (gold["t"][m] < 2.0)
    assert np.array_equal(grazed, ~(np.abs(det) < gu.DET_THRESHOLD)), "float32 restatement of det disagrees with the reference"
    assert grazed.sum() >= 32 and (~grazed).sum() >= 32 and np.isfinite(uv).all()


def test_floor_far(gold, rays_in):
    m = _cls(rays_in, "far")
    hit = gold["hit"].astype(bool)
    culled = (m & ~hit & (gold["n_aabb"] > 1)).sum()
    long_hits = (m & hit & (gold["t"] > 1e8)).sum()
    assert culled >= 8 and long_hits >= 8, (culled, long_hits)


def test_far_class_straddles_the_entry_distance_cull(gold, rays_in):
    """The axis rays whose origins lie within four floats of 1e9 from the room: on each of the
    six directions the reference's AABB count takes two values, the larger one up to exactly
    1e9 (the room's subtree is entered), the smaller beyond (entry distance > 1e9: culled)."""
    m = _cls(rays_in, "far")
    o, d = rays_in["origin"], rays_in["direction"]
    for axis in range(3):
        for sign in (1, -1):
            k = np.flatnonzero(m & (np.abs(sign * o[:, axis] - 1e9) <= 256) & (d[:, axis] == -sign) & ((d != 0).sum(1) == 1))
            dist, n = sign * o[k, axis].astype(np.float64), gold["n_aabb"][k]
            assert len(k) == 9 and len(set(n.tolist())) == 2, (axis, sign, n)
            assert n[dist <= 1e9].min() > n[dist > 1e9].max(), (axis, sign, dist, n)


def test_floor_light(gold, rays_in):
    p = gold["light_pdf"][_cls(rays_in, "light")]
    zero, positive = (p == 0).sum(), (np.isfinite(p) & (p > 0)).sum()
    other = (~np.isfinite(p)).sum()
    assert zero >= 8 and positive >= 8, f"pdf 0: {zero}, finite positive: {positive}, infinite or NaN: {other}"


def test_floor_axis(rays_in, arrays):
    m = _cls(rays_in, "axis")
    o, d = rays_in["origin"][m], rays_in["direction"][m]
    node = np.asarray(arrays["node"], np.float32)
    on = np.zeros(len(o), bool)
    for i in range(3):
        planes = np.unique(np.concatenate([node[:, i], node[:, 3 + i]]))
        on |= (d[:, i] == 0) & np.isin(o[:, i], planes)
    assert on.sum() >= 64, on.sum()
    # both signs of zero, one and two zero components
    assert (np.signbit(d) & (d == 0)).any() and (~np.signbit(d) & (d == 0)).any()
    assert ((d == 0).sum(1) == 1).any() and ((d == 0).sum(1) == 2).any()


def test_reference_answers_cover_the_special_values(gold, rays_in):
    """What the remaining classes are there for, read from the golden."""
    hit = gold["hit"].astype(bool)
    sc, nf = _cls(rays_in, "scale"), _cls(rays_in, "nonfinite")
    assert (sc & hit).sum() >= 16 and (sc & ~hit).sum() >= 16     # 1e-20 directions hit, 1e20 ones are zero rays
    assert nf.sum() >= 12
    d = rays_in["direction"]
    assert (~np.isfinite(d[nf])).any() and (d[nf] == 0).all(1).any() and np.isnan(rays_in["origin"][nf]).any()


# ---------------------------------------------------------------- oracle against reference
def test_oracle_rays_match_reference(oracle, arrays, rays_in, gold):
    out_f, out_i = oracle.rays(arrays, rays_in["origin"], rays_in["direction"])
    gu.check_rays(rays_in, gold, out_f, out_i, "oracle")


def test_oracle_frame_matches_reference(rt, oracle):
    g = rtref.sums_golden("geoedge", W, H, S)
    out, cnt, _ = oracle.render(rtref.ref_arrays(rt, "geoedge", W, H, S), S)
    assert rtref.same(out, g["sums"].reshape(-1, 3)).all()
    assert list(cnt) == list(g["counters"])


def test_frame_sees_the_edge_meshes(rt, oracle):
    """At least 10% of the frame's pixel-centre rays first-hit a triangle outside the room's
    walls and light; at most 2% of the golden's pixels are non-finite."""
    a = rtref.ref_arrays(rt, "geoedge", W, H, S)
    f, i = oracle.rays(a, *rtref.pixel_centre_rays(a))
    seen = (i[:, 0].astype(bool) & np.isin(i[:, 1], gu.edge_mesh_triangles(a))).mean()
    assert seen >= 0.10, seen
    sums = rtref.sums_golden("geoedge", W, H, S)["sums"].reshape(-1, 3)
    assert (~np.isfinite(sums).all(1)).mean() <= 0.02
    assert np.nanmax(sums) > 0
