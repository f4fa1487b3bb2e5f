"""The shadeedge chain on the CPU: reference -> golden -> host build of the kernel
text, on shading frames built to sit where scene_sample / scene_pdf are singular
(tests/shadeedge_util.py).  First the goldens are shown to reach those places (conditions on the
goldens themselves and on the host build's record of the draws), then the host build is pinned to
them with rtref.same (bit for bit, NaN equals NaN) through both compositions of the pdf: scene_pdf,
and light_step until done followed by scene_pdf_lp.  The device's side is tests/test_gpu_shadeedge.py."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtref
import shadeedge_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "kernel_host.cpp")


@pytest.fixture(scope="module")
def kh(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("kh_shadeedge") / "libkh.so")
    subprocess.run(["g++", "-O2", "-fno-tree-vectorize", "-fno-tree-slp-vectorize", "-ffp-contract=off", "-fopenmp",
                    "-std=c++17", "-shared", "-fPIC", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    V = ctypes.c_void_p
    lib.kh_sample_frames.argtypes = [V, ctypes.c_int, ctypes.c_int64, V, V, V, V, V]
    lib.kh_sample_frames.restype = None
    lib.kh_sampler_trace.argtypes = [ctypes.c_int, ctypes.c_int64, V, V, V, V]
    lib.kh_sampler_trace.restype = None
    return lib


@pytest.fixture(scope="module")
def sets(rt):
    """scene -> (arrays, the committed frames, the reference's answers)."""
    return {s: (su.scene_arrays(rt, s), rtref.golden(f"shadeedge_{s}_in.rtd"), rtref.golden(f"shadeedge_{s}.rtd"))
            for s in su.SCENES}


def host_frames(rt, kh, arrays, fin, path):
    v, keep = rt.make_view(arrays)
    n = len(fin["seed"])
    frame, seed, warm = (np.ascontiguousarray(fin[k]) for k in ("frame", "seed", "warm"))
    out_f, out_i = np.zeros((n, 6), np.float32), np.zeros((n, 4), np.int64)
    kh.kh_sample_frames(ctypes.addressof(v), path, n, frame.ctypes.data, seed.ctypes.data, warm.ctypes.data, out_f.ctypes.data,
                        out_i.ctypes.data)
    del keep
    return out_f, out_i


def host_trace(kh, n_lights, fin):
    n = len(fin["seed"])
    seed, warm = np.ascontiguousarray(fin["seed"]), np.ascontiguousarray(fin["warm"])
    tf, ti = np.zeros((n, 4), np.float32), np.zeros((n, 3), np.int64)
    kh.kh_sampler_trace(n_lights, n, seed.ctypes.data, warm.ctypes.data, tf.ctypes.data, ti.ctypes.data)
    return {"s": tf[:, 0], "pick": tf[:, 1], "u": tf[:, 2], "v": tf[:, 3], "sampler": ti[:, 0], "rejected": ti[:, 1],
            "next": ti[:, 2]}


def _cls(fin, name):
    return fin["cls"] == su.CLASSES.index(name)


def _nan_rows(gold):
    return np.isnan(gold["dir"]).any(1) | np.isnan(gold["pdf"]) | np.isnan(gold["light_pdf"]) | np.isnan(gold["next_normal"])


def _exact_minus_z(fin):
    n = fin["frame"][:, 3:6]
    return (n[:, 0] == 0) & (n[:, 1] == 0) & (n[:, 2] == -1)


# ---------------------------------------------------------------- the inputs
@pytest.mark.parametrize("scene", su.SCENES)
def test_generator_reproduces_the_committed_frames(sets, scene):
    arrays, fin, gold = sets[scene]
    made = su.shadeedge_frames(arrays)
    assert np.array_equal(rtref.bits(made["frame"]), rtref.bits(fin["frame"]))
    for k in ("seed", "warm", "cls"):
        assert made[k].dtype == fin[k].dtype and np.array_equal(made[k], fin[k]), k
    n = len(fin["seed"])
    assert n <= 4096 and len(gold["pdf"]) == n
    assert fin["seed"].min() >= 1 and fin["seed"].max() <= 2147483646
    assert set(np.unique(fin["warm"]).tolist()) == {0, 1}
    assert ((fin["warm"] == 1) == _cls(fin, "warm")).all()
    for name in ("shadeedge_%s_in.rtd" % scene, "shadeedge_%s.rtd" % scene):
        assert os.path.getsize(os.path.join(rtref.GOLD, name)) < 1000000


@pytest.mark.parametrize("scene", su.SCENES)
def test_every_class_is_present_and_runs_every_sampler(sets, kh, scene):
    arrays, fin, gold = sets[scene]
    n_lights = len(arrays["light"])
    t = host_trace(kh, n_lights, fin)
    for name in su.CLASSES:
        m = _cls(fin, name)
        if name == "light" and not n_lights:
            assert not m.any()
            continue
        assert m.any(), name
        for sampler in range(3 if n_lights else 2):
            assert (t["sampler"][m] == sampler).sum() >= 16, (name, sampler, int((t["sampler"][m] == sampler).sum()))
    assert _cls(fin, "generic").sum() == 256


@pytest.mark.parametrize("scene", su.SCENES)
def test_trace_follows_the_sampler(sets, rt, kh, scene):
    """The restated draws of kh_sampler_trace end in the engine state scene_sample itself ends in."""
    arrays, fin, gold = sets[scene]
    t = host_trace(kh, len(arrays["light"]), fin)
    assert np.array_equal(t["next"], host_frames(rt, kh, arrays, fin, 0)[1][:, 1])


@pytest.mark.parametrize("scene", su.SCENES)
def test_branch_aims_hold_on_the_host_build(sets, kh, scene):
    arrays, fin, gold = sets[scene]
    n_lights = len(arrays["light"])
    t = host_trace(kh, n_lights, fin)
    rows = np.flatnonzero(_cls(fin, "branch"))
    aims = [a for a, (_, needs_lights) in su.AIMS.items() if n_lights or not needs_lights]
    assert len(rows) == su.AIM_FRAMES * len(aims)
    for k, aim in enumerate(aims):
        r = rows[su.AIM_FRAMES * k:su.AIM_FRAMES * (k + 1)]
        with np.errstate(all="ignore"):
            ok = su.AIMS[aim][0]({f: v[r] for f, v in t.items()})
        assert ok.all() and len(r) >= 8, (aim, {f: v[r].tolist() for f, v in t.items()})


def test_aims_without_lights_are_the_reachable_ones():
    """Without a light list s = (u + 1) * 1.5 / 1.5 never exceeds 2 (the largest uniform gives the float
    below it), so `s <= 2.f` has one side there; the light aims need a light."""
    top = su.mixture_s(np.arange(su.M - 400, su.M, dtype=np.uint64), False)
    assert top.max() < 2
    assert sorted(su.aimed_seeds(False)) == sorted(a for a, (_, needs) in su.AIMS.items() if not needs)
    assert sorted(su.aimed_seeds(True)) == sorted(su.AIMS)


@pytest.mark.parametrize("scene", su.SCENES)
def test_class_reach(sets, scene):
    """What the classes are there for, read from the frames and from the reference's answers."""
    arrays, fin, gold = sets[scene]
    f = fin["frame"]
    ax, an, ro = _cls(fin, "axis"), _cls(fin, "antipode"), _cls(fin, "rough")
    n, eye = f[:, 3:6], f[:, 6:9]
    assert (_exact_minus_z(fin) & ax & np.signbit(n[:, 1])).any() and (_exact_minus_z(fin) & ax & ~np.signbit(n[:, 1])).any()
    dot = (eye[:, 0] * n[:, 0] + eye[:, 1] * n[:, 1]).astype(np.float32) + eye[:, 2] * n[:, 2]
    for m in (ax, an):
        assert (m & (dot == 0)).sum() >= 16 and (m & (dot > 0) & (dot < 4e-6)).sum() >= 16 and (m & (dot < 0) & (dot > -4e-6)).sum() >= 16
        assert (m & (eye == -n).all(1)).any() and (m & (eye == n).all(1)).any()
    off = np.hypot(n[an, 0].astype(np.float64), n[an, 1]) / np.abs(n[an, 2])
    for d in (1e-3, 1e-5, 1e-7, 3e-8):
        assert ((off > 0.9 * d) & (off < 1.6 * d)).any(), d
    assert not _exact_minus_z(fin)[an].any()
    lim = np.array([su.R2_LIMIT], np.float32)
    for r2 in (lim[0], np.nextafter(lim, np.float32(0))[0], np.nextafter(lim, np.float32(1))[0], 0.25, 1, 2, 1e-3, 1e-6):
        assert (f[ro, 9] == np.float32(r2)).sum() >= 16, r2
    nf = _cls(fin, "nonfinite")
    assert np.isnan(n[nf]).any() and np.isinf(n[nf]).any() and (n[nf] == 0).all(1).any()
    assert np.isnan(f[nf, 0:3]).any() and np.isinf(f[nf, 0:3]).any() and (eye[nf] == 0).all(1).any()


def test_light_class_aims_at_shared_edges(sets, kh):
    """practice6_1's light quads: every light triangle's hypotenuse is another's.  The light sampler with
    u + v == 1 draws the direction through a point of that edge."""
    arrays, fin, gold = sets["practice6_1"]
    L = np.asarray(arrays["light"], np.float64)
    v0, v1, v2 = (np.round(v, 6) for v in (L[:, 0:3], L[:, 0:3] + L[:, 3:6], L[:, 0:3] + L[:, 6:9]))
    edge = lambda a, b: [tuple(sorted([tuple(p), tuple(q)])) for p, q in zip(a, b)]
    uses = collections.Counter(edge(v0, v1) + edge(v0, v2) + edge(v1, v2))
    assert all(uses[e] == 2 for e in edge(v1, v2))
    t = host_trace(kh, len(L), fin)
    m = _cls(fin, "light") & (t["sampler"] == 2)
    assert (m & (t["u"] + t["v"] == 1)).sum() >= 8 and (m & (t["u"] + t["v"] > 1)).sum() >= 8


@pytest.mark.parametrize("scene", ["cornell", "geoedge", "practice6_1"])
def test_ray_light_pdf_is_the_ray_entrys_answer(sets, oracle, scene):
    """`ray_light_pdf` is ManyLightsDistribution::pdf through Ray(point, dir), which normalises the drawn
    direction once more: the oracle's ray entry equals it on every finite row.  It equals `light_pdf`
    wherever normalising dir is the identity, and only there is it bound to: elsewhere the reference's two
    values differ by an ulp on some rows, which is why tests/test_gpu_shadeedge.py compares as it does."""
    import geoedge_util as gu
    arrays, fin, gold = sets[scene]
    point, d = fin["frame"][:, 0:3], gold["dir"]
    finite = np.isfinite(point).all(1) & np.isfinite(d).all(1)
    f, _ = oracle.rays(arrays, point[finite], d[finite])
    assert rtref.same(f[:, 3], gold["ray_light_pdf"][finite]).all()
    fixed = np.array([np.array_equal(rtref.bits(gu.ray_dir(v)), rtref.bits(v)) for v in d[finite]])
    same = rtref.same(gold["ray_light_pdf"][finite], gold["light_pdf"][finite])
    assert same[fixed].all() and fixed.mean() >= 0.5
    assert (~same).sum() >= 16, "the renormalised direction no longer moves the reference's light pdf"


@pytest.mark.parametrize("scene", ["cornell", "geoedge", "practice6_1"])
def test_light_class_reach(sets, scene):
    """Points on a light's plane, vertices, edges and centroid, just off it, inside the light BVH's root box
    and 1e3 and 1e6 away from it: zero and finite positive light pdfs, walks that test triangles."""
    arrays, fin, gold = sets[scene]
    m = _cls(fin, "light")
    lp = gold["light_pdf"][m]
    assert (lp == 0).sum() >= 8 and (np.isfinite(lp) & (lp > 0)).sum() >= 8, ((lp == 0).sum(), (np.isfinite(lp) & (lp > 0)).sum())
    assert (gold["n_light_tri"][m] > 0).sum() >= 8
    root = np.asarray(arrays["light_node"], np.float32)[0, :6]
    p = fin["frame"][m, 0:3]
    inside = ((p >= root[:3]) & (p <= root[3:])).all(1)
    far = np.abs(p - (root[:3] + root[3:]) / 2).max(1)
    assert inside.sum() >= 8 and ((far > 9e2) & (far < 2e3)).sum() >= 8 and (far > 9e5).sum() >= 8


# ---------------------------------------------------------------- the caps
@pytest.mark.parametrize("scene", su.SCENES)
def test_nan_share_and_pdf_signs(sets, scene):
    arrays, fin, gold = sets[scene]
    nan = _nan_rows(gold)
    assert nan.mean() <= 0.25, nan.mean()
    free = ~_cls(fin, "nonfinite") & ~(_cls(fin, "axis") & _exact_minus_z(fin))
    for name in su.CLASSES:
        m = _cls(fin, name) & free
        if m.any():
            assert nan[m].mean() <= 0.40, (name, nan[m].mean())
    pdf = gold["pdf"]
    assert (pdf < 0).any() and (pdf == 0).any() and (pdf > 0).any(), ((pdf < 0).sum(), (pdf == 0).sum(), (pdf > 0).sum())


# ---------------------------------------------------------------- host build against reference
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("scene", su.SCENES)
def test_host_build_matches_reference(sets, rt, kh, scene, path):
    arrays, fin, gold = sets[scene]
    out_f, out_i = host_frames(rt, kh, arrays, fin, path)
    su.check_frames(fin, gold, out_f, out_i, f"host build, {scene}, path {path}:")
