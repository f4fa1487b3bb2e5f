"""Posable meshes on the host (include/rt_hw.h rt_scene_pose_meshes, rt_pose_view, rt_scene_set_rest;
the rule is raytracing-hw_amd/csrc/rt_pose.h): a mesh posed with matrix M holds the records the
reference's loader makes of the same glTF whose node carries M.  The expected arrays are the reference's
own dumps of the variant files (tests/golden/pose_*_dump.rtd, tools/make_pose_goldens.py); every equality
is bit equality."""
from fractions import Fraction

import numpy as np
import pytest

import pose_util
import rtref
from refit_util import bits, f32, np_refit, tri_mesh

VARIANTS = list(pose_util.VARIANTS)
KEYS = ["tri", "tri_attr", "tri_tan", "node", "light", "light_node", "mesh_f", "mesh_tex", "mesh_normal_transform"]


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


@pytest.fixture(scope="module")
def vdir(tmp_path_factory):
    return tmp_path_factory.mktemp("pose_variants")


_posed = {}


def posed(rt, variant):
    """(the base fixture loaded and posed to the variant's matrices, its view before, its view after);
    shared: read only."""
    if variant not in _posed:
        s = rt.Scene.load(rtref.scene_path(pose_util.VARIANTS[variant][0]), 64, 64, 1)
        before = s.view()
        s.enable_poses()
        s.pose(pose_util.pose_matrices(rt, variant))
        _posed[variant] = (s, before, s.view())
    return _posed[variant]


# ------------------------------------------------------------------------ 1. the chain's first link
@pytest.mark.parametrize("variant", VARIANTS)
def test_loader_is_the_references_on_the_variants(rt, vdir, variant):
    ref, path = pose_util.variant_golden(rt, variant, vdir)
    mine = rt.Scene.load(path, 64, 64, 1).view()
    for k in KEYS:
        assert same(mine[k], ref[k].astype(mine[k].dtype)), k
    base = rt.Scene.load(rtref.scene_path(pose_util.VARIANTS[variant][0]), 64, 64, 1).view()
    assert not same(mine["tri"], base["tri"])   # the variant is another scene


# ------------------------------------------------------------------------ 2. rest data restates the load
@pytest.mark.parametrize("name", ["cornell", "cornell_blob", "practice6_1", "texedge", "geoedge"])
def test_rest_data_restates_the_load(rt, name):
    s = rt.Scene.load(rtref.scene_path(name), 64, 64, 1)
    v, r = s.view(), s.rest()
    assert r["rest"].shape == (len(v["tri"]), 18) and sorted(r["tri_source"]) == list(range(len(v["tri"])))
    for m in range(len(v["mesh_f"])):
        assert same(s.mesh_transform(m), r["mesh_matrix"][m])
    wiped = dict(v, tri=np.full_like(v["tri"], 7), mesh_normal_transform=np.full_like(v["mesh_normal_transform"], 7))
    wiped["tri_attr"] = v["tri_attr"].copy()
    wiped["tri_attr"][:, 0:9] = 7
    tri, attr, mnt = rt.pose_view(wiped, r["rest"], {m: r["mesh_matrix"][m] for m in range(len(v["mesh_f"]))})
    assert same(tri, v["tri"]) and same(attr, v["tri_attr"]) and same(mnt, v["mesh_normal_transform"])


# ------------------------------------------------------------------------ 3. a pose is the reference's load
@pytest.mark.parametrize("variant", VARIANTS)
def test_pose_is_the_references_load_of_that_pose(rt, vdir, variant):
    ref, path = pose_util.variant_golden(rt, variant, vdir)
    s, before, v = posed(rt, variant)
    place = pose_util.through_source(s.tri_source(), rt.Scene.load(path, 64, 64, 1).tri_source())
    assert same(v["tri"], ref["tri"][place])
    assert same(v["tri_attr"][:, 0:9], ref["tri_attr"][place, 0:9])
    assert same(v["tri_attr"], ref["tri_attr"][place]) and same(v["tri_tan"], ref["tri_tan"][place])
    assert same(v["mesh_normal_transform"], ref["mesh_normal_transform"])
    meshes = list(pose_util.pose_matrices(rt, variant))
    still = ~np.isin(tri_mesh(before), meshes)
    assert still.any() and not still.all()
    assert same(v["tri"][still], before["tri"][still]) and same(v["tri_attr"][still], before["tri_attr"][still])
    assert not same(v["tri"][~still], before["tri"][~still])
    assert same(v["tri_attr"][:, 9:16], before["tri_attr"][:, 9:16]) and same(v["tri_tan"], before["tri_tan"])
    assert same(v["node"], np_refit(v["tri"], before["node"]))
    for m, M in pose_util.pose_matrices(rt, variant).items():
        assert same(s.mesh_transform(m), M)
    # the pure host function gives the same arrays
    tri, attr, mnt = rt.pose_view(before, s.rest()["rest"], pose_util.pose_matrices(rt, variant))
    assert same(tri, v["tri"]) and same(attr, v["tri_attr"]) and same(mnt, v["mesh_normal_transform"])


def test_posed_lamp_moves_the_lights(rt):
    s = rt.Scene.load(rtref.scene_path("cornell"), 64, 64, 1)
    s.enable_light_updates()
    s.enable_poses()
    before = s.view()
    s.pose({**pose_util.lamp_pose(rt), **pose_util.pose_matrices(rt, "pose_cornell")})
    v = s.view()
    light, lnode = rt.relight_view(v, s.light_map())
    assert same(v["light"], light) and same(v["light_node"], lnode)
    assert not same(v["light"], before["light"]) and not same(v["light_node"], before["light_node"])
    assert same(v["light"][:, 0:12], v["tri"][s.light_map()])
    assert same(v["node"], np_refit(v["tri"], before["node"]))


# ------------------------------------------------------------------------ 4. a fused build is another rule
def fused_dot(m, i, p, w, once):
    """Component i of M (p, w) where every product-and-add is rounded once (an fma in double), exactly:
    per add (rounded to float after each) or the four terms accumulated in double and rounded to float once."""
    terms = [(m[i], p[0]), (m[4 + i], p[1]), (m[8 + i], p[2]), (m[12 + i], w)]
    if once:
        acc = float(Fraction(float(terms[0][0])) * Fraction(float(terms[0][1])))
        for a, b in terms[1:]:
            acc = float(Fraction(float(a)) * Fraction(float(b)) + Fraction(acc))
        return np.float32(acc)
    r = np.float32(0)
    for a, b in terms:
        r = np.float32(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(r))))
    return r


def plain_dot(m, i, p, w, once):
    """The rule itself (rt_pose.h dot_per_add / dot_once) in numpy doubles: every product and add rounded."""
    terms = [(m[i], p[0]), (m[4 + i], p[1]), (m[8 + i], p[2]), (m[12 + i], w)]
    if once:
        acc = np.float64(terms[0][0]) * np.float64(terms[0][1])
        for a, b in terms[1:]:
            acc = acc + np.float64(a) * np.float64(b)
        return np.float32(acc)
    r = np.float32(0)
    for a, b in terms:
        r = np.float32(np.float64(r) + np.float64(a) * np.float64(b))
    return r


def transformed_words(dot, M, NT, q, n):
    """The words of the rule that come straight out of a transform, for unique positions q and normals n:
    M q per add (3), the once-rounded y and z of M q (2), and NT n before it is normalised (3)."""
    out = []
    for p in q:
        out += [dot(M, 0, p, 1.0, False), dot(M, 1, p, 1.0, False), dot(M, 2, p, 1.0, False),
                dot(M, 1, p, 1.0, True), dot(M, 2, p, 1.0, True)]
    for p in n:
        out += [dot(NT, 0, p, 0.0, True), dot(NT, 1, p, 0.0, True), dot(NT, 2, p, 0.0, False)]
    return np.array(out, np.float32)


def test_the_inputs_tell_a_fused_build_from_the_rule(rt, vdir):
    """The blob's pose: the transforms of its vertices restated (a) as the rule says and (b) with every
    product-and-add rounded once, in exact rational arithmetic.  (a) must give the words of the expected
    records, which are the reference's; (b) must not: a build that fuses is caught by these inputs."""
    variant = "pose_cornell_blob"
    ref, path = pose_util.variant_golden(rt, variant, vdir)
    s, before, v = posed(rt, variant)
    (mesh, M), = pose_util.pose_matrices(rt, variant).items()
    NT = v["mesh_normal_transform"][mesh]
    assert same(NT, ref["mesh_normal_transform"][mesh])
    mine = tri_mesh(v) == mesh
    rest = s.rest()["rest"][mine]
    q, qi = np.unique(rest[:, 0:9].reshape(-1, 3), axis=0, return_inverse=True)
    n, ni = np.unique(rest[:, 9:18].reshape(-1, 3), axis=0, return_inverse=True)
    qi, ni = qi.reshape(-1, 3), ni.reshape(-1, 3)
    plain = transformed_words(plain_dot, M, NT, q, n)
    fused = transformed_words(fused_dot, M, NT, q, n)
    place = pose_util.through_source(s.tri_source(), rt.Scene.load(path, 64, 64, 1).tri_source())
    want_v0 = ref["tri"][place][mine][:, 0:3]
    want_nrm = ref["tri_attr"][place][mine][:, 0:9]

    def record_words(words):
        """v0 (M q0 per add) and the three shading normals (normal(NT n), rt_vec.h's order) of every triangle."""
        v0 = words[: 5 * len(q)].reshape(-1, 5)[qi[:, 0], 0:3]
        x, y, z = words[5 * len(q):].reshape(-1, 3).T
        length = np.sqrt(((f32(0) + x * x) + y * y) + z * z)
        inv = f32(1) / length
        nrm = np.stack([x * inv, y * inv, z * inv], 1).astype(f32)[ni].reshape(-1, 9)
        return v0, nrm

    v0, nrm = record_words(plain)
    assert same(v0, want_v0) and same(nrm, want_nrm)   # (a) is the golden, word for word
    v0, nrm = record_words(fused)
    changed = int((bits(v0) != bits(want_v0)).sum() + (bits(nrm) != bits(want_nrm)).sum())
    print(f"fused restatement: {int((bits(plain) != bits(fused)).sum())} of {len(plain)} transformed words differ, "
          f"{changed} words of the expected records")
    assert changed >= 1


# ------------------------------------------------------------------------ 5. from-view scenes
def test_from_view_scenes_need_set_rest(rt):
    loaded = rt.Scene.load(rtref.scene_path("cornell"), 64, 64, 1)
    a = loaded.view()
    s = rt.Scene.from_view(a)
    for call in (s.enable_poses, s.rest, s.tri_source, lambda: s.mesh_transform(0)):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.ERR_STATE
    with pytest.raises(rt.RtError) as e:
        s.pose(pose_util.pose_matrices(rt, "pose_cornell"))
    assert e.value.code == rt.ERR_STATE
    assert all(same(s.view()[k], a[k]) for k in KEYS)
    bad = loaded.rest()
    bad["tri_source"] = bad["tri_source"].copy()
    bad["tri_source"][0] = bad["tri_source"][1]
    with pytest.raises(rt.RtError, match="permutation"):
        s.set_rest(bad)
    s.set_rest(loaded.rest())
    assert all(same(s.rest()[k], loaded.rest()[k]) for k in ("rest", "tri_source", "mesh_matrix"))
    s.enable_poses()
    s.enable_poses()   # idempotent
    poses = pose_util.pose_matrices(rt, "pose_cornell")
    s.pose(poses)
    loaded.enable_poses()
    loaded.pose(poses)
    assert all(same(s.view()[k], loaded.view()[k]) for k in KEYS)
    assert not same(s.view()["tri"], a["tri"])
    with pytest.raises(rt.RtError) as e:
        s.set_rest(loaded.rest())
    assert e.value.code == rt.ERR_STATE


# ------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_scene_as_it_was(rt):
    s = rt.Scene.load(rtref.scene_path("cornell"), 64, 64, 1)
    poses = pose_util.pose_matrices(rt, "pose_cornell")
    (m0, M0), (m1, M1) = list(poses.items())
    lamp = next(iter(pose_util.lamp_pose(rt)))
    lib = rt.lib()
    ids = np.array([m0, m0], np.uint32)
    two = np.concatenate([M0, M1])
    flat = M0.copy()
    flat[0:3] = 0   # a zero column: the determinant is exactly zero
    u, d = rt._c_u, rt._c_d

    def refused(code, n, mesh, mat, match):
        before = s.view()
        rc = lib.rt_scene_pose_meshes(s.handle, n, None if mesh is None else mesh.ctypes.data_as(u),
                                      None if mat is None else mat.ctypes.data_as(d))
        assert rc == code and match in lib.rt_last_error().decode(), lib.rt_last_error()
        after = s.view()
        assert all(same(after[k], before[k]) for k in KEYS)

    refused(rt.ERR_STATE, 1, ids[:1], M0, "not enabled")
    s.enable_poses()
    one = ids[:1]
    refused(rt.ERR_ARG, 0, one, M0, "no mesh named")
    refused(rt.ERR_ARG, 1, None, M0, "NULL")
    refused(rt.ERR_ARG, 1, one, None, "NULL")
    refused(rt.ERR_ARG, 1, np.array([len(s.view()["mesh_f"])], np.uint32), M0, "no mesh")
    refused(rt.ERR_ARG, 2, ids, two, "named twice")
    refused(rt.ERR_ARG, 1, one, flat, "zero determinant")
    refused(rt.ERR_ARG, 2, np.array([m1, m0], np.uint32), np.concatenate([M1, flat]), "zero determinant")
    refused(rt.ERR_ARG, 2, np.array([m0, lamp], np.uint32), two, "emissive")
    with pytest.raises(rt.RtError, match="zero determinant"):
        rt.pose_view(s.view(), s.rest()["rest"], {m0: flat})
    s.pose({m0: M0})   # and the scene still takes a good pose
    assert same(s.mesh_transform(m0), M0)


# ------------------------------------------------------------------------ 7. special values
def special_matrices(rt):
    """(a matrix with one NaN entry, one with an infinite translation): both determinants are not zero
    (they are NaN), so neither is refused."""
    M = pose_util.pose_matrices(rt, "pose_cornell")
    (m0, M0), _ = list(M.items())
    nan, inf = M0.copy(), M0.copy()
    nan[5] = np.nan
    inf[12] = np.inf
    return m0, nan, inf


@pytest.mark.parametrize("which", ["nan", "inf"])
def test_special_values_follow_the_refit_rule(rt, which):
    s = rt.Scene.load(rtref.scene_path("cornell"), 64, 64, 1)
    s.enable_poses()
    before = s.view()
    mesh, nan, inf = special_matrices(rt)
    with np.errstate(all="ignore"):
        s.pose({mesh: nan if which == "nan" else inf})
        v = s.view()
        assert not np.isfinite(v["tri"][tri_mesh(v) == mesh]).all()
        assert same(v["node"], np_refit(v["tri"], before["node"]))
    # a subtree without a posed triangle keeps its boxes
    ab = bits(before["node"])[:, 6:8]
    has = np.zeros(len(ab), bool)
    for i in range(len(ab) - 1, -1, -1):
        a, b = int(ab[i, 0]), int(ab[i, 1])
        has[i] = (tri_mesh(v)[a:a + (b >> 2)] == mesh).any() if b & 3 == 3 else has[a] or has[a + 1]
    assert (~has).any() and has.any()
    assert same(v["node"][~has], before["node"][~has])
    assert not np.isnan(v["node"][:, 0:6]).any()
