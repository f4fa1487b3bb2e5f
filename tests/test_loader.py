"""Host scene path: glTF loader, BVH build, light list, textures — against the reference's own
parsed and BVH-built scene (tests/golden/*_dump.rtd, written by oracle/ref_harness `dump`, i.e.
the reference's sources compiled as its CMake build compiles them: GCC 11, -O3).

Every fixture is bit-exact (triangles, attributes, tangents, BVH nodes, light BVH, materials,
normal transforms, decoded texels), rotated meshes included: the loader reproduces the
roundings of the shipped binary's SLP-vectorized transform loop (rt_host.cpp
m4_mul_vector_gcc), which differ from the source's in a few ulp.  test_slp_evidence shows the
difference is the compiler's: the same sources built with -fno-tree-slp-vectorize give other
arrays, which this loader does not match.
"""
import numpy as np
import pytest

import rtref

EXACT = ["cornell", "sponza_mini", "cornell_blob", "practice6_1", "texedge", "geoedge"]
ROTATED = ["cornell_blob", "practice6_1"]
KEYS = ["tri", "tri_attr", "tri_tan", "node", "light", "light_node", "mesh_f", "mesh_tex", "mesh_normal_transform"]


def _mine(rt, name):
    return rt.Scene.load(rtref.scene_path(name), 64, 64, 1).view()


@pytest.mark.parametrize("name", EXACT)
def test_loader_bit_exact(rt, name):
    mine = _mine(rt, name)
    ref = rtref.ref_arrays(rt, name, 64, 64, 1)
    for k in KEYS:
        a, b = np.ascontiguousarray(mine[k]), np.ascontiguousarray(ref[k])
        assert a.shape == b.shape, k
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
    d = rtref.golden(f"{name}_dump.rtd")
    assert int(mine["ray_depth"]) == int(d["ray_depth"][0])


@pytest.mark.parametrize("name", EXACT)
def test_camera_matches_reference(rt, name):
    mine = _mine(rt, name)
    cam = rtref.golden(f"{name}_dump.rtd")["camera"]
    assert np.array_equal(rtref.bits(mine["cam_pos"]), rtref.bits(cam[:3]))
    assert np.array_equal(rtref.bits(np.asarray(mine["cam_axes"]).reshape(-1)), rtref.bits(cam[3:12]))
    assert np.array_equal(rtref.bits(mine["cam_fov"]), rtref.bits(cam[12:14]))


@pytest.mark.parametrize("name", ROTATED)
def test_slp_evidence(rt, tmp_path, name):
    """The reference's scene_parser.cpp built without GCC's SLP vectorizer (oracle/Makefile
    ref_harness_noslp; needs the reference build, i.e. this container) yields different vertex
    arrays for the rotated meshes, and this loader matches the shipped -O3 build instead."""
    import os
    import subprocess
    exe = os.path.join(rtref.ROOT, "oracle", "_ref", "ref_harness_noslp")
    if not os.path.exists(exe):
        pytest.skip("reference build absent (oracle/_ref is built only where /root/reference exists)")
    out = str(tmp_path / "noslp.rtd")
    subprocess.run([exe, "dump", rtref.scene_path(name), "64", "64", out], check=True, capture_output=True)
    noslp = rtref.ref_arrays(rt, name, 64, 64, 1, dump=rtref.rtdump.load(out))
    slp = rtref.ref_arrays(rt, name, 64, 64, 1)
    mine = _mine(rt, name)
    def raw(a):
        return np.ascontiguousarray(a).view(np.uint8)
    assert not np.array_equal(raw(noslp["tri"]), raw(slp["tri"]))      # the two builds disagree
    assert np.array_equal(raw(mine["tri"]), raw(slp["tri"]))            # this loader = the shipped build
    assert np.array_equal(raw(mine["node"]), raw(slp["node"]))


def test_texels_match_reference(rt):
    """Decoded texels of every texture, by FNV-1a hash: sponza_mini's 69 16x16 images and
    texedge's eight odd sizes (1x1 to 13x6)."""
    for name in ("sponza_mini", "texedge"):
        mine = _mine(rt, name)
        d = rtref.golden(f"{name}_dump.rtd")
        info = np.asarray(mine["tex_info"])
        tex = np.asarray(mine["texels"])
        assert len(info) == len(d["tex_fnv1a"])
        for (off, w, h, ch), (rw, rh, rch), want in zip(info, d["tex_dim"], d["tex_fnv1a"]):
            assert (w, h) == (rw, rh)
            # texels are stored RGBA8 from texel `off`; the reference keeps `channels` bytes per texel
            px = tex[4 * int(off):4 * (int(off) + int(w) * int(h))].reshape(-1, 4)[:, :int(rch)]
            hsh = 1469598103934665603
            for byte in px.reshape(-1).tobytes():
                hsh = ((hsh ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
            assert hsh == int(want), name


def test_texedge_fixture_covers_its_edges(rt):
    """The texedge fixture as the reference parsed it: the eight texture sizes (none a
    multiple of 4 on both sides), every one of the four material slots in use, UVs over about
    [-3, 4], the four constant-UV quads, and a zfar inside the room."""
    sc = rtref.scenes_module()
    d = rtref.golden("texedge_dump.rtd")
    assert [(int(w), int(h)) for w, h, _ in d["tex_dim"]] == [(w, h) for w, h, _ in sc.TEXEDGE_TEXTURES]
    assert (d["mesh_tex"] >= 0).any(0).all()
    used = set(int(t) for t in d["mesh_tex"].reshape(-1) if t >= 0)
    assert used == set(range(len(sc.TEXEDGE_TEXTURES)))
    uv = d["obj_texcoord"].reshape(-1, 2)
    assert uv.min() <= -2.9 and uv.max() >= 3.9
    const = set()
    for t in d["obj_texcoord"]:
        if (t == t[0]).all():
            const.add((float(t[0, 0]), float(t[0, 1])))
    assert const == {(float(np.float32(u)), float(np.float32(v))) for u, v in sc.TEXEDGE_CONST_UVS}
    assert np.any(d["obj_tangent"])
    assert float(_mine(rt, "texedge")["max_distance"]) == float(np.float32(sc.TEXEDGE_ZFAR))


def test_scene_generator_deterministic(tmp_path):
    sc = rtref.scenes_module()
    a = sc.SCENES["cornell_blob"](str(tmp_path / "a"))
    b = sc.SCENES["cornell_blob"](str(tmp_path / "b"))
    import filecmp
    import os
    for f in sorted(os.listdir(os.path.dirname(a))):
        assert filecmp.cmp(os.path.join(os.path.dirname(a), f), os.path.join(os.path.dirname(b), f), shallow=False), f
    # the committed texedge fixture is what the generator writes
    c = os.path.dirname(sc.SCENES["texedge"](str(tmp_path / "c")))
    committed = os.path.dirname(rtref.scene_path("texedge"))
    assert sorted(os.listdir(c)) == sorted(os.listdir(committed))
    for f in sorted(os.listdir(c)):
        assert filecmp.cmp(os.path.join(c, f), os.path.join(committed, f), shallow=False), f


def test_loader_errors(rt, tmp_path):
    with pytest.raises(rt.RtError):
        rt.Scene.load(str(tmp_path / "missing.gltf"), 8, 8, 1)
    bad = tmp_path / "bad.gltf"
    bad.write_text("{ not json")
    with pytest.raises(rt.RtError):
        rt.Scene.load(str(bad), 8, 8, 1)


@pytest.mark.slow
@pytest.mark.parametrize("scene", ["sponza", "sponza_dragon"])
def test_large_scenes_match_reference(rt, scene):
    """The full-size BASELINE scenes (sponza proxy, 262 k triangles; dragon-100k + sponza,
    362 k): the generator writes the same files the goldens were made from (sha256), and
    this loader's arrays equal the reference's post-BVH arrays (sha256 of each array,
    recorded by tools/make_goldens.py from the reference's own dump)."""
    import hashlib
    import json
    import os
    import tempfile
    meta = json.load(open(os.path.join(rtref.GOLD, "golden_meta.json")))["configs"][scene]
    d = os.path.join(tempfile.gettempdir(), "rt_scenes")
    path = rtref.scenes_module().ensure_scene(scene, d)
    assert rtref.scene_sha256(d, scene) == meta["scene_sha256"]
    mine = rt.Scene.load(path, 64, 64, 1).view()
    got = {k: hashlib.sha256(np.ascontiguousarray(mine[k]).tobytes()).hexdigest() for k in meta["ref_layout_sha256"]}
    assert got == meta["ref_layout_sha256"]


def test_loader_rejects_malformed_buffers(rt, tmp_path):
    """A truncated .bin, an accessor running past its buffer, or a vertex index beyond an
    attribute accessor is RT_ERR_FORMAT (never a read past the end of a buffer)."""
    import json
    import os
    import shutil
    src = os.path.dirname(rtref.scene_path("cornell"))
    doc = json.load(open(rtref.scene_path("cornell")))
    binname = doc["buffers"][0]["uri"]

    def variant(tag, mutate_doc=None, truncate=None):
        d = tmp_path / tag
        shutil.copytree(src, d)
        g = json.loads(json.dumps(doc))
        if mutate_doc:
            mutate_doc(g)
        (d / "cornell.gltf").write_text(json.dumps(g))
        if truncate is not None:
            data = (d / binname).read_bytes()
            (d / binname).write_bytes(data[:truncate(len(data))])
        return str(d / "cornell.gltf")

    prim = doc["meshes"][0]["primitives"][0]
    pos_acc = prim["attributes"]["POSITION"]

    def shrink_positions(g):
        g["accessors"][pos_acc]["count"] = 2

    def huge_count(g):
        g["accessors"][prim["indices"]]["count"] = 10 ** 9

    for path in (variant("trunc", truncate=lambda n: n // 2), variant("count", huge_count),
                 variant("index", shrink_positions)):
        with pytest.raises(rt.RtError):
            rt.Scene.load(path, 8, 8, 1)
    rt.Scene.load(variant("ok"), 8, 8, 1)   # the unmodified copy still loads
