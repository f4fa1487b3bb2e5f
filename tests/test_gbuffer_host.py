"""The first-hit feature record without a GPU: raytracing-hw_amd/csrc/rt_gbuffer.h compiled for the
host (tests/native/gbuffer_host.cpp) on the reference's own flattened scenes.  The hit, its
distance and its triangle are checked against the CPU oracle (the independent restatement the
reference's goldens pin) on the very rays the twin cast; the attributes against the scene arrays."""
import numpy as np
import pytest

import rtref
from denoise_util import FIXTURES, arrays_of, f32, host_gbuffer, twin

bits = rtref.bits


@pytest.fixture(scope="module")
def gh(tmp_path_factory):
    return twin(tmp_path_factory)


def fields(rec):
    ids = rec.view(np.int32)
    return dict(N=rec[:, 0:3], t=rec[:, 3], albedo=rec[:, 4:7], prim=ids[:, 7], E=rec[:, 8:11], mesh=ids[:, 11], P=rec[:, 12:15],
                pad=ids[:, 15])


@pytest.mark.parametrize("name,w,h", FIXTURES)
def test_hits_match_the_oracle(rt, oracle, gh, name, w, h):
    a = arrays_of(rt, name, w, h)
    rec, org, dirs = host_gbuffer(rt, gh, name, w, h)
    g = fields(rec)
    out_f, out_i = oracle.rays(a, org, dirs)
    hit = out_i[:, 0].astype(bool) & (out_f[:, 0] < f32(a["max_distance"]))
    assert hit.any()
    assert np.array_equal(g["prim"] >= 0, hit)
    assert np.array_equal(g["prim"][hit], out_i[hit, 1])
    assert np.array_equal(bits(g["t"][hit]), bits(out_f[hit, 0]))
    # a miss is all-zero words with both ids -1
    miss_words = rec[~hit].view(np.uint32).copy()
    assert (miss_words[:, [7, 11]] == 0xFFFFFFFF).all()
    miss_words[:, [7, 11]] = 0
    assert not miss_words.any()
    assert (g["pad"] == 0).all()
    assert np.array_equal(g["mesh"][hit], a["tri_attr"][g["prim"][hit], 15].view(np.int32))
    if name == "texedge":   # the fixture's zfar clips: hits beyond it are misses here
        assert (out_i[:, 0].astype(bool) & ~hit).any()


@pytest.mark.parametrize("name,w,h", FIXTURES)
def test_position_is_origin_plus_direction_times_t(rt, gh, name, w, h):
    rec, org, dirs = host_gbuffer(rt, gh, name, w, h)
    g = fields(rec)
    hit = g["prim"] >= 0
    m = np.zeros(len(dirs), f32)   # Ray::Ray normalises: length by three accumulating adds, then * (1 / length)
    for c in range(3):
        m = m + dirs[:, c] * dirs[:, c]
    inv = f32(1) / np.sqrt(m)
    d = dirs * inv[:, None]
    want = org + d * g["t"][:, None]
    assert want.dtype == f32
    assert np.array_equal(bits(g["P"][hit]), bits(want[hit]))


@pytest.mark.parametrize("name,w,h", FIXTURES)
def test_albedo_and_emission(rt, gh, name, w, h):
    a = arrays_of(rt, name, w, h)
    g = fields(host_gbuffer(rt, gh, name, w, h)[0])
    hit = g["prim"] >= 0
    mesh = g["mesh"]
    base, emis, tex = a["mesh_f"][:, 0:3], a["mesh_f"][:, 3:6], a["mesh_tex"]
    plain = hit & (tex[np.maximum(mesh, 0), 0] < 0)
    assert np.array_equal(bits(g["albedo"][plain]), bits(base[mesh[plain]]))
    no_etex = hit & (tex[np.maximum(mesh, 0), 3] < 0)
    assert np.array_equal(bits(g["E"][no_etex]), bits(emis[mesh[no_etex]]))
    textured = hit & ~plain
    if name in ("texedge", "sponza_mini"):
        assert textured.sum() >= 50
        al, factor = g["albedo"][textured], base[mesh[textured]]
        assert (al >= 0).all() and (al <= factor).all()   # an sRGB sample is in [0, 1]
        # Every textured mesh seen by two pixels or more shows more than one albedo.  (Exempt by
        # construction: a mesh whose hit triangles share one texture coordinate, texedge's
        # constant-UV quads, and a texture of one colour.  The fixtures are fixed data, so "two
        # pixels fetch different values" is a fact of them, not a chance.)
        texels, info = a["texels"].reshape(-1, 4), a["tex_info"]
        checked = 0
        for m in np.unique(mesh[textured]):
            here = textured & (mesh == m)
            off, tw, th = (int(v) for v in info[tex[m, 0]][:3])
            uv = a["tri_attr"][np.unique(g["prim"][here]), 9:15].reshape(-1, 2)
            if here.sum() < 2 or len(np.unique(bits(uv), axis=0)) < 2 or len(np.unique(texels[off:off + tw * th, :3], axis=0)) < 2:
                continue
            checked += 1
            assert len(np.unique(bits(g["albedo"][here]), axis=0)) > 1, f"mesh {m}: one albedo over {here.sum()} pixels"
        assert checked >= (4 if name == "texedge" else 20)
    else:
        assert not textured.any()


def test_cornell_normals_are_the_faces(rt, gh):
    """Cornell's faces are flat, so the shading normal is the geometric one up to the sign (the
    vertex normals' own, flipped where the ray is inside) and to the few ulp that normalising a unit
    vector costs in f32."""
    name, w, h = FIXTURES[0]
    a = arrays_of(rt, name, w, h)
    rec, org, dirs = host_gbuffer(rt, gh, name, w, h)
    g = fields(rec)
    hit = g["prim"] >= 0
    ngeo = a["tri"][g["prim"][hit], 9:12].astype(np.float64)
    N = g["N"][hit].astype(np.float64)
    assert (np.abs((N * ngeo).sum(-1)) >= 1 - 1e-6).all()


@pytest.mark.parametrize("name,w,h", FIXTURES[1:])
def test_normals_are_unit(rt, gh, name, w, h):
    g = fields(host_gbuffer(rt, gh, name, w, h)[0])
    hit = g["prim"] >= 0
    length = np.linalg.norm(g["N"][hit].astype(np.float64), axis=-1)
    assert np.abs(length - 1).max() <= 1e-6


def test_shards_are_rows_of_the_frame(rt, gh):
    """A (rank, world, row_block) shard's records are the frame's, at the rows it owns."""
    for name, w, h, rank, world, rb in [("sponza_mini", 64, 36, 0, 3, 8), ("sponza_mini", 64, 36, 1, 3, 8),
                                        ("sponza_mini", 64, 36, 2, 3, 8), ("sponza_mini", 64, 36, 1, 5, 1),
                                        ("cornell", 33, 17, 4, 5, 1)]:
        full = host_gbuffer(rt, gh, name, w, h)[0].reshape(h, w, 16)
        rows = rt.shard_rows(h, rank, world, rb)
        part = host_gbuffer(rt, gh, name, w, h, rank, world, rb)[0].reshape(len(rows), w, 16)
        assert np.array_equal(part.view(np.uint32), full[rows].view(np.uint32))
