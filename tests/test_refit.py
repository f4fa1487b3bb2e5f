"""Movable geometry without a GPU (include/rt_hw.h rt_scene_update_tris, rt_refit_view; the rule is
raytracing-hw_amd/csrc/rt_refit.h): the host refit against the reference's own boxes and against a
numpy restatement of the rule, +-0 / NaN / infinite records, ranges, refusals, the host-only plan,
the CPU oracle on an updated scene, and the CLI's RT_MOVES usage errors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtref
from refit_util import (DUMPS, bits, box_mesh, changed_runs, emissive_meshes, f32, np_refit, same_view,
                        special_records, translated, tri_mesh, twin_arrays, word)

ERR_ARG = -1
W, H, S = 33, 17, 3
_c_f = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def cornell(rt):
    return rtref.ref_arrays(rt, "cornell", W, H, S)


def fptr(a):
    return a.ctypes.data_as(_c_f)


# ------------------------------------------------------------------------ 1. the reference's boxes
@pytest.mark.parametrize("name", DUMPS)
def test_refit_view_gives_the_reference_boxes(rt, name):
    """rt_refit_view on the reference's own triangles and topology gives the dump's node_aabb, every
    bit, and copies a and b; the numpy restatement gives the same (so the two agree with each other)."""
    a = rtref.ref_arrays(rt, name, W, H, S)
    got = rt.refit_view(a)
    assert got.shape == a["node"].shape
    assert np.array_equal(bits(got), bits(a["node"]))
    assert np.array_equal(bits(np_refit(a["tri"], a["node"])), bits(a["node"]))
    # boxes wiped first: nothing of the input's boxes is read
    wiped = dict(a)
    wiped["node"] = a["node"].copy()
    wiped["node"][:, 0:6] = np.nan
    assert np.array_equal(bits(rt.refit_view(wiped)), bits(a["node"]))


# ------------------------------------------------------------------------ 2. special values
def test_special_values_keep_the_first_attaining_bits(rt, cornell):
    tri, expect = special_records(cornell)
    want = twin_arrays(cornell, tri)
    wb = bits(want["node"])
    for node, k, pattern in expect:   # the restatement itself shows every case
        assert wb[node, k] == pattern, (node, k, hex(wb[node, k]), hex(pattern))
    assert {word(0.0), word(-0.0)} <= {p for _, _, p in expect}
    s = rt.Scene.from_view(cornell)
    for first, count in changed_runs(cornell["tri"], tri):
        s.update_triangles(first, tri[first:first + count])
    v = s.view()
    assert np.array_equal(bits(v["tri"]), bits(tri))
    assert np.array_equal(bits(v["node"]), wb)
    assert np.array_equal(bits(rt.refit_view(want)), wb)
    assert same_view(rt.Scene.from_view(want).view(), v)


# ------------------------------------------------------------------------ 3. ranges
def test_ranges(rt, cornell):
    em = emissive_meshes(cornell)
    mesh = tri_mesh(cornell)
    n = len(cornell["tri"])
    movable = np.flatnonzero(~em[mesh])
    rng = np.random.default_rng(7)
    s = rt.Scene.from_view(cornell)
    cur = {k: cornell[k].copy() for k in ("tri", "tri_attr", "tri_tan")}

    def check():
        v = s.view()
        want = twin_arrays(cornell, cur["tri"], cur["tri_attr"], cur["tri_tan"])
        assert same_view(v, want)

    # first odd, count 1
    k = int(next(i for i in movable if i % 2 == 1))
    cur["tri"][k, 0:9] += rng.random(9, dtype=f32)
    s.update_triangles(k, cur["tri"][k:k + 1])
    check()
    # the last triangle (cornell's is not emissive)
    assert not em[mesh[n - 1]]
    cur["tri"][n - 1, 0:3] -= f32(0.25)
    s.update_triangles(n - 1, cur["tri"][n - 1:])
    check()
    # two successive updates of overlapping runs; attr and tan given, then NULL keeps them
    run = movable[:4]
    assert np.array_equal(run, np.arange(run[0], run[0] + 4))
    a0 = int(run[0])
    new_attr = cur["tri_attr"][a0:a0 + 4].copy()
    new_attr[:, 0:15] = rng.random((4, 15), dtype=f32)
    new_attr[:, 15] = np.array([12345], np.int32).view(f32)[0]          # the caller's mesh id word: ignored
    new_tan = rng.random((4, 12), dtype=f32)
    cur["tri"][a0:a0 + 4, 0:9] *= f32(1.5)
    cur["tri_attr"][a0:a0 + 4, 0:15] = new_attr[:, 0:15]
    cur["tri_tan"][a0:a0 + 4] = new_tan
    s.update_triangles(a0, cur["tri"][a0:a0 + 4], attr=new_attr, tan=new_tan)
    check()
    assert np.array_equal(tri_mesh(s.view()), mesh)
    cur["tri"][a0 + 1:a0 + 3, 0:3] += f32(0.125)
    s.update_triangles(a0 + 1, cur["tri"][a0 + 1:a0 + 3])                # attr / tan NULL: kept
    check()
    # count == 0: RT_OK, nothing happens (also at first == n_tris)
    before = s.view()
    lib = rt.lib()
    assert lib.rt_scene_update_tris(s.handle, 3, 0, fptr(cur["tri"]), None, None) == 0
    assert lib.rt_scene_update_tris(s.handle, n, 0, fptr(cur["tri"]), None, None) == 0
    assert same_view(s.view(), before)


def test_whole_scene_update_of_a_scene_without_lights(rt):
    """The whole range in one call (every mesh of geoedge that is emissive is skipped by using a scene
    whose emission is zeroed: the light list is not part of the refit)."""
    a = rtref.ref_arrays(rt, "geoedge", W, H, S)
    a = dict(a)
    a["mesh_f"] = a["mesh_f"].copy()
    a["mesh_f"][:, 3:6] = 0
    s = rt.Scene.from_view(a)
    tri = a["tri"].copy()
    tri[:, 0:3] = (tri[:, 0:3] + f32(0.5)).astype(f32)
    s.update_triangles(0, tri)
    assert same_view(s.view(), twin_arrays(a, tri))
    s.update_triangles(0, a["tri"])                                      # and back: the reference's boxes again
    assert np.array_equal(bits(s.view()["node"]), bits(a["node"]))


# ------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_view_as_it_was(rt, cornell):
    lib = rt.lib()
    s = rt.Scene.from_view(cornell)
    n = len(cornell["tri"])
    em = emissive_meshes(cornell)
    mesh = tri_mesh(cornell)
    lit = int(np.flatnonzero(em[mesh])[0])
    tri = (cornell["tri"] + f32(1)).astype(f32)
    before = s.view()

    def refused(rc, *words):
        msg = lib.rt_last_error().decode()
        assert rc == ERR_ARG and all(w in msg for w in words), (rc, msg)
        assert same_view(s.view(), before)

    refused(lib.rt_scene_update_tris(s.handle, 0, 1, None, None, None), "NULL tri")
    refused(lib.rt_scene_update_tris(None, 0, 1, fptr(tri), None, None), "NULL scene")
    refused(lib.rt_scene_update_tris(s.handle, n, 1, fptr(tri), None, None), "beyond")
    refused(lib.rt_scene_update_tris(s.handle, n - 1, 2, fptr(tri), None, None), "beyond")
    refused(lib.rt_scene_update_tris(s.handle, 0xFFFFFFFF, 2, fptr(tri), None, None), "beyond")
    refused(lib.rt_scene_update_tris(s.handle, lit, 1, fptr(tri), None, None), "moving lights are not supported", "emissive")
    refused(lib.rt_scene_update_tris(s.handle, 0, n, fptr(tri), None, None), "moving lights are not supported")
    # the device entry: the same refusals, and a scene that is on no device
    V = ctypes.c_void_p
    fake = V(4096)   # (never dereferenced: every refusal comes before any launch or copy)
    refused(lib.rt_scene_update_tris_device(s.handle, 0, 0, 1, None, None, None, None), "NULL tri")
    refused(lib.rt_scene_update_tris_device(s.handle, 0, n, 1, fake, None, None, None), "beyond")
    refused(lib.rt_scene_update_tris_device(s.handle, 0, lit, 1, fake, None, None, None), "moving lights are not supported")
    refused(lib.rt_scene_update_tris_device(s.handle, 0, 0, 1, fake, None, None, None), "not uploaded to device 0")
    refused(lib.rt_scene_update_tris_device(s.handle, -1, 0, 1, fake, None, None, None), "not uploaded")
    refused(lib.rt_scene_read_device(s.handle, 0, None, None, None, None), "not uploaded")
    assert lib.rt_refit_view(None, None) == ERR_ARG
    with pytest.raises(ValueError, match="emissive"):
        s.translated_records(int(mesh[lit]), (1, 0, 0))
    with pytest.raises(ValueError, match="no mesh"):
        s.translated_records(len(em), (1, 0, 0))


def test_translated_records_move_a_mesh(rt, cornell):
    s = rt.Scene.from_view(cornell)
    m = box_mesh(cornell)
    off = (0.1, 0, 0.05)
    runs = s.translated_records(m, off)
    assert sum(len(t) for _, t in runs) == 12
    for first, tri in runs:
        s.update_triangles(first, tri)
    want = twin_arrays(cornell, translated(cornell, m, off))
    assert same_view(s.view(), want)
    assert not np.array_equal(bits(want["node"]), bits(cornell["node"]))
    # cover=True: the covering range cut at emissive triangles; the same scene in no more calls, and on
    # a mesh whose triangles lie scattered (cornell_blob's blob against its walls) in far fewer
    s2 = rt.Scene.from_view(cornell)
    covered = s2.translated_records(m, off, cover=True)
    assert len(covered) <= len(runs)
    for first, tri in covered:
        s2.update_triangles(first, tri)
    assert same_view(s2.view(), want)
    blob = rtref.ref_arrays(rt, "cornell_blob", W, H, S)
    sb = rt.Scene.from_view(blob)
    counts = np.bincount(tri_mesh(blob))
    big = int(np.argmax(counts * ~emissive_meshes(blob)))
    few, many = sb.translated_records(big, off, cover=True), sb.translated_records(big, off)
    assert len(few) <= len(many) and len(few) <= 1 + int(emissive_meshes(blob)[tri_mesh(blob)].sum())
    for first, tri in few:
        sb.update_triangles(first, tri)
    assert same_view(sb.view(), twin_arrays(blob, translated(blob, big, off)))


# ------------------------------------------------------------------------ 5. the plan
@pytest.fixture(scope="module")
def rp(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rp") / "librp.so")
    src = os.path.join(rtref.ROOT, "tests", "native", "refit_plan_host.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-shared", "-fPIC", src, "-o", out], check=True)
    return ctypes.CDLL(out)


def test_plan_levels_and_id_maps(rt, rp):
    a = rtref.ref_arrays(rt, "cornell_blob", W, H, S)
    node = np.ascontiguousarray(a["node"], f32)
    mf = np.ascontiguousarray(a["mesh_f"], f32)
    n, nm = len(node), len(mf)
    b_of, of_b, lf = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint32)
    em, bfs, nl = np.zeros(nm, np.uint8), np.zeros((n, 8), f32), ctypes.c_uint32(0)
    V = ctypes.c_void_p
    rc = rp.rp_plan(V(node.ctypes.data), n, V(mf.ctypes.data), nm, V(b_of.ctypes.data), V(of_b.ctypes.data), V(lf.ctypes.data),
                    ctypes.byref(nl), V(em.ctypes.data), V(bfs.ctypes.data))
    assert rc == 0
    L = int(nl.value)
    lf = lf[:L + 1].astype(np.int64)
    # the level ranges partition [0, n)
    assert lf[0] == 0 and lf[-1] == n and np.all(np.diff(lf) > 0) and L == a["bvh_depth"] + 1
    # the id maps are inverse to each other
    assert np.array_equal(of_b[b_of], np.arange(n)) and np.array_equal(b_of[of_b], np.arange(n)) and b_of[0] == 0
    # every child lies in the level after its parent's; siblings are adjacent with the left one odd
    level = np.searchsorted(lf, np.arange(n), side="right") - 1
    ab = bits(bfs)[:, 6:8]
    inner = np.flatnonzero(ab[:, 1] & 3 != 3)
    kids = ab[inner, 0].astype(np.int64)
    assert np.all(level[kids] == level[inner] + 1) and np.all(level[kids + 1] == level[inner] + 1)
    assert np.all(kids % 2 == 1) and np.all(kids > inner)
    # the renumbered records are the build-order ones, child ids mapped
    src = bits(node)
    assert np.array_equal(bits(bfs)[:, 0:6], src[b_of][:, 0:6]) and np.array_equal(ab[:, 1], src[b_of][:, 7])
    assert np.array_equal(b_of[kids], src[b_of[inner], 6])
    leaf = np.flatnonzero(ab[:, 1] & 3 == 3)
    assert np.array_equal(ab[leaf, 0], src[b_of[leaf], 6])
    assert np.array_equal(em.astype(bool), emissive_meshes(a))


# ------------------------------------------------------------------------ 6. the oracle on an updated scene
def test_oracle_rays_on_the_updated_view(rt, oracle, cornell):
    a = dict(cornell, width=24, height=16)
    s = rt.Scene.from_view(a)
    m = box_mesh(a)
    for first, tri in s.translated_records(m, (0.1, 0, 0.05)):
        s.update_triangles(first, tri)
    twin = rt.Scene.from_view(twin_arrays(a, translated(a, m, (0.1, 0, 0.05))))
    org, dirs = rtref.pixel_centre_rays(a)
    f1, i1 = oracle.rays(s.view(), org, dirs)
    f2, i2 = oracle.rays(twin.view(), org, dirs)
    assert rtref.same(f1, f2).all() and np.array_equal(i1, i2)
    f0, i0 = oracle.rays(a, org, dirs)
    assert not np.array_equal(i0[:, 1], i1[:, 1]) or not rtref.same(f0, f1).all()   # the move is visible


# ------------------------------------------------------------------------ 7. CLI usage errors
def test_cli_moves_usage_errors(rt, tmp_path, cornell):
    """Reported before anything is rendered (no GPU is touched)."""
    exe = os.path.join(rtref.ROOT, "raytracing-hw_amd", "rt_solution")
    em = emissive_meshes(cornell)
    lit, free = int(np.flatnonzero(em)[0]), int(np.flatnonzero(~em)[0])

    def run(**env_more):
        env = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}
        r = subprocess.run([exe, rtref.scene_path("cornell"), "8", "8", "1", str(tmp_path / "o.ppm")], env=dict(env, **env_more),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and not list(tmp_path.glob("o*.ppm")), r.stderr
        return r.stderr

    def moves(text):
        (tmp_path / "moves.txt").write_text(text)
        return str(tmp_path / "moves.txt")

    good = f"{free} 0.1 0 0.05"
    for other in ({"RT_PASS_SPP": "2"}, {"RT_ADAPT": "0.1"}, {"RT_CHECKPOINT": str(tmp_path / "ck")}):
        assert "RT_MOVES excludes" in run(RT_MOVES=moves(good + "\n"), **other)
    assert "cannot read" in run(RT_MOVES=str(tmp_path / "nope.txt"))
    assert "no frame" in run(RT_MOVES=moves("# nothing\n\n"))
    for bad in (f"{free} 0.1 0", good + " 3", f"{free} 0.1 x 0", f"{free} 0.1 nan 0", f"{free}.5 0 0 0", "one 0 0 0"):
        assert "line 3: expected groups of four numbers" in run(RT_MOVES=moves("# a comment\n" + good + "\n" + bad + "\n")), bad
    assert f"line 2: mesh {lit} is emissive" in run(RT_MOVES=moves(good + "\n" + good + f" {lit} 0 1 0\n"))
    assert f"line 1: unknown mesh {len(em)}" in run(RT_MOVES=moves(f"{len(em)} 0 0 0\n"))
    assert "line 1: unknown mesh -1" in run(RT_MOVES=moves("-1 0 0 0\n"))
    cams = tmp_path / "cams.txt"
    cams.write_text("0 0 6  1 0 0  0 1 0  0 0 -1  0.5 0.5\n")
    assert "line counts must be equal" in run(RT_MOVES=moves(good + "\n" + good + "\n"), RT_CAMERAS=str(cams))
