"""Movable lights without a GPU (include/rt_hw.h rt_scene_enable_light_updates, rt_scene_light_map,
rt_relight_view, rt_scene_update_tris on an opted-in scene; the rule is
raytracing-hw_amd/csrc/rt_relight.h): the restated light records and light boxes against the
reference's own and against a numpy restatement, the map, an opt-in that fails cleanly, the host
entry on practice6_1's 1,152 lights, +-0 / NaN / infinite records in the light tree, the refusals
of a scene that has not opted in, the CPU oracle on a moved light, and the CLI's RT_MOVE_LIGHTS."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtref
from refit_util import DUMPS, bits, changed_runs, emissive_meshes, f32, same_view, tri_mesh, word
from relight_util import (light_mesh, np_light_map, np_relight, same_lights, special_light_records, translated_mesh,
                          twin_arrays_lit, wiped)

ERR_ARG = -1
W, H, S = 33, 17, 3
_c_f = ctypes.POINTER(ctypes.c_float)
LIT_KEYS = ("tri", "tri_attr", "tri_tan", "node", "light", "light_node", "mesh_f")


@pytest.fixture(scope="module")
def cornell(rt):
    return rtref.ref_arrays(rt, "cornell", W, H, S)


@pytest.fixture(scope="module")
def practice(rt):
    return rtref.ref_arrays(rt, "practice6_1", 24, 16, 2)


def fptr(a):
    return a.ctypes.data_as(_c_f)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------ 1. the reference's records
@pytest.mark.parametrize("name", DUMPS)
def test_relight_view_gives_the_reference_lights(rt, name):
    """From light words 0..12 and every light box wiped to NaN, rt_relight_view gives the dump's light
    and light_node in every bit (geoedge's three NaN areas included: host against host), and so does
    the numpy restatement; the scene's map is the restated one, a bijection onto the emissive triangles."""
    a = rtref.ref_arrays(rt, name, W, H, S)
    want_map = np_light_map(a)
    lit = np.flatnonzero(emissive_meshes(a)[tri_mesh(a)])
    assert len(a["light"]) > 0 and np.array_equal(np.sort(want_map), lit)
    s = rt.Scene.from_view(a)
    with pytest.raises(rt.RtError, match="has not enabled light updates"):
        s.light_map()
    s.enable_light_updates()
    s.enable_light_updates()   # idempotent
    assert np.array_equal(s.light_map(), want_map)
    assert np.array_equal(rt.Scene.load(rtref.scene_path(name), W, H, S).view()["light"].shape, a["light"].shape)
    light, lnode = rt.relight_view(wiped(a), want_map)
    assert same_bits(light, a["light"]) and same_bits(lnode, a["light_node"])
    nl, nn = np_relight(wiped(a), a["tri"], want_map)
    assert same_bits(nl, a["light"]) and same_bits(nn, a["light_node"])
    assert same_view(s.view(), a)   # the opt-in changed nothing


def test_loaded_scene_opts_in(rt):
    """A scene built by the loader follows the same map rule as one from a view."""
    s = rt.Scene.load(rtref.scene_path("practice6_1"), 24, 16, 2)
    s.enable_light_updates()
    assert np.array_equal(s.light_map(), np_light_map(s.view()))


# ------------------------------------------------------------------------ 2. the opt-in fails cleanly
def test_opt_in_fails_cleanly(rt, cornell):
    lib = rt.lib()
    em, mesh = emissive_meshes(cornell), tri_mesh(cornell)
    lit = int(np.flatnonzero(em[mesh])[0])
    tri = (cornell["tri"] + f32(1)).astype(f32)
    # A: one bit flipped in one light's word 3
    a = dict(cornell, light=cornell["light"].copy())
    a["light"].view(np.uint32)[1, 3] ^= 1
    # B: one more emissive mesh and no light for its triangles
    b = dict(cornell, mesh_f=cornell["mesh_f"].copy())
    extra = int(np.flatnonzero(~em)[0])
    b["mesh_f"][extra, 3] = 1
    first_unlit = int(np.flatnonzero(mesh == extra)[0])
    for arrays, names in ((a, "light 1"), (b, f"triangle {first_unlit}")):
        s = rt.Scene.from_view(arrays)
        before = s.view()
        assert lib.rt_scene_enable_light_updates(s.handle) == ERR_ARG
        assert names in lib.rt_last_error().decode(), lib.rt_last_error()
        with pytest.raises(ValueError, match=names):
            np_light_map(arrays)
        assert same_view(s.view(), before)
        assert lib.rt_scene_light_map(s.handle, np.zeros(8, np.uint32).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == ERR_ARG
        assert lib.rt_scene_update_tris(s.handle, lit, 1, fptr(tri), None, None) == ERR_ARG
        assert "moving lights are not supported" in lib.rt_last_error().decode()
        with pytest.raises(rt.RtError):
            s.translated_records(int(mesh[lit]), (1, 0, 0), lights=True)
        assert same_view(s.view(), before)
    assert lib.rt_scene_enable_light_updates(None) == ERR_ARG
    assert lib.rt_relight_view(None, None, None, None) == ERR_ARG


# ------------------------------------------------------------------------ 3. the host entry
def test_host_entry_moves_the_lights_of_practice6_1(rt, practice):
    a = practice
    m = light_mesh(a)
    assert (tri_mesh(a) == m).sum() == 1152 == len(a["light"]) and len(a["light_node"]) == 777
    off = (0.25, 0, -0.125)
    s = rt.Scene.from_view(a)
    s.enable_light_updates()
    runs = s.translated_records(m, off, lights=True, cover=True)
    assert len(runs) == 1 and runs[0][0] == 15744 and len(runs[0][1]) == 16910 - 15744   # lights and others interleaved
    for first, tri in runs:
        s.update_triangles(first, tri)
    want = twin_arrays_lit(a, translated_mesh(a, m, off))
    v = s.view()
    for k in LIT_KEYS:
        assert same_bits(v[k], want[k]), k
    assert v["light_bvh_depth"] == a["light_bvh_depth"] and v["bvh_depth"] == a["bvh_depth"]
    assert not same_bits(want["light"], a["light"]) and not same_bits(want["light_node"], a["light_node"])
    assert same_bits(want["light"][:, 12], a["light"][:, 12])   # a translation keeps U and V: the areas stay
    light, lnode = rt.relight_view(want, s.light_map())
    assert same_bits(light, want["light"]) and same_bits(lnode, want["light_node"])
    assert same_view(rt.Scene.from_view(want).view(), v)
    # the runs of the mesh alone, one call each: the same scene
    s2 = rt.Scene.from_view(a)
    s2.enable_light_updates()
    for first, tri in s2.translated_records(m, off, lights=True):
        s2.update_triangles(first, tri)
    assert same_view(s2.view(), v)
    # and back: the reference's light list and light boxes
    s.update_triangles(15744, a["tri"][15744:16910])
    assert same_view(s.view(), a)


# ------------------------------------------------------------------------ 4. special values
def test_special_values_in_the_light_tree(rt, practice):
    a = practice
    tri, expect, nan_light = special_light_records(a)
    want = twin_arrays_lit(a, tri)
    wb = bits(want["light_node"])
    for node, k, pattern in expect:   # the restatement itself shows every case
        assert wb[node, k] == pattern, (node, k, hex(wb[node, k]), hex(pattern))
    assert {word(0.0), word(-0.0)} <= {p for _, _, p in expect}
    assert np.isnan(want["light"][nan_light, 0:13]).all() and np.isnan(want["light"][:, 12]).sum() >= 2
    s = rt.Scene.from_view(a)
    s.enable_light_updates()
    for first, count in changed_runs(a["tri"], tri):
        s.update_triangles(first, tri[first:first + count])
    v = s.view()
    assert same_bits(v["tri"], tri) and same_bits(v["node"], want["node"])
    assert np.array_equal(bits(v["light_node"]), wb)
    assert same_lights(v["light"], want["light"]) and np.isnan(v["light"][nan_light, 12])
    light, lnode = rt.relight_view(want, s.light_map())
    assert same_lights(light, want["light"]) and np.array_equal(bits(lnode), wb)


# ------------------------------------------------------------------------ 5. without the opt-in
def test_without_opt_in_an_emissive_update_is_still_refused(rt, cornell):
    lib = rt.lib()
    s = rt.Scene.from_view(cornell)
    mesh = tri_mesh(cornell)
    lit = int(np.flatnonzero(emissive_meshes(cornell)[mesh])[0])
    before = s.view()
    assert lib.rt_scene_update_tris(s.handle, lit, 1, fptr(cornell["tri"][lit:lit + 1].copy()), None, None) == ERR_ARG
    assert "moving lights are not supported" in lib.rt_last_error().decode()
    with pytest.raises(ValueError, match="emissive"):
        s.translated_records(int(mesh[lit]), (1, 0, 0))
    with pytest.raises(rt.RtError, match="has not enabled light updates"):
        s.translated_records(int(mesh[lit]), (1, 0, 0), lights=True)
    assert same_view(s.view(), before)
    assert lib.rt_scene_read_device_lights(s.handle, 0, None, None) == ERR_ARG and b"not uploaded" in lib.rt_last_error()


# ------------------------------------------------------------------------ 6. the oracle and the CLI
def test_oracle_sees_the_moved_light(rt, oracle, cornell):
    m = light_mesh(cornell)
    off = (0.1, 0, 0.05)
    s = rt.Scene.from_view(cornell)
    s.enable_light_updates()
    for first, tri in s.translated_records(m, off, lights=True, cover=True):
        s.update_triangles(first, tri)
    want = twin_arrays_lit(cornell, translated_mesh(cornell, m, off))
    assert same_view(s.view(), want)
    moved, _, _ = oracle.render(want, S)
    mine, _, _ = oracle.render(s.view(), S)
    still, _, _ = oracle.render(cornell, S)
    assert same_bits(moved, mine) and not same_bits(moved, still)


def test_cli_move_lights(rt, tmp_path, cornell):
    """Reported before anything is rendered (no GPU is touched): with RT_MOVE_LIGHTS=1 a line that names
    an emissive mesh parses (the error is the next line's); without it the line is still refused."""
    exe = os.path.join(rtref.ROOT, "raytracing-hw_amd", "rt_solution")
    em = emissive_meshes(cornell)
    lit = int(np.flatnonzero(em)[0])
    moves = tmp_path / "moves.txt"
    moves.write_text(f"{lit} 0.1 0 0.05\n{lit} 0.1 0\n")

    def run(**env_more):
        env = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}
        r = subprocess.run([exe, rtref.scene_path("cornell"), "8", "8", "1", str(tmp_path / "o.ppm")],
                           env=dict(env, RT_MOVES=str(moves), **env_more), capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and not list(tmp_path.glob("o*.ppm")), r.stderr
        return r.stderr

    err = run(RT_MOVE_LIGHTS="1")
    assert "line 2: expected groups of four numbers" in err and "is emissive" not in err
    for off in ({}, {"RT_MOVE_LIGHTS": "0"}):
        assert f"line 1: mesh {lit} is emissive" in run(**off)
