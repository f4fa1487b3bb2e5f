"""Movable lights on the GPU (include/rt_hw.h rt_scene_enable_light_updates, rt_scene_update_tris* on
an opted-in scene, rt_scene_read_device_lights; the kernels are rt_lights_scatter_kernel and
rt_refit_light_level_kernel in raytracing-hw_amd/csrc/rt_refit_device.h): the device's light records
and light boxes against the reference's own, +-0 / NaN / infinite records in the light tree through
both entries, a scene whose light was moved against a scene built with the moved records (every
entry, bit for bit) and against the CPU oracle, the way back to the reference's golden, a range of
lights and other triangles interleaved, the entry rules, stale accumulators, and the CLI's
RT_MOVE_LIGHTS end to end."""
import os
import subprocess

import numpy as np
import pytest

import rtref
from refit_util import bits, changed_runs, emissive_meshes, f32, tri_mesh
from relight_util import light_mesh, same_lights, special_light_records, translated_mesh, twin_arrays_lit, wiped
from test_gpu_accum import gpu   # noqa: F401  (fixture)
from test_gpu_refit import arrays_of, frame_bytes, same_bits, update

pytestmark = pytest.mark.gpu
SOLUTION = os.path.join(rtref.ROOT, "raytracing-hw_amd", "rt_solution")
NAME, W, H, S = "cornell", 33, 17, 3
BIG, BW, BH, BS = "practice6_1", 24, 16, 2
OFFSET = (0.1, 0, 0.05)
COUNTERS = ("rays", "aabb_tests", "tri_tests", "light_queries", "light_aabb_tests", "light_tri_tests", "shading_hits")
ENTRIES = ["host", "device"]


def big_arrays(gpu):
    return arrays_of(gpu, BIG, BW, BH)


def runs_of(ids):
    return np.split(ids, np.flatnonzero(np.diff(ids) != 1) + 1) if len(ids) else []


def device_equals(scene, want):
    """Every array of the device copy and of the host mirror equals `want`."""
    d, dl, v = scene.read_device(), scene.read_device_lights(), scene.view()
    for k in ("tri", "tri_attr", "tri_tan", "node"):
        assert same_bits(d[k], want[k]) and same_bits(v[k], want[k]), k
    assert same_bits(dl["light_node"], want["light_node"]) and same_bits(v["light_node"], want["light_node"])
    assert same_lights(dl["light"], want["light"]) and same_lights(v["light"], want["light"])


def moved_light(gpu, name=NAME, w=W, h=H, entry="host"):
    """(the scene with its light mesh translated by OFFSET through `entry` after an upload and a render
    of the old geometry, the twin built by from_view, the twin's arrays, the old render)."""
    a = arrays_of(gpu, name, w, h)
    b = gpu.Scene.from_view(a)
    b.upload(0)
    old, _ = b.render_sums(1)
    b.enable_light_updates()
    for first, tri in b.translated_records(light_mesh(a), OFFSET, cover=True, lights=True):
        update(b, entry, first, tri)
    want = twin_arrays_lit(a, translated_mesh(a, light_mesh(a), OFFSET))
    return b, gpu.Scene.from_view(want), want, old


# ------------------------------------------------------------------------ 7. the reference's records
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", [BIG, NAME])
def test_device_kernels_give_the_reference_lights(gpu, name, entry):
    """practice6_1: 1,152 lights, 777 light nodes in 12 levels, leaves of up to 11; cornell: a single
    leaf that is the root (one level).  The scene is uploaded with every light's area and every light
    box NaN (words 0..11 are what the opt-in's map reads, so they stay); a first pass then sends all-NaN
    records for every emissive triangle, after which words 0..12 of every light on the device are NaN;
    the second pass sends each triangle's own record.  What is read back can only come from the kernels."""
    a = arrays_of(gpu, name)
    s = gpu.Scene.from_view(wiped(a, first_word=12))
    s.upload(0)
    d = s.read_device_lights()
    assert np.isnan(d["light"][:, 12]).all() and np.isnan(d["light_node"][:, 0:6]).all()
    s.enable_light_updates()
    lit = np.flatnonzero(emissive_meshes(a)[tri_mesh(a)])
    for run in runs_of(lit):
        update(s, entry, int(run[0]), np.full((len(run), 12), np.nan, f32))
    d = s.read_device_lights()
    assert np.isnan(d["light"][:, 0:13]).all() and same_bits(d["light"][:, 13:16], a["light"][:, 13:16])
    assert same_bits(d["light_node"][:, 6:8], a["light_node"][:, 6:8])
    for run in runs_of(lit):
        update(s, entry, int(run[0]), a["tri"][run])
    d = s.read_device_lights()
    assert same_bits(d["light"], a["light"]), f"{(bits(d['light']) != bits(a['light'])).any(axis=1).sum()} light records differ"
    assert same_bits(d["light_node"], a["light_node"]), \
        f"{(bits(d['light_node']) != bits(a['light_node'])).any(axis=1).sum()} light node records differ"
    device_equals(s, a)


# ------------------------------------------------------------------------ 8. special values
@pytest.mark.parametrize("entry", ENTRIES)
def test_special_values_in_the_light_tree_on_the_device(gpu, entry):
    """The test that catches a min / max instruction in the light kernels: the rule keeps the first
    element that attains a bound (+0 / -0 in either order) and never takes a NaN component."""
    a = big_arrays(gpu)
    tri, expect, nan_light = special_light_records(a)
    want = twin_arrays_lit(a, tri)
    for node, k, pattern in expect:
        assert bits(want["light_node"])[node, k] == pattern
    s = gpu.Scene.from_view(a)
    s.upload(0)
    s.enable_light_updates()
    for first, count in changed_runs(a["tri"], tri):
        update(s, entry, first, tri[first:first + count])
    d = s.read_device_lights()
    diff = np.argwhere(bits(d["light_node"]) != bits(want["light_node"]))
    assert len(diff) == 0, f"device light nodes differ from the restatement at (node, word) {diff[:8].tolist()}"
    assert np.isnan(d["light"][nan_light, 0:13]).all()
    device_equals(s, want)


# ------------------------------------------------------------------------ 9. render parity
def test_moved_light_is_a_scene_built_with_it(gpu, oracle):
    b, a, want_arrays, old = moved_light(gpu)
    want, _ = a.render_sums(S)
    got, _ = b.render_sums(S)
    assert same_bits(got, want) and not same_bits(old, a.render_sums(1)[0])
    still, _ = gpu.Scene.from_view(arrays_of(gpu, NAME)).render_sums(S)
    assert not same_bits(got, still)
    cpu, cnt, _ = oracle.render(want_arrays, S)
    assert same_bits(cpu.reshape(want.shape), want)
    assert same_bits(b.render_sums(S, kernel=4)[0], want) and same_bits(a.render_sums(S, kernel=4)[0], want)
    assert same_bits(b.render_sums(S, runahead=False)[0], want)
    assert same_bits(b.render_sums(S, fast=True)[0], a.render_sums(S, fast=True)[0])
    for kernel in (0, 4):
        (gc, sc), (wc, swc) = b.render_sums(S, count=True, kernel=kernel), a.render_sums(S, count=True, kernel=kernel)
        assert same_bits(gc, want) and same_bits(wc, want)
        for k in COUNTERS:
            assert sc[k] == swc[k], (kernel, k)
        assert sc["rays"] > 0 and sc["light_queries"] > 0 and sc["light_tri_tests"] > 0   # (one light leaf: no box test)
        assert [sc[k] for k in COUNTERS[:6]] == [int(x) for x in cnt], kernel
    assert same_bits(b.gbuffer()["records"], a.gbuffer()["records"])
    assert same_bits(b.render_frame(S, n_shards=1)[1], want)
    device_equals(b, want_arrays)


def test_moved_lights_of_practice6_1(gpu, oracle):
    b, a, want_arrays, _ = moved_light(gpu, BIG, BW, BH)
    (got, sc), (want, swc) = b.render_sums(BS, count=True), a.render_sums(BS, count=True)
    assert same_bits(got, want)
    cpu, cnt, _ = oracle.render(want_arrays, BS)
    assert same_bits(cpu.reshape(want.shape), want)
    for k in COUNTERS:
        assert sc[k] == swc[k], k
    assert [sc[k] for k in COUNTERS[:6]] == [int(x) for x in cnt] and sc["light_tri_tests"] > 0
    assert same_bits(b.render_sums(BS, kernel=4)[0], want)
    assert not same_bits(got, gpu.Scene.from_view(big_arrays(gpu)).render_sums(BS)[0])
    # the light pdf of a ray query walks the light BVH: paths 0, 1 and 2 against the oracle
    org, dirs = rtref.pixel_centre_rays(want_arrays)
    wf, wi = oracle.rays(want_arrays, org, dirs)
    hit = wi[:, 0].astype(bool)
    for path in (0, 1, 2):
        f, i = b.intersect_rays(org, dirs, path=path)
        assert np.array_equal(i[:, 0], wi[:, 0]) and np.array_equal(i[hit, 1], wi[hit, 1]), path
        assert np.array_equal(i[:, 2:6], wi[:, 2:6]) and rtref.same(f[:, 3], wf[:, 3]).all(), path
    assert gpu.device_selfcheck(5) == 0 and gpu.device_selfcheck(4) == 0


# ------------------------------------------------------------------------ 10. back to the golden
@pytest.mark.parametrize("entry", ENTRIES)
def test_moving_the_light_back_gives_the_reference_frame(gpu, entry):
    a = arrays_of(gpu, NAME)
    b, _, _, _ = moved_light(gpu)
    for run in runs_of(np.flatnonzero(tri_mesh(a) == light_mesh(a))):
        update(b, entry, int(run[0]), a["tri"][run])
    gold = rtref.golden(f"{NAME}_sums_{W}x{H}x{S}.rtd")
    got, st = b.render_sums(S, count=True)
    assert same_bits(got, gold["sums"].reshape(got.shape)) and st["rays"] == int(gold["counters"][0])
    assert same_bits(b.render_sums(S)[0], got)
    d = b.read_device_lights()
    assert same_bits(d["light"], a["light"]) and same_bits(d["light_node"], a["light_node"])
    device_equals(b, a)


# ------------------------------------------------------------------------ 11. a mixed range
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_range_of_lights_and_other_triangles(gpu, entry):
    a = big_arrays(gpu)
    lo, hi = 15744, 16910
    lit = emissive_meshes(a)[tri_mesh(a)]
    assert lit[lo] and lit[hi - 1] and 0 < lit[lo:hi].sum() < hi - lo and not lit[:lo].any()
    rng = np.random.default_rng(23)
    tri = a["tri"].copy()
    tri[lo:hi, 0:9] = (tri[lo:hi, 0:9] + rng.random((hi - lo, 9), dtype=f32) * f32(0.25)).astype(f32)
    s = gpu.Scene.from_view(a)
    s.upload(0)
    s.enable_light_updates()
    update(s, entry, lo, tri[lo:hi])
    want = twin_arrays_lit(a, tri)
    assert not same_bits(want["light"][:, 12], a["light"][:, 12])   # U and V changed: other areas
    device_equals(s, want)
    # a range without a light triangle: the device's light arrays are untouched
    before = s.read_device_lights()
    tri[100:357, 0:3] += f32(0.5)
    update(s, entry, 100, tri[100:357])
    after = s.read_device_lights()
    assert all(before[k].tobytes() == after[k].tobytes() for k in before)
    device_equals(s, twin_arrays_lit(a, tri))


# ------------------------------------------------------------------------ 12. entry rules
def test_device_entry_refusals_on_an_opted_in_scene(gpu):
    import torch
    a = arrays_of(gpu, NAME)
    s = gpu.Scene.from_view(a)
    s.upload(0)
    s.enable_light_updates()
    t = torch.from_numpy(a["tri"]).cuda()
    lit = int(np.flatnonzero(emissive_meshes(a)[tri_mesh(a)])[0])
    before, before_l = s.read_device(), s.read_device_lights()
    with pytest.raises(gpu.RtError, match="beyond"):
        s.update_triangles(len(a["tri"]) - 1, t[0:2], device=0)
    with pytest.raises(gpu.RtError, match="16-byte aligned"):
        s.update_triangles(lit, t.reshape(-1)[1:13], device=0)
    with pytest.raises(gpu.RtError, match="not uploaded to device 63"):
        s.update_triangles(lit, t[lit:lit + 1], device=63)
    lib = gpu.lib()
    assert lib.rt_scene_update_tris_device(s.handle, 0, lit, 1, None, None, None, None) == -1 and b"NULL tri" in lib.rt_last_error()
    after, after_l = s.read_device(), s.read_device_lights()
    assert all(same_bits(before[k], after[k]) for k in before) and all(same_bits(before_l[k], after_l[k]) for k in before_l)
    device_equals(s, a)
    s.update_triangles(lit, t[lit:lit + 1], device=0)   # and the emissive triangle itself is accepted
    device_equals(s, a)


def test_later_uploads_of_a_moved_light_are_current(gpu):
    if gpu.device_count() < 2:
        pytest.skip("needs two GPUs")
    b, _, want, _ = moved_light(gpu)
    b.upload(1)
    d = b.read_device_lights(1)
    assert same_lights(d["light"], want["light"]) and same_bits(d["light_node"], want["light_node"])
    a = arrays_of(gpu, NAME)
    for run in runs_of(np.flatnonzero(tri_mesh(a) == light_mesh(a))):   # the host entry updates both copies
        b.update_triangles(int(run[0]), a["tri"][run])
    for dev in (0, 1):
        d = b.read_device_lights(dev)
        assert same_bits(d["light"], a["light"]) and same_bits(d["light_node"], a["light_node"])


def test_accumulators_go_stale_after_a_light_move(gpu):
    a = arrays_of(gpu, NAME)
    m = light_mesh(a)
    b = gpu.Scene.from_view(a)
    b.enable_light_updates()
    twin = gpu.Scene.from_view(twin_arrays_lit(a, translated_mesh(a, m, OFFSET)))
    accs = [b.accumulator(), b.accumulator(fast=True, fast_chunk=2)]
    for acc in accs:
        acc.add(2)
    old = [acc.sums() for acc in accs]
    for first, tri in b.translated_records(m, OFFSET, cover=True, lights=True):
        b.update_triangles(first, tri)
    lib = gpu.lib()
    for acc, was in zip(accs, old):
        assert lib.rt_accum_add(acc._h, 1, None, None) == -1 and b"rt_accum_reset" in lib.rt_last_error()
        with pytest.raises(gpu.RtError, match="rt_accum_reset"):
            acc.frame()
        assert same_bits(acc.sums(), was) and acc.samples == 2 and (acc.counts() == 2).all()
        acc.reset()
    fresh = [twin.accumulator(), twin.accumulator(fast=True, fast_chunk=2)]
    for acc, new in zip(accs, fresh):
        for x in (acc, new):
            x.add(3)
            x.add(2)
        assert same_bits(acc.sums(), new.sums()) and np.array_equal(acc.state(), new.state())
    assert same_bits(accs[0].sums(), twin.render_sums(5)[0])
    assert not same_bits(accs[0].sums(), gpu.Scene.from_view(a).render_sums(5)[0])


# ------------------------------------------------------------------------ 13. CLI
def test_cli_move_lights(gpu, tmp_path):
    scene = gpu.Scene.load(rtref.scene_path(NAME), W, H, S)
    a = scene.view()
    m = light_mesh(a)
    moves = tmp_path / "moves.txt"
    moves.write_text(f"# mesh dx dy dz\n{m} 0 0 0\n{m} {OFFSET[0]} {OFFSET[1]} {OFFSET[2]}\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}
    r = subprocess.run([SOLUTION, rtref.scene_path(NAME), str(W), str(H), str(S), str(tmp_path / "out.ppm")],
                       env=dict(env, RT_GPUS="1", RT_MOVES=str(moves), RT_MOVE_LIGHTS="1"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    gold = open(os.path.join(rtref.GOLD, f"{NAME}_{W}x{H}x{S}.ppm"), "rb").read()
    assert (tmp_path / "out.0000.ppm").read_bytes() == gold   # the reference's frame
    twin = gpu.Scene.from_view(twin_arrays_lit(a, translated_mesh(a, m, OFFSET)))
    assert np.array_equal(frame_bytes(tmp_path / "out.0001.ppm"), gpu.tonemap(twin.render_sums(S)[0], S))
    assert (tmp_path / "out.0001.ppm").read_bytes() != gold
