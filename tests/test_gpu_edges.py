"""GPU parity outside the other fixtures' envelope: ray depths 1..15, a zfar that clips, textures
of odd sizes (tiled texel addressing with partial tiles, 1-texel sides, the p - floor(p) == 1
wrap), the emissive texture slot, and more meshes than the wavefront shade kernel keeps in LDS.

Every assertion is bit equality of the float32 sums (and of the six traversal counters where the
schedule counts), against the reference's own goldens (texedge at depths 6, 1, 2 and 15; cornell at
depth 15: tools/make_goldens.py --edges) or, for array edits no glTF can express, against the CPU
oracle on the same arrays.  Every edited case first shows that the edit changes at least 10% of
the oracle's pixels, so a variation the view ignores cannot pass as parity.
"""
import os

import numpy as np
import pytest

import rtref

pytestmark = pytest.mark.gpu

# (scene, W, H, spp, ray depth or None for the scene's own 6)
# (geoedge: degenerate geometry and scale extremes; its golden frame holds no
# NaN, tests/test_geoedge.py, so bit equality is the whole comparison rule there too)
GOLDEN_CASES = [("texedge", 40, 24, 6, None)] + rtref.DEPTH_CASES + [("geoedge", 24, 16, 4, None)]
# texture sizes (W, H) dealt over sponza_mini's 69 texture slots
ODD_SIZES = [(1, 1), (1, 7), (5, 1), (5, 3), (3, 5), (13, 6), (2, 2), (7, 9), (6, 13), (4, 4), (9, 4), (4, 10)]


@pytest.fixture(scope="module")
def gpu(rt):
    import torch   # initialises the HIP runtime librt_hw_amd.so shares (see test_gpu_parity.py)
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    if rt.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return rt


def _counters(st):
    return [st["rays"], st["aabb_tests"], st["tri_tests"], st["light_queries"], st["light_aabb_tests"],
            st["light_tri_tests"]]


def _same(out, ref, what):
    bad = (rtref.bits(out).reshape(-1, 3) != rtref.bits(ref).reshape(-1, 3)).any(1)
    assert bad.sum() == 0, f"{what}: {bad.sum()} of {len(bad)} pixels differ, first {np.flatnonzero(bad)[:8]}"


def _check_variants(gpu, scene, s, ref, cnt, tag, light_split=True):
    """Every schedule of the parity render on `scene` against ref (h, w, 3) and the six counters."""
    h = scene.height
    cnt = [int(x) for x in cnt]
    for kw, sched in [(dict(count=True, heavy_order=True), gpu.SCHED_LANE),
                      (dict(count=True, natural_order=True), gpu.SCHED_LANE),
                      (dict(count=True, kernel=4), gpu.SCHED_WAVEFRONT)] + \
                     ([(dict(count=True, light_split=True), gpu.SCHED_LIGHT_SPLIT)] if light_split else []):
        out, st = scene.render_sums(s, **kw)
        _same(out, ref, f"{tag} {kw}")
        assert _counters(st) == cnt, (tag, kw)
        assert st["schedule"] == sched, (tag, kw)
    for kw, sched in [(dict(), gpu.SCHED_RUNAHEAD), (dict(runahead=False), gpu.SCHED_LANE),
                      (dict(kernel=4), gpu.SCHED_WAVEFRONT)] + \
                     ([(dict(light_split=True), gpu.SCHED_LIGHT_SPLIT)] if light_split else []):
        out, st = scene.render_sums(s, **kw)
        _same(out, ref, f"{tag} {kw}")
        assert st["schedule"] == sched, (tag, kw)
    frame = np.full_like(ref, np.nan)
    for rank in range(8):
        rows = gpu.shard_rows(h, rank, 8, 8)
        if len(rows):
            frame[rows], st = scene.render_sums(s, rank=rank, world=8, heavy_order=rank % 2 == 0)
            assert st["schedule"] == gpu.SCHED_RUNAHEAD, (tag, rank)
    _same(frame, ref, f"{tag} 8-way shards")


def _changed(ref, base):
    """Fraction of pixels whose bits differ between two oracle frames."""
    return float((rtref.bits(ref).reshape(-1, 3) != rtref.bits(base).reshape(-1, 3)).any(1).mean())


# ------------------------------------------------------------------ against the reference goldens
@pytest.mark.parametrize("name,w,h,s,depth", GOLDEN_CASES)
def test_goldens_every_schedule(gpu, name, w, h, s, depth):
    """The reference's sums and counters through every schedule, from the reference's arrays
    and from this build's loader, and through the three-shard device gather with its 8-bit
    finish."""
    g = rtref.sums_golden(name, w, h, s, depth)
    ref = g["sums"].reshape(h, w, 3)
    arrays = rtref.ref_arrays(gpu, name, w, h, s)
    loaded = gpu.Scene.load(rtref.scene_path(name), w, h, s)
    if depth:
        arrays = rtref.with_depth(arrays, depth)
        loaded = gpu.Scene.from_view(rtref.with_depth(loaded.view(), depth))
    _check_variants(gpu, gpu.Scene.from_view(arrays), s, ref, g["counters"], f"{name} d{depth} reference arrays")
    out, st = loaded.render_sums(s, count=True)
    _same(out, ref, f"{name} d{depth} loader")
    assert _counters(st) == [int(x) for x in g["counters"]]
    _same(loaded.render_sums(s)[0], ref, f"{name} d{depth} loader, runahead")
    rgb, sums, st = loaded.render_frame(s, devices=[0] * 3, row_block=4)
    _same(sums, ref, f"{name} d{depth} render_frame")
    ppm = os.path.join(rtref.GOLD, f"{name}_{w}x{h}x{s}" + (f"_d{depth}" if depth else "") + ".ppm")
    if os.path.exists(ppm):   # the reference's own finished frame of these sums
        assert rgb.tobytes() == open(ppm, "rb").read()[len(b"P6\n%d %d\n255\n" % (w, h)):]
    else:                     # (the host finish is pinned to the reference's by finish_37x23x16)
        assert np.array_equal(rgb, gpu.tonemap(ref, s))
    assert st["pixels"] == w * h


@pytest.mark.parametrize("name,w,h,s,depth", [("texedge", 40, 24, 6, None), ("cornell", 33, 17, 8, 15),
                                              ("geoedge", 24, 16, 4, None)])
def test_fast_mode_vs_oracle(gpu, oracle, name, w, h, s, depth):
    """Fast mode (per-sample Philox streams) on the odd textures, the emissive slot and the
    clip, and at depth 15, against the oracle's restatement of it."""
    arrays = rtref.ref_arrays(gpu, name, w, h, s)
    if depth:
        arrays = rtref.with_depth(arrays, depth)
    scene = gpu.Scene.from_view(arrays)
    for chunk in (2, 1):
        out, st = scene.render_sums(s, fast=True, fast_chunk=chunk, count=True)
        ref, _ = oracle.render_fast(arrays, s, chunk)
        _same(out, ref, f"{name} d{depth} fast chunk {chunk}")
        assert st["schedule"] == gpu.SCHED_FAST and st["samples"] == w * h * s


# ------------------------------------------------------------------ against the oracle on edited arrays
@pytest.fixture(scope="module")
def cornell_base(rt, oracle):
    a = rtref.ref_arrays(rt, "cornell", 33, 17, 8)
    return a, oracle.render(a, 8)[0]


@pytest.fixture(scope="module")
def sponza_base(rt, oracle):
    a = rtref.ref_arrays(rt, "sponza_mini", 48, 27, 4)
    return a, oracle.render(a, 4)[0]


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 7, 9, 10, 13, 15])
def test_ray_depths_vs_oracle(gpu, oracle, cornell_base, depth):
    """Every residue of the folds' batch-of-four boundary and both ends of the range, with
    every second material translucent so the lane records' alpha plane is live on long paths."""
    base, base_ref = cornell_base
    w, h, s = 33, 17, 8
    a = rtref.with_depth(base, depth)
    a["mesh_f"] = base["mesh_f"].copy()
    a["mesh_f"][::2, 8] = np.float32(0.37)
    ref, cnt, _ = oracle.render(a, s)
    assert _changed(ref, base_ref) >= 0.10
    _check_variants(gpu, gpu.Scene.from_view(a), s, ref.reshape(h, w, 3), cnt, f"cornell depth {depth}")


@pytest.mark.parametrize("zfar", [3.0, 8.0, 15.0])
def test_zfar_clip_vs_oracle(gpu, oracle, sponza_base, zfar):
    """max_distance inside the scene: a clipped hit ends the path unshaded and without an RNG
    draw (1.14, 2.14 and 2.53 rays per sample against 2.87 unclipped)."""
    base, base_ref = sponza_base
    w, h, s = 48, 27, 4
    a = dict(base)
    a["max_distance"] = zfar
    ref, cnt, _ = oracle.render(a, s)
    assert _changed(ref, base_ref) >= 0.10
    assert int(cnt[0]) < 0.95 * 2.87 * w * h * s
    _check_variants(gpu, gpu.Scene.from_view(a), s, ref.reshape(h, w, 3), cnt, f"sponza_mini zfar {zfar}")


def _odd_textures(base, emissive):
    """sponza_mini's 69 texture slots refilled with seeded random RGBA texels of ODD_SIZES;
    emissive: every textured mesh's emission slot points at its base texture."""
    a = dict(base)
    rng = np.random.default_rng(20261019)
    info = np.asarray(base["tex_info"], np.uint32).copy()
    texels, off = [], 0
    for t in range(len(info)):
        tw, th = ODD_SIZES[t % len(ODD_SIZES)]
        info[t, 0:3] = (off, tw, th)
        texels.append(rng.integers(0, 256, tw * th * 4, dtype=np.uint8))
        off += tw * th
    a["tex_info"], a["texels"] = info, np.concatenate(texels)
    if emissive:
        a["mesh_tex"] = np.asarray(base["mesh_tex"], np.int32).copy()
        textured = a["mesh_tex"][:, 0] >= 0
        assert textured.sum() >= 20
        a["mesh_tex"][textured, 3] = a["mesh_tex"][textured, 0]
        a["mesh_f"] = base["mesh_f"].copy()
        a["mesh_f"][:, 3:6] = np.array([0.5, 0.25, 1.0], np.float32)
    return a


@pytest.mark.parametrize("depth", [6, 15])
@pytest.mark.parametrize("emissive", [False, True])
def test_odd_textures_vs_oracle(gpu, oracle, sponza_base, emissive, depth):
    """The tiled texel addressing on sizes with W != H, partial last tiles and 1-texel sides,
    in the base, normal and metallic-roughness slots and, with `emissive`, in the emission
    slot (its sRGB decode) of every textured mesh."""
    base, base_ref = sponza_base
    w, h, s = 48, 27, 4
    a = rtref.with_depth(_odd_textures(base, emissive), depth)
    ref, cnt, _ = oracle.render(a, s)
    assert _changed(ref, base_ref) >= 0.10
    if emissive:   # the emission slot is live: not the frame of the same textures without it
        plain, _, _ = oracle.render(rtref.with_depth(_odd_textures(base, False), depth), s)
        assert _changed(ref, plain) >= 0.10
    _check_variants(gpu, gpu.Scene.from_view(a), s, ref.reshape(h, w, 3), cnt,
                    f"sponza_mini odd textures emissive={emissive} depth {depth}")


def _many_meshes(base, n):
    """sponza_mini's mesh rows replicated to n (copy k of row m at m + k * rows), each copy's
    base colour, alpha and roughness perturbed, the triangles' mesh ids dealt over the copies."""
    a = dict(base)
    rows = len(base["mesh_f"])
    src = np.arange(n) % rows
    rng = np.random.default_rng(n)
    mf = np.asarray(base["mesh_f"], np.float32)[src].copy()
    copies = np.arange(n) >= rows
    mf[copies, 0:3] = (mf[copies, 0:3] * rng.uniform(0.3, 1.0, (copies.sum(), 3))).astype(np.float32)
    mf[copies, 7] = (mf[copies, 7] * rng.uniform(0.2, 1.0, copies.sum())).astype(np.float32)
    mf[copies, 8] = rng.uniform(0.4, 1.0, copies.sum()).astype(np.float32)
    a["mesh_f"] = mf
    a["mesh_tex"] = np.asarray(base["mesh_tex"], np.int32)[src].copy()
    a["mesh_normal_transform"] = np.asarray(base["mesh_normal_transform"], np.float64)[src].copy()
    attr = np.asarray(base["tri_attr"], np.float32).copy()
    ids = attr[:, 15].view(np.int32).copy()
    n_copies = (n - 1 - ids) // rows + 1                 # copies of each triangle's mesh row
    ids = ids + rows * (np.arange(len(ids)) % n_copies)
    assert ids.min() >= 0 and ids.max() == n - 1 and len(np.unique(ids)) > min(n, 64) // 2
    attr[:, 15] = ids.astype(np.int32).view(np.float32)
    a["tri_attr"] = attr
    return a


@pytest.mark.parametrize("n", [64, 65, 200])
def test_mesh_counts_vs_oracle(gpu, oracle, sponza_base, n):
    """The wavefront shade kernel's material tables: in LDS up to 64 meshes (exactly 64 here),
    read from memory above (65 and 200); the lane-resident kernels on the same arrays."""
    base, base_ref = sponza_base
    w, h, s = 48, 27, 4
    a = _many_meshes(base, n)
    ref, cnt, _ = oracle.render(a, s)
    assert _changed(ref, base_ref) >= 0.10
    _check_variants(gpu, gpu.Scene.from_view(a), s, ref.reshape(h, w, 3), cnt, f"sponza_mini {n} meshes")


@pytest.mark.parametrize("kernel", [0, 4])
@pytest.mark.parametrize("depth", [0, 16])
def test_ray_depth_outside_the_range_is_refused(gpu, cornell_base, depth, kernel):
    """ray_depth 0 and 16 are RT_ERR_LIMIT (include/rt_hw.h), on both kernels."""
    import ctypes
    scene = gpu.Scene.from_view(rtref.with_depth(cornell_base[0], depth))
    with pytest.raises(gpu.RtError, match="ray_depth"):
        scene.render_sums(8, kernel=kernel)
    out = np.zeros((17, 33, 3), np.float32)
    p = gpu.RtParams(8, 0, 1, 8, 0, kernel, 0, 0, 0)
    assert gpu.lib().rt_render(scene.handle, ctypes.byref(p), out.ctypes.data_as(gpu._c_f), None) == -5   # RT_ERR_LIMIT
    assert not out.any()
