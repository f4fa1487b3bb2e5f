"""Per-pixel motion records without a GPU (include/rt_hw.h "per-pixel motion records", DESIGN.md
§5.24): rt_motion (the host function of librt_hw_amd.so, whose text is
raytracing-hw_amd/csrc/rt_motion.h) against the numpy restatement of motion_util.py, bit for bit, on
the committed dumps' triangles; an unmoved scene; cases that are exact in f32; the accuracy of the
carry against a float64 evaluation; the refusals and the CLI's usage errors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtref
from denoise_util import arrays_of, host_gbuffer, twin
from motion_util import (CARRIED, LOST, STATIC, bits, f32, np_motion, np_temporal_motion, records_on, rotated_tris, rotation,
                         translated_tris)
from refit_util import tri_mesh
from temporal_util import DEFAULTS, camera, moved, plane_frame, rotated

ERR_ARG, ERR_LIMIT = -1, -5


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def check_motion(rt, rec, tri, tri_prev):
    """rt_motion against the restatement, bit for bit; returns the host function's dict."""
    got = rt.motion(rec, tri, tri_prev)
    want = np_motion(rec, tri, tri_prev)
    diff = bits(got["records"]) != bits(want)
    assert not diff.any(), f"{diff.sum()} words differ, first at {np.argwhere(diff)[0]}"
    assert np.array_equal(got["state"], want.view(np.int32)[..., 3])
    assert same_bits(got["prev_position"], want[..., 0:3]) and same_bits(got["prev_normal"], want[..., 4:7])
    return got


def check_temporal(rt, sums, spp, rec, cam, rec_prev, hist_prev, motion, **params):
    """rt_temporal_motion against the restatement, bit for bit; returns the host function's outputs."""
    got = rt.temporal(sums, spp, rec, cam, rec_prev, hist_prev, motion=motion, **params)
    want = np_temporal_motion(sums, None, spp, rec, cam, rec_prev, hist_prev, motion["records"], **dict(DEFAULTS, **params))
    for name, g, w in zip(("history", "mean", "variance"), got, want):
        assert same_bits(g, w), f"{name}: {(bits(g) != bits(w)).sum()} words differ"
    return got


def largest_mesh(arrays):
    mesh = tri_mesh(arrays)
    return mesh == np.bincount(mesh).argmax()


# ------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["cornell_blob", "geoedge"])
def test_host_function_is_the_restatement(rt, name):
    """Synthetic records on the dump's triangles (several rounds for the small one), with misses
    and ids at n_tris - 1, n_tris and far beyond; tri_prev a translation and a rotation of the
    largest mesh, and a translation of everything."""
    arrays = arrays_of(rt, name, 8, 8)
    tri = np.ascontiguousarray(arrays["tri"], f32).copy()
    n = len(tri)
    # geoedge-style records are allowed in both arrays: a NaN vertex word, an infinite edge, a whole NaN record
    # and an overflowing edge, on triangles the records below do sit on (ids 10 .. 13 of the first round)
    tri[10, 0], tri[11, 4], tri[12, 0:12], tri[13, 3:6] = np.nan, np.inf, np.nan, 3e30
    h, w = 64, max(8, -(-min(n, 4096) // 64) + 1)
    rng = np.random.default_rng(7)
    ids = rng.permutation(np.resize(np.arange(n), h * w)).astype(np.int32)
    ids[:6] = [-1, n - 1, n, n + 1, 2 ** 31 - 1, -(2 ** 31)]
    ids[rng.integers(6, h * w, 40)] = -1
    rec = records_on(tri, ids, h, w, seed=3, mesh=tri_mesh(arrays))
    rec.view(np.int32)[0, 2:6, 7] = ids[2:6]   # (records_on writes a miss for what is no triangle: these keep their id)
    sel, everything = largest_mesh(arrays), np.ones(n, bool)
    R = rotation((0.3, 1.0, -0.2), 0.35)
    centre = tri[sel, 0:3].astype(np.float64).mean(0) if np.isfinite(tri[sel, 0:3]).all() else np.zeros(3)
    for tri_prev in (translated_tris(tri, sel, (0.25, -0.125, 0.5)), rotated_tris(tri, sel, R, centre),
                     translated_tris(tri, everything, (-0.0625, 0.03, 1.0))):
        got = check_motion(rt, rec, tri, tri_prev)
        state = got["state"].reshape(-1)
        assert state[0] == STATIC and (state[2:6] == STATIC).all()   # a miss; ids at n_tris and beyond are tested, not indexed
        assert same_bits(got["prev_position"].reshape(-1, 3)[2:6], rec.reshape(-1, 16)[2:6, 12:15])
        assert (bits(got["records"].reshape(-1, 8)[0]) == 0).all()   # a miss: zero words, state 0
        fin = np.isfinite(got["records"]).all(-1).reshape(-1)
        assert fin[state != STATIC].all()   # the function makes no NaN: a lost pixel is zero words (a static one copies its record)
        assert (state == CARRIED).sum() > 50
    # after the last one (everything moved): what cannot be carried is lost, not a NaN with state 1
    hit = (ids >= 0) & (ids < n)
    T = tri[np.where(hit, ids, 0)].astype(np.float64)
    with np.errstate(all="ignore"):
        U, V = T[:, 3:6], T[:, 6:9]
        det = (U * U).sum(-1) * (V * V).sum(-1) - (U * V).sum(-1) ** 2
    broken = hit & ~np.isfinite(T[:, 0:9]).all(-1)
    moved_bits = (bits(tri)[:, 0:9] != bits(tri_prev)[:, 0:9]).any(-1)[np.where(hit, ids, 0)]
    assert (state[broken & moved_bits] == LOST).all() and (state[broken & ~moved_bits] == STATIC).all()
    with np.errstate(all="ignore"):   # U parallel to V, a zero edge, or a sliver well below the rule's 2^-20
        flat = hit & np.isfinite(T[:, 0:9]).all(-1) & ~(det > 2.0 ** -21 * (U * U).sum(-1) * (V * V).sum(-1))
    assert (state[flat] == LOST).all()
    assert (broken & moved_bits).sum() >= 2 and (broken & ~moved_bits).sum() >= 1   # (the whole-NaN record keeps its bits)
    assert (state[hit & (ids == 13)] == LOST).all() and (ids == 13).any()   # a c overflows: det is not finite
    if name == "geoedge":   # the fixture's own degenerate triangles
        assert flat.sum() >= 6


# ------------------------------------------------------------------------ nothing moved
W, H = 16, 8
ORIGIN = camera()
# the plane frame's triangle 5 (plane_frame's records name it): the plane z = 4 over the whole view
PLANE_TRI = np.zeros((6, 12), f32)
PLANE_TRI[:, 0:9] = [-8, -8, 4, 16, 0, 0, 0, 16, 0]
PLANE_TRI[:, 9:12] = [0, 0, -1]
PLANE_TRI[:5, 2] = 9   # (the others lie elsewhere)


def test_nothing_moved(rt):
    arrays = arrays_of(rt, "cornell_blob", 8, 8)
    tri = np.ascontiguousarray(arrays["tri"], f32)
    ids = np.resize(np.arange(len(tri)), 64 * 48).astype(np.int32)
    ids[::17] = -1
    rec = records_on(tri, ids, 48, 64, seed=5)
    got = check_motion(rt, rec, tri, tri.copy())
    assert (got["state"] == STATIC).all()
    assert same_bits(got["prev_position"], rec[..., 12:15]) and same_bits(got["prev_normal"], rec[..., 0:3])
    # the step with such a plane is rt_temporal in every bit, camera moves included
    frames = [plane_frame(W, H, 1.0 + k, seed=20 + k) for k in range(4)]
    rec = frames[0][1]
    mo = rt.motion(rec, PLANE_TRI, PLANE_TRI.copy())
    assert (mo["state"] == STATIC).all()
    cams = [ORIGIN, moved(ORIGIN, (0.25, 0, 0)), rotated(ORIGIN, 0.03), moved(ORIGIN, (0, -1, 0.1))]
    hist = rt.temporal(frames[0][0], 1, rec)[0]
    for k in range(1, 4):
        plain = rt.temporal(frames[k][0], 1, rec, cams[k], rec, hist, alpha=0.3)
        with_motion = check_temporal(rt, frames[k][0], 1, rec, cams[k], rec, hist, mo, alpha=0.3)
        for a, b in zip(plain, with_motion):
            assert same_bits(a, b)
        hist = plain[0]
    assert (hist[0][..., 3] >= 2).sum() > W * H // 2


# ------------------------------------------------------------------------ exact cases
def two_plane_frames():
    (s1, rec), (s2, _) = plane_frame(W, H, 1.0, seed=1), plane_frame(W, H, 3.0, seed=2)
    return s1, s2, rec


def demodulated(sums):
    return (sums / f32(0.5)).astype(f32)   # (albedo 0.5, no emission, 1 sample)


def moved_plane(rt, offset):
    """(s1, s2, rec, h1, h2 with motion, h2 without): a still camera; the plane's triangle stood at
    v0 - offset at the first frame, so what pixel P shows now was at P - offset then."""
    s1, s2, rec = two_plane_frames()
    prev = translated_tris(PLANE_TRI, np.arange(6) == 5, -np.asarray(offset, f32))
    mo = check_motion(rt, rec, PLANE_TRI, prev)
    assert (mo["state"] == CARRIED).all()
    assert np.array_equal(mo["prev_position"], (rec[..., 12:15] - np.asarray(offset, f32)).astype(f32))
    assert np.array_equal(mo["prev_normal"], rec[..., 0:3])
    h1 = rt.temporal(s1, 1, rec)[0]
    h2 = check_temporal(rt, s2, 1, rec, ORIGIN, rec, h1, mo)[0]
    plain = rt.temporal(s2, 1, rec, ORIGIN, rec, h1)[0]
    L1, L2 = demodulated(s1), demodulated(s2)
    assert (plain[0][..., 3] == 2).all() and same_bits(plain[0][..., :3], L1 + f32(0.5) * (L2 - L1))   # its own pixel's history
    return L1, L2, h2


def test_half_a_unit_right_takes_the_left_neighbour(rt):
    L1, L2, h2 = moved_plane(rt, (0.5, 0, 0))   # fx = i - 1 exactly
    assert (h2[0][:, 0, 3] == 1).all() and (h2[0][:, 1:, 3] == 2).all()
    assert same_bits(h2[0][:, 1:, :3], L1[:, :-1] + f32(0.5) * (L2[:, 1:] - L1[:, :-1]))
    assert same_bits(h2[0][:, 0, :3], L2[:, 0])


def test_a_quarter_unit_right_blends_two_neighbours_evenly(rt):
    L1, L2, h2 = moved_plane(rt, (0.25, 0, 0))   # fx = i - 1/2: weights (1/2, 1/2)
    assert (h2[0][..., 3] == 2).all()
    Lh = (f32(0.5) * L1[:, :-1] + f32(0.5) * L1[:, 1:]) / f32(1)
    assert same_bits(h2[0][:, 1:, :3], Lh + f32(0.5) * (L2[:, 1:] - Lh))
    Lh0 = (f32(0.5) * L1[:, 0]) / f32(0.5)   # column 0: its own old pixel only, the tap at -1 is outside
    assert same_bits(h2[0][:, 0, :3], Lh0 + f32(0.5) * (L2[:, 0] - Lh0))


def test_one_unit_down_takes_the_row_above(rt):
    L1, L2, h2 = moved_plane(rt, (0, -1, 0))   # fy = j - 1 exactly
    assert (h2[0][0, :, 3] == 1).all() and (h2[0][1:, :, 3] == 2).all()
    assert same_bits(h2[0][1:, :, :3], L1[:-1] + f32(0.5) * (L2[1:] - L1[:-1]))


def test_a_lost_pixel_takes_no_history(rt):
    s1, s2, rec = two_plane_frames()
    flat = PLANE_TRI.copy()
    flat[5, 6:9] = flat[5, 3:6]   # U parallel to V now; it was a triangle before
    mo = check_motion(rt, rec, flat, PLANE_TRI)
    assert (mo["state"] == LOST).all() and (bits(mo["prev_position"]) == 0).all()
    h1 = rt.temporal(s1, 1, rec)[0]
    h2 = check_temporal(rt, s2, 1, rec, ORIGIN, rec, h1, mo)[0]
    assert (h2[0][..., 3] == 1).all() and same_bits(h2[0][..., :3], demodulated(s2))


# ------------------------------------------------------------------------ exactness of the carry
@pytest.fixture(scope="module")
def gh(tmp_path_factory):
    return twin(tmp_path_factory)


# The largest error of rt_motion's carried position and normal against the float64 evaluation of the
# same carry over cornell_blob's 48 x 48 hit pixels on the blob (181 of them; coordinates of order 1),
# the blob rotated by 0.2 rad about (0.2, 1, 0.1) through its centre, as measured on the host
# (DESIGN.md §5.24): 5.92e-8 in position (2^-24) and 1.08e-7 in the unit normal.  The test asserts
# four times that; host and device agree bit for bit, so the bound guards the rule, not a rounding.
CARRY_BOUND_P, CARRY_BOUND_N = 4 * 5.92e-8, 4 * 1.08e-7


def test_carry_is_exact_for_a_translation_and_close_for_a_rotation(rt, gh):
    name, w, h = "cornell_blob", 48, 48
    arrays = arrays_of(rt, name, w, h)
    tri = np.ascontiguousarray(arrays["tri"], f32)
    rec = host_gbuffer(rt, gh, name, w, h)[0].reshape(h, w, 16)
    sel = largest_mesh(arrays)
    ids = rec.view(np.int32)[..., 7]
    on = (ids >= 0) & sel[np.where(ids >= 0, ids, 0)]
    assert on.sum() > 100
    # a translation by powers of two: P_prev is P - offset, one f32 subtraction, wherever the triangle's
    # own v0' - v0 gives the offset back exactly (a property of the inputs)
    off = np.array([0.25, -0.125, 0.5], f32)
    prev = translated_tris(tri, sel, -off)
    mo = check_motion(rt, rec, tri, prev)
    assert (mo["state"][on] == CARRIED).all() and (mo["state"][~on] == STATIC).all()
    exact = on & ((prev[:, 0:3] - tri[:, 0:3]) == -off).all(-1)[np.where(ids >= 0, ids, 0)]
    assert exact.sum() > 0.9 * on.sum()
    assert np.array_equal(mo["prev_position"][exact], (rec[..., 12:15] - off).astype(f32)[exact])
    assert np.array_equal(mo["prev_normal"][on], rec[..., 0:3][on])
    # a rotation about an axis through the blob's centre against the same carry in float64
    centre = tri[sel, 0:3].astype(np.float64).mean(0)
    prev = rotated_tris(tri, sel, rotation((0.2, 1.0, 0.1), 0.2), centre)
    mo = check_motion(rt, rec, tri, prev)
    assert (mo["state"][on] == CARRIED).all()
    T, Tp = tri[ids[on]].astype(np.float64), prev[ids[on]].astype(np.float64)
    P, N = rec[..., 12:15][on].astype(np.float64), rec[..., 0:3][on].astype(np.float64)
    v0, U, V, v0p, Up, Vp = T[:, 0:3], T[:, 3:6], T[:, 6:9], Tp[:, 0:3], Tp[:, 3:6], Tp[:, 6:9]
    d = lambda a, b: (a * b).sum(-1)   # noqa: E731
    a, b, c = d(U, U), d(U, V), d(V, V)
    det = a * c - b * b
    e = P - v0
    u, v = (c * d(U, e) - b * d(V, e)) / det, (a * d(V, e) - b * d(U, e)) / det
    Pw = P + (v0p - v0) + u[:, None] * (Up - U) + v[:, None] * (Vp - V)
    Wn, Wp = np.cross(U, V), np.cross(Up, Vp)
    al, be = (c * d(U, N) - b * d(V, N)) / det, (a * d(V, N) - b * d(U, N)) / det
    ga = d(Wn, N) / d(Wn, Wn)
    Nw = N + al[:, None] * (Up - U) + be[:, None] * (Vp - V) + ga[:, None] * (Wp - Wn)
    err_p = float(np.abs(mo["prev_position"][on] - Pw).max())
    err_n = float(np.abs(mo["prev_normal"][on] - Nw).max())
    # the carried normal is the rotated one (a rigid motion), and the carried point the rotated point
    R = rotation((0.2, 1.0, 0.1), 0.2)
    rigid_p = float(np.abs(Pw - ((P - centre) @ R.T + centre)).max())
    rigid_n = float(np.abs(Nw - N @ R.T).max())
    print(f"\n{name} {w}x{h}, {int(on.sum())} pixels: carry against float64 |dP| {err_p:.3g} |dN| {err_n:.3g}; "
          f"float64 carry against the rotation itself |dP| {rigid_p:.3g} |dN| {rigid_n:.3g}")
    assert err_p <= CARRY_BOUND_P and err_n <= CARRY_BOUND_N
    assert rigid_p < 1e-5 and rigid_n < 1e-5   # (tri_prev is rounded to f32: a few 2^-24 of the coordinates)


# ------------------------------------------------------------------------ refusals
def test_argument_refusals(rt):
    lib = rt.lib()
    w, h = 16, 8
    s1, s2, rec = two_plane_frames()
    mo = np.zeros((h, w, 8), f32)
    hist, hist2 = np.zeros((3, h, w, 4), f32), np.zeros((3, h, w, 4), f32)
    P = lambda a: a.ctypes.data_as(rt._c_f)   # noqa: E731
    V = ctypes.c_void_p
    cam = rt.make_camera(**ORIGIN)

    def host(g=P(rec), w=w, h=h, t=P(PLANE_TRI), tp=P(PLANE_TRI), n=6, o=P(mo)):
        return lib.rt_motion(g, w, h, t, tp, n, o)

    def device(g=16, w=w, h=h, t=32, tp=48, n=6, o=64):
        return lib.rt_motion_device(V(g), w, h, V(t), V(tp), n, V(o), None)

    for call in (host, device):
        assert call(g=None) == ERR_ARG and call(t=None) == ERR_ARG and call(tp=None) == ERR_ARG and call(o=None) == ERR_ARG
        assert call(w=0) == ERR_ARG and call(h=-1) == ERR_ARG
        assert b"rt_motion" in lib.rt_last_error()
        assert call(w=1 << 16, h=1 << 15) == ERR_LIMIT
    for name in ("g", "t", "tp", "o"):   # a misaligned device pointer, before any launch
        assert device(**{name: 24}) == ERR_ARG and b"16-byte aligned" in lib.rt_last_error()
    assert host() == 0 and host(t=None, tp=None, n=0) == 0   # no triangles: every record is a miss's
    assert (mo.view(np.int32)[..., 3] == 0).all()

    def host_t(hp=P(hist2), cp=ctypes.byref(cam), gp=P(rec), m=P(mo), s=P(s1), g=P(rec), o=P(hist), w=w, h=h):
        return lib.rt_temporal_motion(s, None, 1, w, h, g, cp, gp, hp, None, o, None, None, m)

    def device_t(hp=32, cp=ctypes.byref(cam), gp=48, m=64, s=16, g=80, o=96, w=w, h=h):
        return lib.rt_temporal_motion_device(V(s), None, 1, w, h, V(g), cp, V(gp), V(hp), None, V(o), None, None, V(m), None)

    for call in (host_t, device_t):
        assert call(hp=None, cp=None, gp=None) == ERR_ARG and b"previous history" in lib.rt_last_error()   # motion, no history
        assert call(s=None) == ERR_ARG and call(g=None) == ERR_ARG and call(o=None) == ERR_ARG   # rt_temporal's
        assert call(cp=None) == ERR_ARG and call(gp=None) == ERR_ARG and call(w=0) == ERR_ARG
        assert call(w=1 << 16, h=1 << 15) == ERR_LIMIT
        assert b"rt_temporal_motion" in lib.rt_last_error()
    assert device_t(m=72) == ERR_ARG and b"16-byte aligned" in lib.rt_last_error()
    assert host_t() == 0 and host_t(m=None) == 0 and host_t(hp=None, cp=None, gp=None, m=None) == 0
    assert lib.rt_history_enable_motion(None) == ERR_ARG and lib.rt_history_motion_device(None) is None
    assert lib.rt_history_motion(None, None) == ERR_ARG
    with pytest.raises(ValueError):
        rt.temporal(s1, 1, rec, ORIGIN, rec, hist2, motion=np.zeros((h, w, 4), f32))
    assert lib.rt_abi_version() == 6 and rt.MOTION_WORDS == 8


def test_cli_usage_errors(tmp_path):
    """Reported before anything is rendered (no GPU is touched): RT_MOTION without RT_TEMPORAL or
    without RT_MOVES; with all three the moves file is the next thing looked at, RT_CAMERAS is not
    asked for."""
    exe = os.path.join(rtref.ROOT, "raytracing-hw_amd", "rt_solution")

    def run(**env_more):
        env = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}
        r = subprocess.run([exe, rtref.scene_path("cornell"), "8", "8", "1", str(tmp_path / "o.ppm")], env=dict(env, **env_more),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and not list(tmp_path.glob("o*.ppm"))
        return r.stderr

    (tmp_path / "moves.txt").write_text("1 0 0 0\n")
    moves = str(tmp_path / "moves.txt")
    assert "RT_MOTION needs RT_TEMPORAL" in run(RT_MOTION="1")
    assert "RT_MOTION needs RT_TEMPORAL" in run(RT_MOTION="1", RT_MOVES=moves)
    assert "RT_MOTION needs RT_MOVES" in run(RT_MOTION="1", RT_TEMPORAL="0.2")
    (tmp_path / "cams.txt").write_text("0 0 6  1 0 0  0 1 0  0 0 -1  0.5 0.5\n")
    assert "RT_MOTION needs RT_MOVES" in run(RT_MOTION="1", RT_TEMPORAL="0.2", RT_CAMERAS=str(tmp_path / "cams.txt"))
    err = run(RT_MOTION="1", RT_TEMPORAL="0.2", RT_MOVES=str(tmp_path / "nope.txt"))
    assert "RT_CAMERAS" not in err and "nope.txt" in err
    assert "RT_TEMPORAL must be in 0..1" in run(RT_MOTION="1", RT_TEMPORAL="1.5", RT_MOVES=moves)
    assert "RT_TEMPORAL needs RT_CAMERAS" in run(RT_MOTION="0", RT_TEMPORAL="0.2", RT_MOVES=moves)   # not opted in: as before
