"""The movable camera and the reprojected temporal history without a GPU: rt_scene_get/set_camera on
the host; rt_temporal (the host function of librt_hw_amd.so, whose text is
raytracing-hw_amd/csrc/rt_temporal.h) against a numpy float32 restatement written from
include/rt_hw.h, bit for bit; cases that are exact in f32; what rejects a history; the refusals; and
that the history reduces the error of independent 1-sample frames."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtref
from denoise_util import arrays_of, f32, host_gbuffer, synthetic, twin
from temporal_util import DEFAULTS, camera, moved, np_temporal, plane_frame, rotated

ERR_ARG, ERR_LIMIT = -1, -5
bits = rtref.bits
# the camera synthetic()'s positions were made with: rays ((x + .5) / w - .5, (y + .5) / h - .5, 1), y down
SYN_CAM = camera(axes=((1, 0, 0), (0, -1, 0), (0, 0, 1)), tan=(0.5, 0.5))


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def check(rt, sums, counts_or_spp, rec, cam=None, rec_prev=None, hist_prev=None, **params):
    """rt_temporal against the restatement, bit for bit; returns the host function's outputs."""
    got = rt.temporal(sums, counts_or_spp, rec, cam, rec_prev, hist_prev, **params)
    counts, spp = (None, counts_or_spp) if np.ndim(counts_or_spp) == 0 else (counts_or_spp, 0)
    want = np_temporal(sums, counts, spp, rec, cam, rec_prev, hist_prev, **dict(DEFAULTS, **params))
    for name, g, w in zip(("history", "mean", "variance"), got, want):
        assert same_bits(g, w), f"{name}: {(bits(g) != bits(w)).sum()} words differ"
    return got


# ------------------------------------------------------------------------ camera
def test_camera_round_trip_on_a_scene_that_was_never_uploaded(rt):
    s = rt.Scene.load(rtref.scene_path("cornell"), 8, 8, 1)
    v, c = s.view(), s.camera()
    assert same_bits(c["pos"], v["cam_pos"]) and same_bits(c["axes"], v["cam_axes"]) and same_bits(c["tan_half_fov"], v["tan_half_fov"])
    new = rotated(moved(c, (0.25, -0.5, 1)), 0.3)
    new["tan_half_fov"] = np.array([0.75, 0.4], f32)
    s.set_camera(**new)
    got, v = s.camera(), s.view()
    for k, vk in (("pos", "cam_pos"), ("axes", "cam_axes"), ("tan_half_fov", "tan_half_fov")):
        assert same_bits(got[k], new[k]) and same_bits(v[vk], new[k])
    assert np.allclose(v["cam_fov"], 2 * np.arctan(new["tan_half_fov"].astype(np.float64)), rtol=1e-6)   # (2 * atanf: an ulp or two)
    s.set_camera(pos=(1, 2, 3))   # an omitted part is kept
    got = s.camera()
    assert same_bits(got["pos"], np.array([1, 2, 3], f32)) and same_bits(got["axes"], new["axes"])
    assert same_bits(got["tan_half_fov"], new["tan_half_fov"])


def test_camera_refusals(rt):
    lib = rt.lib()
    s = rt.Scene.load(rtref.scene_path("cornell"), 8, 8, 1)
    before = s.camera()
    c = rt.make_camera(**{"pos": before["pos"], "axes": before["axes"], "tan_half_fov": before["tan_half_fov"]})
    assert lib.rt_scene_set_camera(None, ctypes.byref(c)) == ERR_ARG and lib.rt_scene_set_camera(s.handle, None) == ERR_ARG
    assert lib.rt_scene_get_camera(None, ctypes.byref(c)) == ERR_ARG and lib.rt_scene_get_camera(s.handle, None) == ERR_ARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        for part, n in (("pos", 3), ("axes", 9), ("tan_half_fov", 2)):
            for i in range(n):
                with pytest.raises(rt.RtError):
                    arr = np.array(before[part], f32).reshape(-1).copy()
                    arr[i] = bad
                    s.set_camera(**{part: arr})
    for tan in ((0, 0.5), (0.5, 0), (-1, 0.5), (0.5, -0.25)):
        with pytest.raises(rt.RtError):
            s.set_camera(tan_half_fov=tan)
    after = s.camera()
    assert all(same_bits(before[k], after[k]) for k in before)   # a refused call changes nothing


# ------------------------------------------------------------------------ the restatement
def test_host_function_is_the_specification_on_chains(rt):
    """Two- and three-frame chains of the synthetic frame (misses, a NaN pixel, an inf pixel,
    zero-count pixels), from the NULL-history first frame on, under several previous cameras."""
    frames = [synthetic(40, 24, seed=s) for s in (1, 2, 3)]
    rec = frames[0][2]
    cams = [SYN_CAM, moved(SYN_CAM, (0.07, -0.03, 0.0)), rotated(SYN_CAM, 0.04), moved(rotated(SYN_CAM, -0.02), (0, 0, -0.5)),
            moved(SYN_CAM, (0, 0, 9))]   # (the last one looks at everything from behind it: no history)
    h1 = check(rt, frames[0][0], frames[0][1], rec)[0]
    assert (h1[0][..., 3] == 1).sum() > 600 and (h1[0][..., 3] == 0).sum() > 10
    seen = []
    for cam in cams:
        h2, _, v2 = check(rt, frames[1][0], frames[1][1], rec, cam, rec, h1)
        seen.append(int((h2[0][..., 3] >= 2).sum()))
        for cam3 in (SYN_CAM, cams[1]):
            h3, _, v3 = check(rt, frames[2][0], 4, rec, cam3, rec, h2, alpha=0.05, alpha_moments=0.5, normal_min=0.99)
        check(rt, frames[2][0], frames[2][1], rec, cam, rec, h2, sigma_plane=0.5, max_history=2)
    assert seen[0] > 700 and min(seen[1:4]) > 300 and seen[4] == 0   # (the chains do exercise the look-up)
    assert (v3 > 0).any()


# ------------------------------------------------------------------------ exact cases
W, H = 16, 8
ORIGIN = camera()


def two_plane_frames():
    (s1, rec), (s2, _) = plane_frame(W, H, 1.0, seed=1), plane_frame(W, H, 3.0, seed=2)
    return s1, s2, rec


def demodulated(sums):
    return (sums / f32(0.5)).astype(f32)   # (albedo 0.5, no emission, 1 sample)


@pytest.mark.parametrize("alpha", [0.2, 0.75])
def test_same_camera_is_an_exact_blend(rt, alpha):
    s1, s2, rec = two_plane_frames()
    h1 = check(rt, s1, 1, rec)[0]
    assert (h1[0][..., 3] == 1).all() and same_bits(h1[0][..., :3], demodulated(s1)) and same_bits(h1[1][..., :3], demodulated(s1))
    h2, mean, var = check(rt, s2, 1, rec, ORIGIN, rec, h1, alpha=alpha)
    L1, L2 = demodulated(s1), demodulated(s2)
    a = max(f32(alpha), f32(0.5))
    assert (h2[0][..., 3] == 2).all()
    assert same_bits(h2[0][..., :3], L1 + a * (L2 - L1))
    assert same_bits(mean, h2[0][..., :3] * f32(0.5) + f32(0))
    am = max(f32(0.2), f32(0.5))
    M1, M2 = L1 + am * (L2 - L1), L1 * L1 + am * (L2 * L2 - L1 * L1)
    vc = np.maximum(M2 - M1 * M1, f32(0))
    assert same_bits(var, ((vc[..., 0] + vc[..., 1]) + vc[..., 2]) * a) and (var > 0).all()


def test_half_a_unit_right_takes_the_left_neighbour(rt):
    s1, s2, rec = two_plane_frames()
    h1 = check(rt, s1, 1, rec)[0]
    h2 = check(rt, s2, 1, rec, moved(ORIGIN, (0.5, 0, 0)), rec, h1)[0]   # fx = i - 1 exactly
    L1, L2 = demodulated(s1), demodulated(s2)
    assert (h2[0][:, 0, 3] == 1).all() and (h2[0][:, 1:, 3] == 2).all()
    assert same_bits(h2[0][:, 1:, :3], L1[:, :-1] + f32(0.5) * (L2[:, 1:] - L1[:, :-1]))
    assert same_bits(h2[0][:, 0, :3], L2[:, 0])


def test_a_quarter_unit_right_blends_two_neighbours_evenly(rt):
    s1, s2, rec = two_plane_frames()
    h1 = check(rt, s1, 1, rec)[0]
    h2 = check(rt, s2, 1, rec, moved(ORIGIN, (0.25, 0, 0)), rec, h1)[0]   # fx = i - 1/2: weights (1/2, 1/2)
    L1, L2 = demodulated(s1), demodulated(s2)
    assert (h2[0][..., 3] == 2).all()
    Lh = (f32(0.5) * L1[:, :-1] + f32(0.5) * L1[:, 1:]) / f32(1)
    assert same_bits(h2[0][:, 1:, :3], Lh + f32(0.5) * (L2[:, 1:] - Lh))
    Lh0 = (f32(0.5) * L1[:, 0]) / f32(0.5)   # column 0: its own old pixel only, the tap at -1 is outside
    assert same_bits(h2[0][:, 0, :3], Lh0 + f32(0.5) * (L2[:, 0] - Lh0))


def test_one_unit_down_takes_the_row_above(rt):
    s1, s2, rec = two_plane_frames()
    h1 = check(rt, s1, 1, rec)[0]
    h2 = check(rt, s2, 1, rec, moved(ORIGIN, (0, -1, 0)), rec, h1)[0]   # fy = j - 1 exactly
    L1, L2 = demodulated(s1), demodulated(s2)
    assert (h2[0][0, :, 3] == 1).all() and (h2[0][1:, :, 3] == 2).all()
    assert same_bits(h2[0][1:, :, :3], L1[:-1] + f32(0.5) * (L2[1:] - L1[:-1]))


def test_tiny_alpha_is_the_running_mean(rt):
    """alpha = alpha_moments = 1e-6 and K = 6 frames of one geometry: N' = K, L' the sequential
    formula with a = 1 / N', the variance from the moments as written."""
    K = 6
    frames = [plane_frame(W, H, 1.0 + k, seed=10 + k) for k in range(K)]
    rec = frames[0][1]
    hist, L, M1, M2 = None, None, None, None
    for k, (s, _) in enumerate(frames):
        hist, mean, var = check(rt, s, 1, rec, ORIGIN if k else None, rec if k else None, hist, alpha=1e-6, alpha_moments=1e-6)
        Lk = demodulated(s)
        if k == 0:
            L, M1, M2 = Lk, Lk, Lk * Lk
        else:
            a = f32(1) / f32(k + 1)
            L, M1, M2 = L + a * (Lk - L), M1 + a * (Lk - M1), M2 + a * (Lk * Lk - M2)
        assert (hist[0][..., 3] == k + 1).all()
        assert same_bits(hist[0][..., :3], L) and same_bits(hist[1][..., :3], M1) and same_bits(hist[2][..., :3], M2)
    vc = np.maximum(M2 - M1 * M1, f32(0))
    assert same_bits(var, ((vc[..., 0] + vc[..., 1]) + vc[..., 2]) * (f32(1) / f32(K)))
    exact = np.mean([demodulated(s).astype(np.float64) for s, _ in frames], 0)
    assert np.abs(L / exact - 1).max() < 1e-5   # (K roundings of 2^-24 each)
    hist = check(rt, frames[0][0], 1, rec, ORIGIN, rec, hist, max_history=4)[0]
    assert (hist[0][..., 3] == 4).all()


# ------------------------------------------------------------------------ rejection and miscellany
def lengths_after(rt, rec_now, cam=ORIGIN, rec_prev=None, **params):
    s1, s2, rec = two_plane_frames()
    rec_prev = rec if rec_prev is None else rec_prev
    h1 = check(rt, s1, 1, rec_prev)[0]
    return check(rt, s2, 1, rec_now, cam, rec_prev, h1, **params)[0][0][..., 3]


def test_each_test_alone_rejects_the_history(rt):
    _, _, rec = two_plane_frames()
    at = (3, 5)
    assert (lengths_after(rt, rec) == 2).all()
    other = rec.copy()
    other.view(np.int32)[at][11] = 9   # a different mesh id
    n = lengths_after(rt, other)
    assert n[at] == 1 and (n == 2).sum() == W * H - 1
    tilted = rec.copy()
    tilted[at][0:3] = [np.sqrt(f32(1) - f32(0.89) ** 2), 0, -0.89]   # dot 0.89 < 0.9
    n = lengths_after(rt, tilted)
    assert n[at] == 1 and (n == 2).sum() == W * H - 1
    assert lengths_after(rt, tilted, normal_min=0.85)[at] == 2
    off = rec.copy()
    off[at][14] = rec[at][14] + f32(0.03) * rec[at][3]   # off the previous plane by more than 0.02 t
    n = lengths_after(rt, off)
    assert n[at] == 1
    assert lengths_after(rt, off, sigma_plane=0.5)[at] == 2
    assert (lengths_after(rt, rec, moved(ORIGIN, (0, 0, 4))) == 1).all()    # z = 0: not in front of the previous camera
    assert (lengths_after(rt, rec, moved(ORIGIN, (0, 0, 5))) == 1).all()    # behind it
    assert (lengths_after(rt, rec, moved(ORIGIN, (9, 0, 0))) == 1).all()    # projected outside the frame
    empty = rec.copy()   # a previous pixel without history (a miss then) offers none
    empty.view(np.int32)[at][7] = -1
    n = lengths_after(rt, rec, rec_prev=empty)
    assert n[at] == 1 and (n == 2).sum() == W * H - 1


def test_pass_and_fill_pixels(rt):
    s1, s2, rec = two_plane_frames()
    h1 = check(rt, s1, 1, rec)[0]
    miss, fill, nan = (1, 2), (4, 7), (6, 11)
    rec2 = rec.copy()
    rec2[miss] = 0
    rec2.view(np.int32)[miss][7] = rec2.view(np.int32)[miss][11] = -1
    counts = np.ones((H, W), np.int32)
    counts[fill] = 0
    s2 = s2.copy()
    s2[fill] = 0
    s2[nan] = [1, np.nan, 1]
    h2, mean, var = check(rt, s2, counts, rec2, ORIGIN, rec, h1)
    for at in (miss, nan):   # pass: zero words, its own mean, no variance
        assert (bits(h2[:, at[0], at[1]]) == 0).all() and same_bits(mean[at], s2[at]) and var[at] == 0
    # fill: the history as it is, no frame added
    assert same_bits(h2[:, fill[0], fill[1]], h1[:, fill[0], fill[1]]) and h2[0][fill][3] == 1
    assert same_bits(mean[fill], h1[0][fill][:3] * f32(0.5) + f32(0))
    h0, mean0, _ = check(rt, s2, counts, rec2)   # without history a fill pixel is zero words and gives E
    assert (bits(h0[:, fill[0], fill[1]]) == 0).all() and (mean0[fill] == 0).all()
    h3 = check(rt, s1, 1, rec, ORIGIN, rec2, h2)[0]   # the pass pixels offer no history to the next frame
    assert h3[0][miss][3] == 1 and h3[0][nan][3] == 1 and h3[0][fill][3] == 2 and h3[0][0, 0][3] == 3


def test_argument_refusals(rt):
    lib = rt.lib()
    sums, counts, rec, _ = synthetic(40, 24)
    hist, hist2 = np.zeros((3, 24, 40, 4), f32), np.zeros((3, 24, 40, 4), f32)
    P = lambda a: a.ctypes.data_as(rt._c_f)   # noqa: E731
    cam = rt.make_camera(**SYN_CAM)
    tp = rt.temporal_params

    def host(s=P(sums), c=counts.ctypes.data_as(rt._c_i), spp=0, w=40, h=24, g=P(rec), cp=ctypes.byref(cam), gp=P(rec), hp=P(hist2),
             p=None, o=P(hist)):
        return lib.rt_temporal(s, c, spp, w, h, g, cp, gp, hp, ctypes.byref(p) if p is not None else None, o, None, None)

    def device(s=1, c=1, spp=0, w=40, h=24, g=1, cp=ctypes.byref(cam), gp=1, hp=1, p=None, o=2):
        V = ctypes.c_void_p
        return lib.rt_temporal_device(V(s), V(c), spp, w, h, V(g), cp, V(gp), V(hp), ctypes.byref(p) if p is not None else None,
                                      V(o), None, None, None)

    for call in (host, device):
        assert call(s=None) == ERR_ARG and call(g=None) == ERR_ARG and call(o=None) == ERR_ARG
        assert call(w=0) == ERR_ARG and call(h=-1) == ERR_ARG and call(c=None, spp=0) == ERR_ARG
        assert call(cp=None) == ERR_ARG and call(gp=None) == ERR_ARG
        assert call(p=tp(alpha=1.5)) == ERR_ARG and call(p=tp(alpha_moments=1.0001)) == ERR_ARG
        assert call(p=tp(max_history=(1 << 20) + 1)) == ERR_ARG
        for name in ("alpha", "alpha_moments", "sigma_plane", "normal_min"):
            assert call(p=tp(**{name: float("nan")})) == ERR_ARG and call(p=tp(**{name: float("inf")})) == ERR_ARG
        assert b"rt_temporal" in lib.rt_last_error()
        assert call(w=1 << 16, h=1 << 15) == ERR_LIMIT
    assert host(hp=P(hist)) == ERR_ARG and b"history_prev" in lib.rt_last_error()
    assert device(hp=2) == ERR_ARG
    assert host() == 0 and host(p=tp(alpha=1.0, max_history=1 << 20)) == 0
    assert host(cp=None, gp=None, hp=None) == 0   # a first frame needs no previous camera or records
    assert lib.rt_history_create(None, 0, None) == ERR_ARG
    s = rt.Scene.load(rtref.scene_path("cornell"), 8, 8, 1)
    h = ctypes.c_void_p()
    assert lib.rt_history_create(s.handle, 0, ctypes.byref(h)) == ERR_ARG and b"not uploaded" in lib.rt_last_error()
    assert lib.rt_history_push(None, None, None, 1, None, None, None, None) == ERR_ARG
    assert lib.rt_history_lengths(None, None) == ERR_ARG and lib.rt_history_reset(None) == ERR_ARG
    assert lib.rt_history_gbuffer_device(None) is None
    assert lib.rt_accum_reset(None, None) == ERR_ARG
    lib.rt_history_free(None)
    assert lib.rt_abi_version() == 6 and ctypes.sizeof(rt.RtCamera) == 56 and ctypes.sizeof(rt.RtTemporalParams) == 20


# ------------------------------------------------------------------------ CLI usage errors
def test_cli_usage_errors(tmp_path):
    """Reported before anything is rendered (no GPU is touched): RT_TEMPORAL without RT_CAMERAS,
    RT_CAMERAS with a pass mode, and a camera file that is missing, empty or malformed."""
    exe = os.path.join(rtref.ROOT, "raytracing-hw_amd", "rt_solution")
    good = "0 0 6  1 0 0  0 1 0  0 0 -1  0.5 0.5"

    def run(**env_more):
        env = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}
        r = subprocess.run([exe, rtref.scene_path("cornell"), "8", "8", "1", str(tmp_path / "o.ppm")], env=dict(env, **env_more),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and not list(tmp_path.glob("o*.ppm"))
        return r.stderr

    def cams(text):
        (tmp_path / "cams.txt").write_text(text)
        return str(tmp_path / "cams.txt")

    assert "RT_TEMPORAL needs RT_CAMERAS" in run(RT_TEMPORAL="0.2")
    for other in ({"RT_PASS_SPP": "2"}, {"RT_ADAPT": "0.1"}, {"RT_CHECKPOINT": str(tmp_path / "ck")}):
        assert "RT_CAMERAS excludes" in run(RT_CAMERAS=cams(good + "\n"), **other)
    assert "cannot read" in run(RT_CAMERAS=str(tmp_path / "nope.txt"))
    assert "no camera" in run(RT_CAMERAS=cams("# nothing\n\n"))
    for bad in ("0 0 6 1 0 0 0 1 0 0 0 -1 0.5", good + " 7", good.replace("6", "six"), good.replace("0.5 0.5", "0.5 0"),
                good.replace("6", "nan")):
        assert "line 2: expected 14 finite floats" in run(RT_CAMERAS=cams("# a comment\n" + bad + "\n" + good + "\n")), bad
    assert "RT_TEMPORAL must be in 0..1" in run(RT_CAMERAS=cams(good + "\n"), RT_TEMPORAL="1.5")


# ------------------------------------------------------------------------ quality
@pytest.fixture(scope="module")
def gh(tmp_path_factory):
    return twin(tmp_path_factory)


def test_history_of_independent_frames_beats_the_last_frame(rt, oracle, gh):
    """cornell 64 x 64, one view: K = 8 independent 1-sample frames (differences of the CPU oracle's
    sums at 0 .. 8 samples) through rt_temporal with a tiny alpha.  Over valid hit pixels the clamped
    RMSE (test_denoise_guided.py's measure) of the result against a 256-sample render is strictly
    below that of the last frame alone: a pure inequality, no margin."""
    name, w, h, K = "cornell", 64, 64, 8
    arrays = arrays_of(rt, name, w, h)
    rec = host_gbuffer(rt, gh, name, w, h)[0].reshape(h, w, 16)
    cam = {"pos": arrays["cam_pos"], "axes": arrays["cam_axes"], "tan_half_fov": arrays["tan_half_fov"]}
    truth = oracle.render(arrays, 256)[0].reshape(h, w, 3) * (f32(1) / f32(256))
    S = [np.zeros((h, w, 3), f32)] + [oracle.render(arrays, k)[0].reshape(h, w, 3) for k in range(1, K + 1)]
    hist = None
    for k in range(1, K + 1):
        frame = (S[k] - S[k - 1]).astype(f32)
        hist, mean, _ = rt.temporal(frame, 1, rec, cam if hist is not None else None, rec if hist is not None else None, hist,
                                    alpha=1e-6, alpha_moments=1e-6)
    use = (rec.view(np.int32)[..., 7] >= 0) & np.isfinite(truth).all(-1) & np.isfinite(frame).all(-1) & np.isfinite(mean).all(-1)
    assert use.mean() > 0.5 and (hist[0][..., 3][use] == K).all()

    def rmse(x):
        d = np.clip(x[use].astype(np.float64), 0, 4) - np.clip(truth[use].astype(np.float64), 0, 4)
        return float(np.sqrt((d * d).mean()))

    e_last, e_temporal = rmse(frame), rmse(mean)
    print(f"\n{name} {w}x{h}, {K} frames of 1 sample against 256: RMSE last frame {e_last:.4f}, temporal {e_temporal:.4f}")
    assert e_temporal < e_last
