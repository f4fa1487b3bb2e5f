"""Helpers of the temporal-history tests (test_temporal.py, test_gpu_temporal.py): the numpy float32
restatement of the step written from include/rt_hw.h, cameras, and the exact plane frames."""
import numpy as np

f32 = np.float32
DEFAULTS = dict(alpha=0.2, alpha_moments=0.2, sigma_plane=0.02, normal_min=0.9, max_history=65536)   # include/rt_hw.h


def camera(pos=(0, 0, 0), axes=((1, 0, 0), (0, 1, 0), (0, 0, 1)), tan=(1, 1)):
    return {"pos": np.asarray(pos, f32), "axes": np.asarray(axes, f32).reshape(3, 3), "tan_half_fov": np.asarray(tan, f32)}


def rotated(cam, yaw):
    """The camera turned by `yaw` radians about the world's y axis."""
    c, s = np.cos(yaw), np.sin(yaw)
    rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return {"pos": cam["pos"].copy(), "axes": (np.asarray(cam["axes"], np.float64) @ rot.T).astype(f32),
            "tan_half_fov": cam["tan_half_fov"].copy()}


def moved(cam, delta):
    return {"pos": (np.asarray(cam["pos"], f32) + np.asarray(delta, f32)).astype(f32), "axes": cam["axes"].copy(),
            "tan_half_fov": cam["tan_half_fov"].copy()}


def np_temporal(sums, counts, spp, records, cam_prev=None, records_prev=None, history_prev=None, alpha=0.2, alpha_moments=0.2,
                sigma_plane=0.02, normal_min=0.9, max_history=65536):
    """The step restated from include/rt_hw.h in numpy float32: one elementwise operation per step,
    taps in the stated order.  counts None: one spp.  Returns (history (3, h, w, 4), mean, variance)."""
    h, w = sums.shape[:2]
    S = np.ascontiguousarray(sums, f32)
    n = np.full((h, w), spp, np.int32) if counts is None else np.asarray(counts, np.int32).reshape(h, w)
    rec = np.ascontiguousarray(records, f32).reshape(h, w, 16)
    ids = rec.view(np.int32)
    N, t, al, E, P = rec[..., 0:3], rec[..., 3], rec[..., 4:7], rec[..., 8:11], rec[..., 12:15]
    mesh = ids[..., 11]
    one, zero, half = f32(1), f32(0), f32(0.5)
    alpha, alpha_moments, sigma_plane, normal_min = f32(alpha), f32(alpha_moments), f32(sigma_plane), f32(normal_min)
    maxh = f32(max_history)
    with np.errstate(all="ignore"):
        rn = np.where(n > 0, one / np.maximum(n, 1).astype(f32), zero).astype(f32)
        m = S * rn[..., None]
        af = np.where(al > f32(1e-3), al, f32(1e-3)).astype(f32)
        L = (m - E) / af
        fin = np.isfinite(m).all(-1) & np.isfinite(L).all(-1)
        kind = np.where(ids[..., 7] < 0, 0, np.where(n <= 0, 2, np.where(fin, 1, 0)))
        L = np.where((kind == 1)[..., None], L, zero).astype(f32)
        have = np.zeros((h, w), bool)
        Lh, M1h, M2h, Nh = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32), np.zeros((h, w), f32)
        if history_prev is not None:
            hp = np.ascontiguousarray(history_prev, f32).reshape(3, h, w, 4)
            rp = np.ascontiguousarray(records_prev, f32).reshape(h, w, 16)
            ip = rp.view(np.int32)
            pos = np.asarray(cam_prev["pos"], f32)
            R, U, F = np.asarray(cam_prev["axes"], f32).reshape(3, 3)
            tan = np.asarray(cam_prev["tan_half_fov"], f32)
            v = P - pos
            z = (v[..., 0] * F[0] + v[..., 1] * F[1]) + v[..., 2] * F[2]
            cx = ((v[..., 0] * R[0] + v[..., 1] * R[1]) + v[..., 2] * R[2]) / z
            cy = ((v[..., 0] * U[0] + v[..., 1] * U[1]) + v[..., 2] * U[2]) / z
            fx = ((cx / tan[0] + one) * half) * f32(w) - half
            fy = ((one - cy / tan[1]) * half) * f32(h) - half
            ok = (z > 0) & (fx > -1) & (fx < f32(w)) & (fy > -1) & (fy < f32(h))
            fxs, fys = np.where(ok, fx, zero).astype(f32), np.where(ok, fy, zero).astype(f32)
            x0 = fxs.astype(np.int32)
            x0 = np.where(x0.astype(f32) > fxs, x0 - 1, x0)
            y0 = fys.astype(np.int32)
            y0 = np.where(y0.astype(f32) > fys, y0 - 1, y0)
            wx, wy = fxs - x0.astype(f32), fys - y0.astype(f32)
            assert wx.dtype == f32
            sb = np.zeros((h, w), f32)
            sL, sM1, sM2, sN = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32), np.zeros((h, w), f32)
            plane_den = sigma_plane * t
            for dy in (0, 1):
                for dx in (0, 1):
                    qx, qy = x0 + dx, y0 + dy
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    ix, iy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    b = (wx if dx else one - wx) * (wy if dy else one - wy)
                    h0, h1, h2 = hp[0][iy, ix], hp[1][iy, ix], hp[2][iy, ix]
                    Nq, Pq, mq = rp[iy, ix, 0:3], rp[iy, ix, 12:15], ip[iy, ix, 11]
                    nd = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                    e = Pq - P
                    pd = (N[..., 0] * e[..., 0] + N[..., 1] * e[..., 1]) + N[..., 2] * e[..., 2]
                    use = ok & inside & (b > 0) & (h0[..., 3] > 0) & (mq >= 0) & (mq == mesh) & (nd >= normal_min) & \
                        (np.abs(pd) <= plane_den)
                    assert b.dtype == f32 and pd.dtype == f32
                    sb = np.where(use, sb + b, sb)
                    sL = np.where(use[..., None], sL + b[..., None] * h0[..., 0:3], sL)
                    sN = np.where(use, sN + b * h0[..., 3], sN)
                    sM1 = np.where(use[..., None], sM1 + b[..., None] * h1[..., 0:3], sM1)
                    sM2 = np.where(use[..., None], sM2 + b[..., None] * h2[..., 0:3], sM2)
            Lh, Nh, M1h, M2h = sL / sb[..., None], sN / sb, sM1 / sb[..., None], sM2 / sb[..., None]
            have = (sb > 0) & np.isfinite(Lh).all(-1) & np.isfinite(Nh) & np.isfinite(M1h).all(-1) & np.isfinite(M2h).all(-1)
        # integrate
        up = Nh + one
        Nv = np.where(up < maxh, up, maxh).astype(f32)
        rN = one / Nv
        a = np.where(alpha > rN, alpha, rN).astype(f32)
        am = np.where(alpha_moments > rN, alpha_moments, rN).astype(f32)
        Lv = Lh + a[..., None] * (L - Lh)
        M1v = M1h + am[..., None] * (L - M1h)
        M2v = M2h + am[..., None] * (L * L - M2h)
        good = have & np.isfinite(Lv).all(-1) & np.isfinite(M1v).all(-1) & np.isfinite(M2v).all(-1)
        valid, fill = kind == 1, kind == 2
        vh, vn, fh = valid & good, valid & ~good, fill & have

        def pick(hist_value, fresh_value, fill_value):
            c = lambda mask: mask[..., None] if np.ndim(hist_value) == 3 else mask   # noqa: E731
            return np.where(c(vh), hist_value, np.where(c(vn), fresh_value, np.where(c(fh), fill_value, zero))).astype(f32)

        N1 = pick(Nv, np.ones((h, w), f32), Nh)
        L1, M1, M2 = pick(Lv, L, Lh), pick(M1v, L, M1h), pick(M2v, L * L, M2h)
        hist = np.zeros((3, h, w, 4), f32)
        hist[0, ..., 0:3], hist[0, ..., 3], hist[1, ..., 0:3], hist[2, ..., 0:3] = L1, N1, M1, M2
        mean = np.where((kind == 0)[..., None], m, L1 * af + E).astype(f32)
        a1 = np.where(alpha > one / N1, alpha, one / N1).astype(f32)
        vc = M2 - M1 * M1
        vc = np.where(vc > 0, vc, zero)
        V = ((vc[..., 0] + vc[..., 1]) + vc[..., 2]) * a1
        var = np.where((N1 >= 2) & np.isfinite(V), V, zero).astype(f32)
    assert hist.dtype == f32 and mean.dtype == f32 and var.dtype == f32
    return hist, mean, var


def plane_frame(w=16, h=8, value=1.0, seed=0, mesh=3):
    """The exact case's frame: camera at the origin, identity axes, tangents 1; every pixel sees the
    plane z = 4 at P = (tx * 4, ty * 4, 4) with tx, ty the camera ray's, normal (0, 0, -1), albedo 0.5,
    one mesh id, 1 sample.  The radiance is `value` plus a per-pixel pattern.  Returns (sums, records)."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    tx = (f32(2) * (i + f32(0.5)) / f32(w) - 1) * f32(1)
    ty = -(f32(2) * (j + f32(0.5)) / f32(h) - 1) * f32(1)
    rec = np.zeros((h, w, 16), f32)
    rec[..., 2] = -1
    rec[..., 12], rec[..., 13], rec[..., 14] = tx * f32(4), ty * f32(4), 4
    rec[..., 3] = np.sqrt(rec[..., 12] ** 2 + rec[..., 13] ** 2 + f32(16)).astype(f32)
    rec[..., 4:7] = 0.5
    ids = rec.view(np.int32)
    ids[..., 7] = 5
    ids[..., 11] = mesh
    sums = (f32(value) + rng.integers(0, 64, (h, w, 3)).astype(f32) / f32(64)).astype(f32)
    return sums, rec
