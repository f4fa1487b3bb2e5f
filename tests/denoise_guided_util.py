"""Helper of the variance-guided denoiser's tests (test_denoise_guided.py, test_gpu_denoise_guided.py):
the numpy float32 restatement of rt_denoise_guided, written from the rule in include/rt_hw.h, one
elementwise operation per step, taps in the stated order."""
import numpy as np

f32 = np.float32
GUIDED_DEFAULTS = dict(iterations=5, sigma_var=2.0, sigma_plane=0.02, normal_power_log2=6, firefly=8.0)   # include/rt_hw.h


def _tap(arr, dy, dx):
    """(arr at p + (dx, dy) with the index clamped into the frame, whether the tap is inside)."""
    h, w = arr.shape[:2]
    ys, xs = np.arange(h) + dy, np.arange(w) + dx
    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    return arr[np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]], inside


def _lum(L):
    return (f32(0.2126) * L[..., 0] + f32(0.7152) * L[..., 1]) + f32(0.0722) * L[..., 2]


def np_denoise_guided(sums, counts, spp, records, variance=None, iterations=5, sigma_var=2.0, sigma_plane=0.02,
                      normal_power_log2=6, firefly=8.0):
    """Returns (out_mean (h, w, 3), out_variance (h, w)).  counts None: one spp.  The parameters are
    the resolved ones (no defaults are substituted here, but firefly < 0 switches the clamp off)."""
    h, w = sums.shape[:2]
    S = np.ascontiguousarray(sums, f32)
    n = np.full((h, w), spp, np.int32) if counts is None else np.asarray(counts, np.int32).reshape(h, w)
    rec = np.ascontiguousarray(records, f32).reshape(h, w, 16)
    ids = rec.view(np.int32)
    N, t, al, E, P = rec[..., 0:3], rec[..., 3], rec[..., 4:7], rec[..., 8:11], rec[..., 12:15]
    one, zero = f32(1), f32(0)
    with np.errstate(all="ignore"):
        rn = np.where(n > 0, one / np.maximum(n, 1).astype(f32), zero).astype(f32)
        m = S * rn[..., None]
        if iterations == 0:
            return m, np.zeros((h, w), f32)
        # 1. prepare
        af = np.where(al > f32(1e-3), al, f32(1e-3)).astype(f32)
        L = (m - E) / af
        fin = np.isfinite(m).all(-1) & np.isfinite(L).all(-1)
        hit = ids[..., 7] >= 0
        kind = np.where(~hit, 0, np.where(n <= 0, 2, np.where(fin, 1, 0)))
        kind = np.where(hit & ~(al > f32(1e-3)).any(-1), 0, kind)
        L = np.where((kind == 1)[..., None], L, zero).astype(f32)
        plane_den = f32(sigma_plane) * t

        def geo_terms(dy, dx):
            """rt_denoise's nd and wp for every centre and its tap at (dx, dy)."""
            Nq, _ = _tap(N, dy, dx)
            Pq, _ = _tap(P, dy, dx)
            nd = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
            nd = np.where(nd > 0, nd, zero)
            for _ in range(normal_power_log2):
                nd = nd * nd
            e = Pq - P
            pd = (N[..., 0] * e[..., 0] + N[..., 1] * e[..., 1]) + N[..., 2] * e[..., 2]
            pr = pd / plane_den
            wp = one / (one + pr * pr)
            return nd.astype(f32), wp.astype(f32)

        # 2. firefly clamp
        if not firefly < 0:
            sg, sl = np.zeros((h, w), f32), np.zeros((h, w), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if dx == 0 and dy == 0:
                        continue
                    nd, wp = geo_terms(dy, dx)
                    g = nd * wp
                    Lq, inside = _tap(L, dy, dx)
                    kq, _ = _tap(kind, dy, dx)
                    use = inside & (kq == 1) & (kind == 1) & (g > 0)
                    sg = np.where(use, sg + g, sg)
                    sl = np.where(use, sl + g * _lum(Lq), sl)
            mean = sl / sg
            cap = f32(firefly) * np.where(mean > 0, mean, zero)
            lc = _lum(L)
            scale = cap / lc
            clamp = (kind == 1) & (sg > 0) & (lc > cap)
            L = np.where(clamp[..., None], L * scale[..., None], L).astype(f32)
        # 3. variance
        if variance is not None:
            vin = np.ascontiguousarray(variance, f32).reshape(h, w)
            V = np.where((kind == 1) & np.isfinite(vin) & (vin > 0), vin, zero).astype(f32)
        else:
            sg, used = np.zeros((h, w), f32), np.zeros((h, w), np.int32)
            s1, s2 = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    nd, wp = geo_terms(dy, dx)
                    g = nd * wp
                    Lq, inside = _tap(L, dy, dx)
                    kq, _ = _tap(kind, dy, dx)
                    use = inside & (kq == 1) & (kind == 1) & (g > 0)
                    sg = np.where(use, sg + g, sg)
                    s1 = np.where(use[..., None], s1 + g[..., None] * Lq, s1)
                    s2 = np.where(use[..., None], s2 + g[..., None] * (Lq * Lq), s2)
                    used = used + use
            mu = s1 / sg[..., None]
            var = s2 / sg[..., None] - mu * mu
            var = np.where(var > 0, var, zero)
            V = (var[..., 0] + var[..., 1]) + var[..., 2]
            V = np.where((used >= 2) & np.isfinite(V), V, zero).astype(f32)
        # 4. levels
        b = [f32(0.375), f32(0.25), f32(0.0625)]
        c = [f32(0.5), f32(0.25)]
        sv2 = f32(sigma_var) * f32(sigma_var)
        for k in range(iterations):
            s = 1 << k
            gw, gv = np.zeros((h, w), f32), np.zeros((h, w), f32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    Vq, inside = _tap(V, dy, dx)
                    kq, _ = _tap(kind, dy, dx)
                    use = inside & (kq == 1)
                    cw = c[abs(dx)] * c[abs(dy)]
                    gw = np.where(use, gw + cw, gw)
                    gv = np.where(use, gv + cw * Vq, gv)
            vbar = np.where(gw > 0, gv / gw, zero)
            cden = sv2 * vbar + f32(1e-8)
            assert cden.dtype == f32
            sw, sL, sV = np.zeros((h, w), f32), np.zeros((h, w, 3), f32), np.zeros((h, w), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    nd, wp = geo_terms(dy * s, dx * s)
                    Lq, inside = _tap(L, dy * s, dx * s)
                    Vq, _ = _tap(V, dy * s, dx * s)
                    kq, _ = _tap(kind, dy * s, dx * s)
                    use = inside & (kq == 1) & (kind != 0)
                    hw = b[abs(dx)] * b[abs(dy)]
                    dl = Lq - L
                    d2 = (dl[..., 0] * dl[..., 0] + dl[..., 1] * dl[..., 1]) + dl[..., 2] * dl[..., 2]
                    wc = np.where(kind == 1, one / (one + d2 / cden), one)
                    wt = ((hw * nd) * wp) * wc
                    assert wt.dtype == f32
                    use = use & (wt > 0)
                    sw = np.where(use, sw + wt, sw)
                    sL = np.where(use[..., None], sL + wt[..., None] * Lq, sL)
                    sV = np.where(use, sV + (wt * wt) * Vq, sV)
            quo = sL / sw[..., None]
            nv = sV / (sw * sw)
            active, some = kind != 0, sw > 0
            good = active & some & np.isfinite(quo).all(-1)
            empty = active & ~some
            L = np.where(good[..., None], quo, np.where(empty[..., None], zero, L)).astype(f32)
            V = np.where(good & np.isfinite(nv), nv, np.where(empty, zero, V)).astype(f32)
            kind = np.where(good, 1, kind)
        # 5. resolve
        out = np.where((kind == 0)[..., None], m, L * af + E)
        out_v = np.where(kind == 1, V, zero).astype(f32)
    assert out.dtype == f32
    return out, out_v
