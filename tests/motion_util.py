"""Helpers of the motion-record tests (test_motion.py, test_gpu_motion.py): the numpy float32
restatement of the carry written from include/rt_hw.h ("per-pixel motion records"), the look-up with
motion as a substitution into temporal_util.np_temporal, moved triangle arrays and synthetic records
placed on triangles."""
import numpy as np

from temporal_util import np_temporal

f32 = np.float32
STATIC, CARRIED, LOST = 0, 1, 2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    """rt_vec.h's cross: (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y)."""
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1).astype(f32)


def np_motion(records, tri, tri_prev):
    """The motion records restated from include/rt_hw.h in numpy float32: one elementwise operation
    per step.  Returns (H, W, 8) float32 (state as int bits in word 3)."""
    rec = np.ascontiguousarray(records, f32)
    h, w = rec.shape[:2]
    tri, trp = np.ascontiguousarray(tri, f32).reshape(-1, 12), np.ascontiguousarray(tri_prev, f32).reshape(-1, 12)
    n_tris = len(tri)
    ids = rec.view(np.int32)[..., 7]
    N, P = rec[..., 0:3], rec[..., 12:15]
    miss = (ids < 0) | (ids >= n_tris)
    safe = np.where(miss, 0, ids)
    T, Tp = (tri[safe], trp[safe]) if n_tris else (np.zeros((h, w, 12), f32), np.zeros((h, w, 12), f32))
    same = (bits(T)[..., 0:9] == bits(Tp)[..., 0:9]).all(-1)
    with np.errstate(all="ignore"):
        v0, U, V = T[..., 0:3], T[..., 3:6], T[..., 6:9]
        v0p, Up, Vp = Tp[..., 0:3], Tp[..., 3:6], Tp[..., 6:9]
        e = P - v0
        a, b, c = dot(U, U), dot(U, V), dot(V, V)
        det = a * c - b * b
        solvable = (det > (a * c) * f32(2.0 ** -20)) & np.isfinite(det)
        d, f = dot(U, e), dot(V, e)
        u, v = (c * d - b * f) / det, (a * f - b * d) / det
        dv0, dU, dV = v0p - v0, Up - U, Vp - V
        Pp = P + ((dv0 + u[..., None] * dU) + v[..., None] * dV)
        Wn, Wp = cross(U, V), cross(Up, Vp)
        dn, fn = dot(U, N), dot(V, N)
        al, be = (c * dn - b * fn) / det, (a * fn - b * dn) / det
        ga = dot(Wn, N) / dot(Wn, Wn)
        dW = Wp - Wn
        Np = N + ((al[..., None] * dU + be[..., None] * dV) + ga[..., None] * dW)
        assert Pp.dtype == f32 and Np.dtype == f32 and det.dtype == f32
    static = miss | same
    carried = ~static & solvable & np.isfinite(Pp).all(-1) & np.isfinite(Np).all(-1)
    out = np.zeros((h, w, 8), f32)
    out[..., 0:3] = np.where(static[..., None], P, np.where(carried[..., None], Pp, f32(0)))
    out[..., 4:7] = np.where(static[..., None], N, np.where(carried[..., None], Np, f32(0)))
    out.view(np.int32)[..., 3] = np.where(static, STATIC, np.where(carried, CARRIED, LOST))
    return out


def np_temporal_motion(sums, counts, spp, records, cam_prev, records_prev, history_prev, motion, **params):
    """The look-up with motion as include/rt_hw.h states it: np_temporal with, for a carried pixel,
    (N_prev, P_prev) in (N, P)'s place (t, the ids, albedo and emission are the pixel's own, so steps
    0, 1, 3 and 4 see what they saw), and for every state but 0 and 1 no history (a NaN position
    fails the look-up's first test and is read nowhere else)."""
    rec = np.ascontiguousarray(records, f32).copy()
    mo = np.ascontiguousarray(motion, f32).reshape(rec.shape[0], rec.shape[1], 8)
    state = mo.view(np.int32)[..., 3]
    carried = state == CARRIED
    rec[carried, 0:3], rec[carried, 12:15] = mo[carried, 4:7], mo[carried, 0:3]
    rec[(state != STATIC) & ~carried, 12:15] = np.nan
    return np_temporal(sums, counts, spp, rec, cam_prev, records_prev, history_prev, **params)


def rotation(axis, angle):
    """The float64 rotation matrix about `axis` by `angle` radians (Rodrigues)."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rotated_tris(tri, sel, R, centre):
    """tri with the selected triangles' v0 rotated about `centre` and their U, V rotated (float64,
    rounded once to float32); words 9..11, which the rule does not read, are rotated too."""
    out = np.ascontiguousarray(tri, f32).reshape(-1, 12).copy()
    c = np.asarray(centre, np.float64)
    t = out[sel].astype(np.float64)
    t[:, 0:3] = (t[:, 0:3] - c) @ R.T + c
    for k in (3, 6, 9):
        t[:, k:k + 3] = t[:, k:k + 3] @ R.T
    out[sel] = t.astype(f32)
    return out


def translated_tris(tri, sel, offset):
    """tri with v0 + offset for the selected triangles: one f32 add per component."""
    out = np.ascontiguousarray(tri, f32).reshape(-1, 12).copy()
    out[sel, 0:3] = (out[sel, 0:3] + np.asarray(offset, f32)).astype(f32)
    return out


def records_on(tri, ids, h, w, seed=0, mesh=None):
    """Synthetic first-hit records, (h, w, 16): pixel k sits on triangle ids[k] (a negative id: a
    miss, all-zero words with both ids -1) at random barycentrics, P = v0 + u U + v V in float32, N
    the normalised cross product tilted a little, t the distance from the origin."""
    rng = np.random.default_rng(seed)
    tri = np.ascontiguousarray(tri, f32).reshape(-1, 12)
    ids = np.asarray(ids, np.int32).reshape(h, w)
    hit = (ids >= 0) & (ids < len(tri))
    T = tri[np.where(hit, ids, 0)]
    u = rng.random((h, w), f32) * f32(0.5)
    v = rng.random((h, w), f32) * f32(0.5)
    rec = np.zeros((h, w, 16), f32)
    with np.errstate(all="ignore"):
        P = (T[..., 0:3] + u[..., None] * T[..., 3:6] + v[..., None] * T[..., 6:9]).astype(f32)
        n = cross(T[..., 3:6], T[..., 6:9]) + (rng.random((h, w, 3), f32) - f32(0.5)) * f32(1e-3)
        n = (n / np.sqrt(dot(n, n))[..., None]).astype(f32)
        rec[..., 0:3], rec[..., 12:15] = n, P
        rec[..., 3] = np.sqrt(dot(P, P))
    rec[..., 4:7] = 0.5
    iv = rec.view(np.int32)
    iv[..., 7] = ids
    iv[..., 11] = 0 if mesh is None else np.asarray(mesh, np.int32)[np.where(hit, ids, 0)]
    rec[ids < 0] = 0
    iv[ids < 0, 7] = iv[ids < 0, 11] = -1
    return rec
