"""Caller-made rays for the geoedge fixture (raytracing-hw_amd/scenes.py make_geoedge): rays
built to sit on the edges clean fixtures never reach.  numpy only, fixed
seeds, no GPU.  geoedge_rays(arrays) -> (origins, directions, class index per ray); the
reference's answers to them are tests/golden/geoedge_rays.rtd (ref_harness rays_from).

Also the float32 restatement of the ray and determinant arithmetic (Ray::Ray, the first lines of
Primitive::intersect, in tri_hit_bl's operation order) that the `det` class is aimed with."""
import numpy as np

import rtref

F32 = np.float32
CLASSES = ["axis", "edge", "tie", "t0", "det", "far", "scale", "light", "nonfinite"]
DET_THRESHOLD = F32(float.fromhex("0x1.0c6f7cp-20"))   # the least float above the double 1e-6


def parts():
    """name -> (n, 3, 3) float32 triangles of the geoedge meshes."""
    return {n: t for n, _, t in rtref.scenes_module().geoedge_parts()}


# ------------------------------------------------------------------ float32 restatement
def ray_dir(dd):
    """Ray::Ray's direction: length from 0.f in x, y, z order, then times the reciprocal."""
    dd = np.asarray(dd, F32)
    with np.errstate(all="ignore"):
        m = F32(0)
        m = F32(m + F32(dd[0] * dd[0]))
        m = F32(m + F32(dd[1] * dd[1]))
        m = F32(m + F32(dd[2] * dd[2]))
        m = F32(F32(1) / np.sqrt(m, dtype=F32))
        return np.array([dd[0] * m, dd[1] * m, dd[2] * m], F32)


def det_f32(U, V, dd):
    """det = dot(U, cross(direction, V)) of Primitive::intersect for the ray direction dd
    (un-normalised, as handed to Ray::Ray), every operation rounded to float32, no FMA."""
    d = ray_dir(dd)
    U, V = np.asarray(U, F32), np.asarray(V, F32)
    with np.errstate(all="ignore"):
        p = np.array([F32(d[1] * V[2]) - F32(V[1] * d[2]), F32(d[2] * V[0]) - F32(V[2] * d[0]),
                      F32(d[0] * V[1]) - F32(V[0] * d[1])], F32)
        s = F32(0)
        s = F32(s + F32(U[0] * p[0]))
        s = F32(s + F32(U[1] * p[1]))
        s = F32(s + F32(U[2] * p[2]))
    return s


def _step(f, k):
    """k floats up (down) from the positive float f."""
    return (np.array([f], F32).view(np.uint32) + np.uint32(k)).view(F32)[0] if k >= 0 else \
        (np.array([f], F32).view(np.uint32) - np.uint32(-k)).view(F32)[0]


# ------------------------------------------------------------------ the classes
_NZ = F32(-0.0)


def _axis(arrays, rng):
    node = np.asarray(arrays["node"], F32)
    ext = node[:, 3:6] - node[:, 0:3]
    ok = np.flatnonzero(np.isfinite(node[:, :6]).all(1) & (np.abs(node[:, :6]).max(1) < 64) & (ext.max(1) > 0))
    pick = ok[np.linspace(0, len(ok) - 1, min(12, len(ok))).astype(int)]
    one, two = [], []
    for z in range(3):
        a, b = [k for k in range(3) if k != z]
        for zero in (F32(0.0), _NZ):
            for va, vb in ((1, 0.5), (-1, 0.5), (0.5, -1), (-1, -1)):
                d = np.zeros(3, F32)
                d[z], d[a], d[b] = zero, va, vb
                one.append(d)
        for sign in (1, -1):
            for za, zb in ((F32(0.0), F32(0.0)), (F32(0.0), _NZ), (_NZ, F32(0.0)), (_NZ, _NZ)):
                d = np.zeros(3, F32)
                d[z], d[a], d[b] = sign, za, zb
                two.append(d)
    O, D = [], []
    for n in pick:
        mn, mx = node[n, 0:3], node[n, 3:6]
        c = ((mn.astype(np.float64) + mx) / 2).astype(F32)
        step = np.maximum(mx - mn, F32(0.5))
        pts = [np.array([(mn, mx)[(k >> i) & 1][i] for i in range(3)], F32) for k in range(8)]    # corners
        for i in range(3):                                                                       # slab planes
            for side in (mn, mx):
                p = c.copy()
                p[i] = side[i]
                pts.append(p)
        for i in range(3):                                                                       # edges
            p = np.array([mn[0], mn[1], mn[2]], F32)
            p[i] = c[i]
            pts.append(p)
        pts.append(c)                                                                            # inside
        for i in range(3):                                                                       # outside
            for s in (-2, 2):
                p = c.copy()
                p[i] = c[i] + F32(s) * step[i]
                pts.append(p)
        for p in pts:
            for d in (one[rng.integers(len(one))], one[rng.integers(len(one))], two[rng.integers(len(two))],
                      two[rng.integers(len(two))]):
                O.append(p)
                D.append(d)
    return O, D


def _edge(rng):
    L = rtref.scenes_module().GEOEDGE_LATTICE
    o0, eu, ev = (np.array(L[k], np.float64) for k in ("origin", "eu", "ev"))
    nu, nv = L["nu"], L["nv"]
    O, D = [], []

    def both_sides(p):
        for dz in (2.0, -2.0):
            O.append(p + [0, 0, dz])
            D.append([0, 0, -dz])

    verts = [o0 + eu * i / nu + ev * j / nv for j in range(nv + 1) for i in range(nu + 1)]
    for p in verts:
        both_sides(p)
    for j in range(nv + 1):
        for i in range(nu):
            both_sides(o0 + eu * (i + 0.5) / nu + ev * j / nv)          # horizontal edges
    for j in range(nv):
        for i in range(nu + 1):
            both_sides(o0 + eu * i / nu + ev * (j + 0.5) / nv)          # vertical edges
    for j in range(nv):
        for i in range(nu):
            both_sides(o0 + eu * (i + 0.5) / nu + ev * (j + 0.5) / nv)  # diagonals
    for k, p in enumerate(verts):                                        # 45 degrees, symmetric components
        for a, b, c in ((1, 0, 1), (-1, 0, 1), (0, 1, -1), (1, 1, 1), (-1, 1, -1))[k % 2::2]:
            O.append(p + np.array([a, b, c], np.float64))
            D.append([-a, -b, -c])
    for j in range(nv + 1):                                              # along the edges, in the plane
        O.append(o0 + ev * j / nv - [1.0, 0, 0])
        D.append([1, 0, 0])
    for i in range(nu + 1):
        O.append(o0 + eu * i / nu + [0, 2.0, 0])
        D.append([0, -1, 0])
    for org in ([0.25, 0.75, -1.0], [-0.5, -0.25, -4.5]):                # dyadic origins, aimed at the vertices
        for p in verts:
            O.append(np.array(org))
            D.append(p - org)
    return O, D


def _tie(rng):
    P = parts()
    O, D = [], []
    for name, n in (("DupA", 160), ("CoplanarA", 80), ("CoplanarB", 80)):
        t = P[name].astype(np.float64)
        lo, hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
        for k in range(n):
            target = lo + rng.random(3) * (hi - lo)
            if k % 4 == 0:   # perpendicular, from a dyadic point
                target = np.round(target * 8) / 8
                target[2] = lo[2]
                o = target + [0, 0, (2.0, -1.0)[k % 8 == 0]]
            else:
                o = np.array([rng.uniform(-3.5, 3.5), rng.uniform(-1.8, 1.8), rng.uniform(-3.5, 1.0)])
            O.append(o)
            D.append(target - o)
    return O, D


def _t0(rng):
    P = parts()
    tris = [P["Lattice"][k] for k in (0, 1, 6, 13, 20, 31)] + [P["Single"][0], P["DupA"][2], P["Floor"][3],
                                                             P["Huge"][0], P["Huge2"][0], P["Far"][0], P["Far"][1]]
    O, D = [], []
    for t in tris:
        v0, U, V = t[0].astype(np.float64), t[1].astype(np.float64) - t[0], t[2].astype(np.float64) - t[0]
        n = np.cross(U, V)
        n /= np.abs(n).max()
        big = np.abs(U).max() > 1e6
        scale = 1.0 if not big else np.abs(U).max() / 4
        for p in (v0 + 0.25 * U + 0.25 * V, v0 + 0.5 * U, v0 + 0.5 * U + 0.5 * V, v0):   # interior, two edges, vertex
            for d in (n, -n, n * scale + U, -n * scale + V, U, -U, V, U + V, U - V):
                O.append(p)
                D.append(d)
    return O, D


def _det(rng):
    """Grazing rays at the lattice's first triangle; |det| (det_f32) sweeps [0.5e-6, 2e-6] on
    both signs, plus the floats next to the threshold where bisection on the slope finds one."""
    t = parts()["Lattice"][0]
    v0, U, V = t[0], t[1] - t[0], t[2] - t[0]
    c = (t[0].astype(np.float64) + t[1] + t[2]) / 3
    nz = float(np.cross(U.astype(np.float64), V)[2])

    def dd_of(s):
        return np.array([1.0, 0.3125, s], F32)

    O, D = [], []
    for sign in (1.0, -1.0):
        for target in np.geomspace(0.5e-6, 2e-6, 40):
            s = sign * target / abs(nz) * np.sqrt(1 + 0.3125 ** 2)
            D.append(dd_of(s))
        # the threshold and its neighbours: least slope s (as a float32) whose |det| reaches the target
        for k in (-1, 0, 1):
            want = _step(DET_THRESHOLD, k)
            lo = np.array([1e-6], F32).view(np.uint32)[0]
            hi = np.array([1e-4], F32).view(np.uint32)[0]
            while lo < hi:
                mid = (int(lo) + int(hi)) // 2
                s = np.array([mid], np.uint32).view(F32)[0]
                if abs(det_f32(U, V, dd_of(sign * s))) >= want:
                    hi = mid
                else:
                    lo = mid + 1
            s = np.array([lo], np.uint32).view(F32)[0]
            if abs(det_f32(U, V, dd_of(sign * s))) == want:
                D.append(dd_of(sign * s))
    for d in D:
        O.append((c - 1.5 * d.astype(np.float64)).astype(F32))
    return O, D


def _far(rng):
    sc = rtref.scenes_module()
    O, D = [], []
    centre = np.array([0.0, 0.0, -2.0])
    # origins farther than 1e9 from the room, aimed at it
    for k, dist in enumerate((1.5e9, 2e9, 1e10, 1e12, 1e15, 1e20)):
        for a in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0.6, 0.64, 0.48], [-0.36, 0.48, -0.8]):
            o = centre + dist * np.array(a, np.float64)
            O.append(o)
            D.append(-np.array(a, np.float64))
    # entry distances within a few floats of 1e9 (64 apart there), along the axes: the cull's own edge
    for axis in range(3):
        for sign in (1.0, -1.0):
            for k in range(-4, 5):
                o = np.array([0.5, 0.25, -2.0])
                o[axis] = sign * (1e9 + 64.0 * k)
                d = np.zeros(3)
                d[axis] = -sign
                O.append(o)
                D.append(d)
    # the only hit lies beyond 1e9: from beside the room at the far mesh
    for k in range(16):
        O.append([10.0 + k, rng.uniform(100, 4000), rng.uniform(-4000, 4000)])
        D.append([1, 0, 0])
    # at the far mesh from 1e4 .. 2e9 in front of it, and from behind
    for k, back in enumerate((1e4, 1e6, 1.5e8, 2.5e8, 5e8, 9e8, 1.2e9, 2e9)):
        for y, z in ((0, 0), (1024, -2048), (-4096, 4096), (100, 4000)):
            O.append([sc.GEOEDGE_FAR_X - back, y, z])
            D.append([1, 0, 0])
            O.append([sc.GEOEDGE_FAR_X + back, y, z])
            D.append([-1, 0.0, 0])
    # against the 1e15 triangle (plane z = -60) and the 2^63 one (plane z = -70), near and far
    for h in (1.0, 1e3, 2e8, 5e8, 9.9e8, 1.1e9, 1e12, 1e20):
        for x, y in ((1e3, 1e3), (3e14, 3e14), (1e14, 8e14), (6e14, 6e14)):
            O.append([x, y, -60.0 + h])
            D.append([0, 0, -1])
            O.append([x + h * 0.6, y, -60.0 - h * 0.8])
            D.append([-0.6, 0, 0.8])
    e2 = sc.GEOEDGE_HUGE2_EDGE
    for h in (1.0, 64.0, 1e6, 3e8, 1e12):
        for x, y in ((1e3, 1e3), (e2 / 4, e2 / 4), (e2 / 2, e2 / 4), (e2 / 8, e2 / 2)):
            for dz in (1.0, 0.51, 0.5, 0.49):   # det = 2^126 dz: above, at and below rcp_ieee's 2^125
                d = np.array([np.sqrt(1 - dz * dz), 0, -dz])
                O.append(np.array([x, y, -70.0]) - h * d)
                D.append(d)
    return O, D


def _scale(rng, arrays):
    sc = rtref.scenes_module()
    cam = np.array([0.0, 0.0, sc.GEOEDGE_CAMERA_Z])
    O, D = [], []
    for k in range(32):
        base = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.4, 0.4), -1.0])
        for length in (1e-20, 1e20):
            O.append(cam)
            D.append((base * length).astype(F32))
        d = base.astype(F32)
        d[k % 2] = F32((1e-40, -1e-40, 1e-45, 3e-39)[k % 4])   # a denormal component: its reciprocal overflows
        O.append(cam)
        D.append(d)
    tiny = sc.GEOEDGE_TINY
    for x, y in ((0, 0), (0.25, 0.25), (0.5, 0.5), (1, 0), (0.75, 0.5), (2, 2)):
        for oz, dz in ((1.0, -1.0), (tiny, -1.0), (-1.0, 1.0)):
            O.append(np.array([x * tiny, y * tiny, oz], F32))
            D.append([0, 0, dz])
    for k in range(8):
        o = np.array([rng.uniform(-3, 3), rng.uniform(-1.5, 1.5), rng.uniform(-1, 1)])
        O.append(o)
        D.append(np.array([0.25 * tiny, 0.25 * tiny, 0.0]) - o)
    return O, D


def _light(rng):
    P = parts()
    lt = P["Light"].reshape(-1, 3).astype(np.float64)
    lo, hi = lt.min(0), lt.max(0)
    y = lo[1]
    O, D = [], []
    for k in range(12):     # from points on the ordinary light: leaving, in its plane, upwards
        p = np.array([rng.uniform(lo[0], hi[0]), y, rng.uniform(lo[2], hi[2])])
        for d in ([0, -1, 0], [rng.uniform(-1, 1), -rng.uniform(0.1, 1), rng.uniform(-1, 1)], [1, 0, 0], [0.6, 0, -0.8],
                  [0, 1, 0]):
            O.append(p)
            D.append(d)
    for t in P["DegenLight"]:   # from points on the zero-area light
        for p in (t[0], (t[0].astype(np.float64) + t[1]) / 2, t[2]):
            for d in ([0, -1, 0], [1, 0, 0], [rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1)],
                      np.array([0.0, y, -2.0]) - p):
                O.append(np.asarray(p, np.float64))
                D.append(d)
    for o in ([3.0, y, -2.0], [-3.0, y, -2.5], [0.0, y, 1.0], [0.5, y, -5.0]):   # edge-on: cosine 0
        for tx, tz in ((0.0, -2.0), (0.5, -1.5), (-1.0, -3.0)):
            O.append(np.array(o))
            D.append(np.array([tx, y, tz]) - o)
    for o in ([0.0, 0.0, 0.0], [0.25, -1.0, -2.0], [-2.0, 0.5, -1.0]):            # through its vertices
        for vx in (lo[0], hi[0]):
            for vz in (lo[2], hi[2]):
                O.append(np.array(o))
                D.append(np.array([vx, y, vz]) - o)
    for k in range(24):     # from below: towards the light and away from every light
        o = np.array([rng.uniform(-3, 3), rng.uniform(-1.8, 1.0), rng.uniform(-5, 1)])
        O.append(o)
        D.append(np.array([rng.uniform(lo[0], hi[0]), y, rng.uniform(lo[2], hi[2])]) - o)
        O.append(o)
        D.append([rng.uniform(-1, 1), -1.0, rng.uniform(-1, 1)])
    return O, D


def _nonfinite():
    inf, nan = np.inf, np.nan
    o = [0.0, 0.0, 1.0]
    rays = [(o, [0, 0, 0]), ([1, 1, -2], [0, 0, 0]), ([0, 0, -3], [0.0, -0.0, 0.0]), ([100, 0, 0], [-0.0, -0.0, -0.0]),
            (o, [inf, 0, -1]), (o, [0, -inf, -1]), (o, [0.1, 0.1, -inf]), (o, [inf, inf, -1]), (o, [-inf, 1, inf]),
            ([1, 0, 0], [inf, inf, inf]),
            ([nan, 0, 1], [0, 0, -1]), ([0, nan, 1], [0.1, 0, -1]), ([0, 0, nan], [0, 0.1, -1]), ([nan, nan, 1], [0, 0, -1]),
            ([nan, nan, nan], [1, 1, 1]), ([nan, 0, 0], [1, 0, 0])]
    return [r[0] for r in rays], [r[1] for r in rays]


def geoedge_rays(arrays):
    """(origins (n, 3), directions (n, 3), class index (n,)) for the scene arrays of geoedge
    (the `axis` class reads boxes from arrays["node"])."""
    rng = np.random.default_rng(20261021)
    made = [_axis(arrays, rng), _edge(rng), _tie(rng), _t0(rng), _det(rng), _far(rng), _scale(rng, arrays), _light(rng),
            _nonfinite()]
    O, D, C = [], [], []
    with np.errstate(over="ignore"):
        for k, (o, d) in enumerate(made):
            assert len(o) == len(d)
            O += [np.asarray(x, np.float64).astype(F32) for x in o]
            D += [np.asarray(x, np.float64).astype(F32) if np.asarray(x).dtype != F32 else np.asarray(x) for x in d]
            C += [k] * len(o)
    return np.array(O, F32).reshape(-1, 3), np.array(D, F32).reshape(-1, 3), np.array(C, np.int32)


def partner_triangles(arrays):
    """Indices (in the scene's triangle order) of triangles that have an exact duplicate or a
    coplanar overlapping partner: the Dup and Coplanar meshes."""
    P = parts()
    tri = np.asarray(arrays["tri"], F32)
    want = np.concatenate([P[n] for n in ("DupA", "DupB", "CoplanarA", "CoplanarB")])
    rec = np.concatenate([want[:, 0], want[:, 1] - want[:, 0], want[:, 2] - want[:, 0]], 1).astype(F32)
    return np.flatnonzero((tri[:, None, :9].view(np.uint32) == rec[None].view(np.uint32)).all(2).any(1))


def edge_mesh_triangles(arrays):
    """Indices of the triangles of every mesh but the room's six walls and the ordinary light."""
    P = parts()
    tri = np.asarray(arrays["tri"], F32)
    room = np.concatenate([P[n] for n in ("Floor", "Ceiling", "Back", "Left", "Right", "Front", "Light")])
    rec = np.concatenate([room[:, 0], room[:, 1] - room[:, 0], room[:, 2] - room[:, 0]], 1).astype(F32)
    is_room = (tri[:, None, :9].view(np.uint32) == rec[None].view(np.uint32)).all(2).any(1)
    return np.flatnonzero(~is_room)


# ------------------------------------------------------------------ the comparison
def _explain(rays_in, bad, what):
    k = np.flatnonzero(bad)
    cls = sorted({CLASSES[c] for c in rays_in["cls"][k]})
    return f"{what}: {len(k)} rays differ, classes {cls}, first {k[:8].tolist()}"


def check_rays(rays_in, gold, out_f, out_i, label):
    """Every field the ray entries return, against the golden, under rtref.same."""
    hit = gold["hit"].astype(bool)
    fields = [("hit", out_i[:, 0], gold["hit"]), ("object_id", out_i[:, 1], gold["object_id"]),
              ("t", out_f[:, 0], gold["t"]), ("u", out_f[:, 1], gold["uv"][:, 0]), ("v", out_f[:, 2], gold["uv"][:, 1]),
              ("light_pdf", out_f[:, 3], gold["light_pdf"]), ("n_aabb", out_i[:, 2], gold["n_aabb"]),
              ("n_tri", out_i[:, 3], gold["n_tri"]), ("n_light_aabb", out_i[:, 4], gold["n_light_aabb"]),
              ("n_light_tri", out_i[:, 5], gold["n_light_tri"])]
    assert len(out_f) == len(hit)
    for name, got, want in fields:
        bad = ~rtref.same(got, want)
        assert not bad.any(), _explain(rays_in, bad, f"{label} {name}")
