"""Caller-made shading frames for the shadeedge chain: inputs of scene_sample /
scene_pdf (rt_path.h) built to sit where those functions are singular, after tests/geoedge_util.py.
numpy only, fixed seeds, no GPU.  shadeedge_frames(arrays) -> dict(frame, seed, warm, cls); the
reference's answers to them are tests/golden/shadeedge_<scene>.rtd (ref_harness samplers_from).

Also the float32 restatement of the engine and of the draws' arithmetic (rng_next, rng_canonical,
rng_uniform_m11, mixture_pick's s) that the `branch` class is aimed with: a seed is found by
stepping the engine backwards from the output wanted.  Each aim is a predicate (AIMS) over
kh_sampler_trace's record of the host build, which tests/test_shadeedge.py re-evaluates."""
import numpy as np

import rtref

F32 = np.float32
CLASSES = ["axis", "antipode", "rough", "branch", "light", "warm", "nonfinite", "generic"]
SCENES = ["cornell", "geoedge", "practice6_1", "cornell_nolights"]
R2_LIMIT = F32(0.03)   # kRoughness2Limit

M = 2147483647
A = 48271
A_INV = pow(A, -1, M)
U_MAX = F32(1) - F32(2.0 ** -23)       # the largest uniform(-1, 1): 2 * nextafter(1, 0) - 1
ULP1 = F32(2.0 ** -23)


def scene_file(scene):
    """The committed scene a shadeedge set is answered on, and whether its lights are dropped."""
    return ("cornell", True) if scene == "cornell_nolights" else (scene, False)


def scene_arrays(rt, scene):
    """The reference's arrays of a shadeedge scene (cornell_nolights: cornell with an empty light list)."""
    name, nolights = scene_file(scene)
    a = rtref.ref_arrays(rt, name, 64, 64, 1)
    if nolights:
        a = dict(a)
        a["light"] = np.zeros((0, 16), np.float32)
        a["light_node"] = np.zeros((0, 8), np.float32)
    return a


# ------------------------------------------------------------------ float32 restatement of the draws
def rng_step(x, k=1):
    return (np.asarray(x, np.uint64) * np.uint64(pow(A, k, M))) % np.uint64(M)


def rng_back(x, k=1):
    """The state k outputs before the output x (the inverse of rng_next's multiplier)."""
    return (np.asarray(x, np.uint64) * np.uint64(pow(A_INV, k, M))) % np.uint64(M)


def canonical(x):
    s = (np.asarray(x, np.uint64) - np.uint64(1)).astype(F32)
    v = s / F32(2147483648.0)
    return np.where(v >= F32(1), F32(1) - F32(2.0 ** -24), v).astype(F32)


def uniform(x):
    return canonical(x) * F32(2) + F32(-1)


def mixture_s(x, lights):
    s = (uniform(x) + F32(1)) * F32(3) * F32(0.5)
    return s if lights else (s / F32(1.5)).astype(F32)


def branch_of(s):
    return np.where(s <= F32(1), 0, np.where(s <= F32(2), 1, 2))


# Each aim: a predicate over kh_sampler_trace's record (s, the pick's uniform, u, v; the sampler, the
# disc pairs rejected) and whether it needs a light list.
AIMS = {
    "mix_below_1": (lambda t: (t["s"] < 1) & (t["s"] >= F32(1) - 4 * ULP1), False),
    "mix_on_1": (lambda t: t["s"] == 1, False),
    "mix_above_1": (lambda t: (t["s"] > 1) & (t["s"] <= F32(1) + 4 * ULP1), False),
    "mix_below_2": (lambda t: (t["s"] < 2) & (t["s"] >= F32(2) - 8 * ULP1), False),
    "mix_on_2": (lambda t: t["s"] == 2, True),
    "mix_above_2": (lambda t: (t["s"] > 2) & (t["s"] <= F32(2) + 8 * ULP1), True),
    "pick_largest": (lambda t: (t["sampler"] == 2) & (t["pick"] == U_MAX), True),
    "fold_below": (lambda t: (t["sampler"] == 2) & (t["u"] + t["v"] < 1) & (t["u"] + t["v"] >= F32(1) - 4 * ULP1), True),
    "fold_on": (lambda t: (t["sampler"] == 2) & (t["u"] + t["v"] == 1), True),
    "fold_above": (lambda t: (t["sampler"] == 2) & (t["u"] + t["v"] > 1) & (t["u"] + t["v"] <= F32(1) + 4 * ULP1), True),
    "disc_twice": (lambda t: (t["sampler"] == 1) & (t["rejected"] >= 2), False),
}
AIM_FRAMES = 8


def _trace(seed, lights):
    """The restatement's own record for cold seeds, in kh_sampler_trace's fields."""
    x1 = rng_step(seed)
    s = mixture_s(x1, lights)
    b = branch_of(s)
    x2, x3, x4, x5 = (rng_step(seed, k) for k in (2, 3, 4, 5))
    rej1 = (uniform(x2) * uniform(x2) + uniform(x3) * uniform(x3)) > F32(1)
    rej2 = (uniform(x4) * uniform(x4) + uniform(x5) * uniform(x5)) > F32(1)
    return {"s": s, "sampler": b, "pick": uniform(x2), "u": ((uniform(x3) + F32(1)) / F32(2)).astype(F32),
            "v": ((uniform(x4) + F32(1)) / F32(2)).astype(F32), "rejected": np.where(rej1 & rej2, 2, rej1.astype(int))}


def _spread(x, n):
    x = np.unique(np.asarray(x, np.uint64))
    return x[np.linspace(0, len(x) - 1, min(n, len(x))).astype(int)]


def aimed_seeds(lights):
    """aim -> up to AIM_FRAMES seeds (cold cache), found backwards from the outputs wanted."""
    out = {}
    # the mixture draw: outputs around the x whose s is 1 and 2
    for edge, c in ((1, 1 / 3 if lights else 0.5), (2, 2 / 3 if lights else 1.0)):
        x = np.arange(int(c * 2 ** 31) - 40000, int(c * 2 ** 31) + 40000, dtype=np.int64)
        x = x[(x >= 1) & (x <= M - 1)].astype(np.uint64)
        for side in ("below", "on", "above"):
            out[f"mix_{side}_{edge}"] = rng_back(x, 1)
    # the light pick draws the largest uniform: the second output is one of the top values
    top = np.arange(M - 400, M, dtype=np.uint64)
    out["pick_largest"] = rng_back(top, 2)
    # u + v next to 1: outputs t with t + 48271 t mod m next to m, i.e. 48272 t next to a multiple of m
    q = np.arange(1, 48272, dtype=np.int64)
    t = ((q * M + 24136) // 48272).astype(np.uint64)
    t = t[(t >= 1) & (t <= M - 1)]
    for side in ("below", "on", "above"):
        out[f"fold_{side}"] = rng_back(t, 3)
    # a disc pair rejected twice: seeded search forwards (the draws' count is not invertible)
    out["disc_twice"] = np.random.default_rng(20261101).integers(1, M, 20000).astype(np.uint64)
    picked = {}
    for aim, (pred, needs_lights) in AIMS.items():
        if needs_lights and not lights:
            continue
        cand = out[aim]
        cand = cand[(cand >= 1) & (cand <= M - 1)]
        with np.errstate(all="ignore"):
            ok = pred(_trace(cand, lights))
        picked[aim] = _spread(cand[ok], AIM_FRAMES).astype(np.uint32)
    return picked


class _Seeds:
    """Seeds whose mixture draw picks a given sampler, handed out in a fixed order."""

    def __init__(self, lights):
        s = np.random.default_rng(20261102).integers(1, M, 40000).astype(np.uint64)
        b = branch_of(mixture_s(rng_step(s), lights))
        self.pool = [s[b == k].astype(np.uint32) for k in range(3)]
        self.at = [0, 0, 0]
        self.samplers = 3 if lights else 2

    def take(self, sampler):
        sampler %= self.samplers
        self.at[sampler] += 1
        return self.pool[sampler][self.at[sampler] - 1]

    def each(self):
        return [self.take(k) for k in range(self.samplers)]


# ------------------------------------------------------------------ the classes
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum())


def _tangent(n32):
    """t with dot(t, n) exactly 0 in float32 (x, y, z order): two products that cancel."""
    n = np.asarray(n32, F32)
    if abs(n[1]) > max(abs(n[0]), abs(n[2])):
        return np.array([0, -n[2], n[1]], F32)
    return np.array([-n[2], 0, n[0]], F32)


def _eyes(n32):
    n = np.asarray(n32, F32).astype(np.float64)
    nh, t = _unit(n), _tangent(n32).astype(np.float64)
    th = _unit(t)
    return [n, nh, [0, 0, 1], [0, 0, -1], _unit(nh + 1e-3 * th), _unit(nh + th), t + 1e-6 * nh * np.sqrt((t * t).sum()), t,
            t - 1e-6 * nh * np.sqrt((t * t).sum()), -nh]


POINT = [0.25, 0.5, -1.0]
_NZ = F32(-0.0)


def _axis(seeds):
    rows = []
    normals = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, _NZ, -1]]
    for n in normals:
        n32 = np.array(n, F32)
        for eye in _eyes(n32):
            for r2 in (R2_LIMIT, 0.25, 1.0):
                for s in seeds.each():
                    rows.append((POINT, n32, eye, r2, s))
    return rows


def antipode_normals():
    out = []
    for d in (1e-3, 1e-5, 1e-7, 3e-8):
        for xy in ((d, 0.0), (d, d), (-d, 0.5 * d)):
            n = np.array([xy[0], xy[1], -1.0])
            out.append(_unit(n).astype(F32))          # unit: the x and y survive, z rounds to -1 for the small ones
            out.append((n * 2.0).astype(F32))         # non-unit
            out.append((n * 0.375).astype(F32))
    return out


def _antipode(seeds):
    rows = []
    for k, n32 in enumerate(antipode_normals()):
        for eye in _eyes(n32):
            for s in seeds.each()[: 2 if k % 3 else 3]:
                rows.append((POINT, n32, eye, 0.25, s))
    return rows


def _generic_frames(rng, n):
    p = rng.uniform(-3, 3, (n, 3))
    nn = np.array([_unit(v) for v in rng.uniform(-1, 1, (n, 3))])
    eye = np.array([_unit(v) for v in rng.uniform(-1, 1, (n, 3))])
    eye *= np.where((eye * nn).sum(1) < 0, -1.0, 1.0)[:, None]
    return p, nn, eye


def _rough(seeds, rng):
    rows = []
    lim = np.array([R2_LIMIT], F32)
    r2s = [np.nextafter(lim, F32(0))[0], R2_LIMIT, np.nextafter(lim, F32(1))[0], 0.25, 1.0, 2.0, 1e-3, 1e-6]
    p, nn, eye = _generic_frames(rng, 12)
    for r2 in r2s:
        for k in range(12):
            for s in seeds.each():
                rows.append((p[k], nn[k], eye[k], r2, s))
    return rows


def _branch(lights, rng):
    rows = []
    for aim, sd in aimed_seeds(lights).items():
        p, nn, eye = _generic_frames(rng, len(sd))
        for k, s in enumerate(sd):
            rows.append((p[k], nn[k], eye[k], 0.25, s))
    return rows


def _light(arrays, seeds, lights_on):
    """Points placed on and around the light list (arrays["light"], arrays["light_node"])."""
    L = np.asarray(arrays["light"], F32)
    if not lights_on or len(L) == 0:
        return []
    fold = aimed_seeds(True)
    fold = np.concatenate([fold["fold_below"], fold["fold_on"], fold["fold_above"]])
    ok = np.flatnonzero(np.isfinite(L[:, :13]).all(1))
    pick = ok[np.linspace(0, len(ok) - 1, min(6, len(ok))).astype(int)]
    rows, at = [], 0
    for k in pick:
        v0, U, V, n = (L[k, 0:3].astype(np.float64), L[k, 3:6].astype(np.float64), L[k, 6:9].astype(np.float64),
                       L[k, 9:12].astype(np.float64))
        c = v0 + (U + V) / 3
        pts = [v0, v0 + U, v0 + 0.5 * U, v0 + 0.5 * (U + V), c, c + 1e-4 * n, c - 1e-4 * n, c + 0.5 * n, c - 2.0 * n]
        for p in pts:
            eye = _unit(n + 0.5 * _unit(U)) if np.abs(U).max() > 0 else n
            sd = [seeds.take(2), seeds.take(2), seeds.take(0), seeds.take(1), fold[at % len(fold)]]
            at += 1
            for s in sd:
                rows.append((p, n, eye, 0.25, s))
    box = np.asarray(arrays["light_node"], F32)[0, :6].astype(np.float64)
    c = (box[:3] + box[3:]) / 2
    far = [c, box[:3], 0.25 * box[:3] + 0.75 * box[3:], c + [1e3, 0, 0], c + [0, -1e3, 0], c + [0, 0, 1e6], c + [1e6, 1e6, 0]]
    for p in far:
        for s in [seeds.take(2), seeds.take(2), seeds.take(2), seeds.take(0), seeds.take(1)]:
            rows.append((p, [0, -1, 0], _unit([0.3, -1, 0.2]), 0.25, s))
    return rows


def _nonfinite(seeds):
    inf, nan = np.inf, np.nan
    e = _unit([0.3, 1, 0.2])
    frames = [(POINT, [nan, 0, 0], e), (POINT, [nan, nan, nan], e), (POINT, [0, 0, 0], e), (POINT, [0, _NZ, 0], e),
              (POINT, [inf, 0, 0], e), (POINT, [0, -inf, 1], e), (POINT, [inf, inf, inf], e),
              ([nan, 0, 0], [0, 1, 0], e), ([nan, nan, nan], [0, 1, 0], e), ([inf, 0, 0], [0, 1, 0], e),
              ([0, -inf, inf], [0, 1, 0], e), (POINT, [0, 1, 0], [0, 0, 0]), (POINT, [0, 0, -1], [0, 0, 0]),
              (POINT, [0, nan, 1], [0, 0, 1]), (POINT, [-inf, 0, 0], [-1, 0, 0]), ([0, 0, nan], [1, 0, 0], [1, 0, 0]),
              ([-inf, -inf, -inf], [0, 0, 1], e), (POINT, [0, 0, 0], [0, 0, 0])]
    return [(p, n, eye, 0.25, s) for p, n, eye in frames for s in seeds.each()]


def _generic():
    """The first 256 frames and seeds ref_harness `samplers` drew (tests/golden/cornell_samplers.rtd)."""
    g = rtref.golden("cornell_samplers.rtd")
    return [(f[0:3], f[3:6], f[6:9], f[9], s) for f, s in zip(g["frame"][:256], g["seed"][:256])]


def shadeedge_frames(arrays):
    """dict(frame (n, 10) f32: point, normal, eye, r2; seed (n,) u32 in 1 .. 2147483646; warm (n,) u32,
    1: one polar pair is drawn before the sampler, so the normal cache is full at entry; cls (n,) i32)
    for a scene's arrays (the `light` class reads arrays["light"] and arrays["light_node"])."""
    lights = len(arrays["light"]) > 0
    seeds = _Seeds(lights)
    rng = np.random.default_rng(20261103)
    made = {"axis": _axis(seeds), "antipode": _antipode(seeds), "rough": _rough(seeds, rng), "branch": _branch(lights, rng),
            "light": _light(arrays, seeds, lights)}
    cold = [r for rows in made.values() for r in rows]
    made["warm"] = cold[::5]
    made["nonfinite"] = _nonfinite(seeds)
    made["generic"] = _generic()
    frame, seed, warm, cls = [], [], [], []
    with np.errstate(all="ignore"):
        for k, name in enumerate(CLASSES):
            for p, n, eye, r2, s in made[name]:
                frame.append(np.concatenate([np.asarray(p, np.float64).astype(F32), np.asarray(n, np.float64).astype(F32)
                                             if np.asarray(n).dtype != F32 else np.asarray(n),
                                             np.asarray(eye, np.float64).astype(F32), [F32(r2)]]).astype(F32))
                seed.append(s)
                warm.append(1 if name == "warm" else 0)
                cls.append(k)
    return {"frame": np.array(frame, F32).reshape(-1, 10), "seed": np.array(seed, np.uint32),
            "warm": np.array(warm, np.uint32), "cls": np.array(cls, np.int32)}


# ------------------------------------------------------------------ the comparison
FIELDS = ["dir.x", "dir.y", "dir.z", "pdf", "light_pdf", "next_normal", "next", "n_light_aabb", "n_light_tri"]


def record_of(gold):
    """A golden in the entries' layout: (n, 6) f32 and the last three columns of the (n, 4) i64."""
    f = np.concatenate([gold["dir"], gold["pdf"][:, None], gold["light_pdf"][:, None], gold["next_normal"][:, None]], 1)
    i = np.stack([gold["next"].astype(np.int64), gold["n_light_aabb"].astype(np.int64), gold["n_light_tri"].astype(np.int64)], 1)
    return f.astype(F32), i


def differing(out_f, out_i, want_f, want_i):
    """field -> bool array of the rows that differ under rtref.same (status is not compared here)."""
    bad = {FIELDS[k]: ~rtref.same(out_f[:, k], want_f[:, k]) for k in range(6)}
    bad.update({FIELDS[6 + k]: ~rtref.same(out_i[:, 1 + k], want_i[:, k]) for k in range(3)})
    return bad


def check_frames(frames_in, gold, out_f, out_i, label):
    """Every field the frame entries return, against the golden, under rtref.same; no status -2."""
    want_f, want_i = record_of(gold)
    assert len(out_f) == len(want_f) == len(frames_in["cls"])
    unfinished = np.flatnonzero(out_i[:, 0] != 0)
    assert len(unfinished) == 0, f"{label}: frames {unfinished[:8].tolist()} have status {out_i[unfinished[:8], 0].tolist()}"
    for name, bad in differing(out_f, out_i, want_f, want_i).items():
        k = np.flatnonzero(bad)
        cls = sorted({CLASSES[c] for c in frames_in["cls"][k]})
        assert len(k) == 0, f"{label} {name}: {len(k)} frames differ, classes {cls}, first {k[:8].tolist()}"
