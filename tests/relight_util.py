"""Helpers of the movable-light tests (test_relight.py, test_gpu_relight.py): the numpy restatement of
the rule written from include/rt_hw.h (independent of csrc/rt_relight.h and rt_refit_plan.h): the
map from lights to triangles, the light record (12 words and the float32 area, one rounding per
operation), the light boxes through refit_util.np_refit over light[:, :12], the twin arrays of an
update, and the special-value records on practice6_1's light tree."""
import numpy as np

from refit_util import FLT_MAX, NZ, PZ, bits, emissive_meshes, f32, np_refit, tri_mesh, word, zero_tri

NONE = 0xFFFFFFFF


def np_light_map(arrays):
    """tri_of_light: the lights in ascending index; light k takes the lowest-numbered triangle of an
    emissive mesh that is not yet taken and whose 12 words equal the light's words 0..11 bit for bit.
    Raises ValueError naming the first light without a triangle or the first triangle without a light."""
    tb = bits(arrays["tri"]).reshape(-1, 12)
    lb = bits(arrays["light"]).reshape(-1, 16)[:, :12]
    lit = np.flatnonzero(emissive_meshes(arrays)[tri_mesh(arrays)])
    free = {}
    for t in lit:   # ascending
        free.setdefault(tb[t].tobytes(), []).append(int(t))
    out = np.full(len(lb), NONE, np.uint32)
    for k in range(len(lb)):
        ids = free.get(lb[k].tobytes())
        if not ids:
            raise ValueError(f"light {k}")
        out[k] = ids.pop(0)
    left = sorted(t for ids in free.values() for t in ids)
    if left:
        raise ValueError(f"triangle {left[0]}")
    return out


def np_area(tri):
    """0.5f * length(cross(U, V)) per record, float32 with one rounding per operation:
    cross(a, b) = (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y), length from 0."""
    tri = np.ascontiguousarray(tri, f32).reshape(-1, 12)
    ax, ay, az = tri[:, 3], tri[:, 4], tri[:, 5]
    bx, by, bz = tri[:, 6], tri[:, 7], tri[:, 8]
    with np.errstate(all="ignore"):
        c = ((ay * bz).astype(f32) - (by * az).astype(f32)).astype(f32), \
            ((az * bx).astype(f32) - (bz * ax).astype(f32)).astype(f32), \
            ((ax * by).astype(f32) - (bx * ay).astype(f32)).astype(f32)
        m = np.zeros(len(tri), f32)
        for x in c:
            m = (m + (x * x).astype(f32)).astype(f32)
        return (f32(0.5) * np.sqrt(m).astype(f32)).astype(f32)


def np_relight(arrays, tri, tri_of_light):
    """(light, light_node): words 0..11 of light k are triangle tri_of_light[k]'s bits, word 12 its
    area, words 13..15 kept; every light box recomputed by the refit rule over the light records."""
    tri = np.ascontiguousarray(tri, f32).reshape(-1, 12)
    light = np.ascontiguousarray(arrays["light"], f32).copy()
    tl = np.asarray(tri_of_light, np.int64)
    if len(light):
        light.view(np.uint32)[:, 0:12] = bits(tri)[tl]
        light[:, 12] = np_area(tri[tl])
    lnode = np.ascontiguousarray(arrays["light_node"], f32)
    if len(lnode):
        lnode = np_refit(np.ascontiguousarray(light[:, :12]), lnode)
    return light, lnode


def twin_arrays_lit(arrays, tri, attr=None, tan=None):
    """The arrays of the scene an update on an opted-in scene must equal: the new records, node,
    light and light_node the restatement's (the map is that of `arrays` as they were)."""
    a = dict(arrays)
    a["tri"] = np.ascontiguousarray(tri, f32)
    if attr is not None:
        a["tri_attr"] = np.ascontiguousarray(attr, f32)
    if tan is not None:
        a["tri_tan"] = np.ascontiguousarray(tan, f32)
    a["node"] = np_refit(a["tri"], arrays["node"])
    a["light"], a["light_node"] = np_relight(arrays, a["tri"], np_light_map(arrays))
    return a


def same_lights(got, want):
    """light arrays equal in every bit, except an area word (12) where both are NaN (an invalid
    operation gives different default NaNs on the host and on the GPU)."""
    g, w = np.ascontiguousarray(got, f32).reshape(-1, 16), np.ascontiguousarray(want, f32).reshape(-1, 16)
    if g.shape != w.shape:
        return False
    eq = bits(g) == bits(w)
    eq[:, 12] |= np.isnan(g[:, 12]) & np.isnan(w[:, 12])
    return bool(eq.all())


def light_leaves(arrays):
    """[(node id, first, count)] of the light tree's leaves, and {child id: parent id}."""
    ab = bits(arrays["light_node"])[:, 6:8]
    out, parent = [], {}
    for i, (a, b) in enumerate(ab):
        if b & 3 == 3:
            out.append((i, int(a), int(b >> 2)))
        else:
            parent[int(a)] = parent[int(a) + 1] = i
    return out, parent


def special_light_records(arrays):
    """refit_util.special_records on the light tree: the records go into the triangles the lights
    restate.  Two sibling pairs of light leaves with at least two lights each take the +-0 orders
    (pair 1: left +0 then -0, right -0 then +0; pair 2 the mirror image), and one more leaf of at
    least four takes a NaN component, an all-NaN record and +-inf / FLT_MAX components.
    Returns (tri, expectations, nan_light): expectations = [(light node id, word, expected bits)],
    nan_light the light whose record is all NaN (its area is NaN)."""
    tri = np.ascontiguousarray(arrays["tri"], f32).copy()
    tl = np_light_map(arrays)
    lv, parent = light_leaves(arrays)
    ok = {i: (a, n) for i, a, n in lv}
    lb = bits(arrays["light_node"])
    pairs = [(i, i + 1) for i in ok if i + 1 in ok and i in parent and parent.get(i) == parent.get(i + 1) and i == lb[parent[i], 6]
             and ok[i][1] >= 2 and ok[i + 1][1] >= 2]
    assert len(pairs) >= 2, "the light tree has no two sibling pairs of leaves with two lights each"
    used, expect = set(), []
    for (l, r), (s_first, s_second) in zip(pairs[:2], ((PZ, NZ), (NZ, PZ))):
        for leaf, (sa, sb) in ((l, (s_first, s_second)), (r, (s_second, s_first))):
            a, n = ok[leaf]
            for k in range(n):
                sx = sa if k == 0 else sb
                t = int(tl[a + k])
                tri[t] = zero_tri(tri[t], sx, -sx, f32(0.125) * k)
            expect += [(leaf, 0, word(sa)), (leaf, 5, word(-sa))]
            used.add(leaf)
        expect += [(parent[l], 0, word(s_first)), (parent[l], 5, word(-s_first))]
    assert {e[2] for e in expect} == {word(PZ), word(NZ)}
    big = max((i for i in ok if i not in used), key=lambda i: ok[i][1])
    a, n = ok[big]
    assert n >= 4
    t1, t2, t3 = (int(tl[a + k]) for k in (1, 2, 3))
    tri[t1, 1] = np.nan
    tri[t2, 0:12] = np.nan
    tri[t3, 0:9] = [0.25, FLT_MAX, 0.25, 0, FLT_MAX, -np.inf, 0, -np.inf, 0]
    expect += [(big, 1, word(-np.inf)), (big, 4, word(np.inf)), (big, 2, word(-np.inf))]
    return tri, expect, a + 2


def translated_mesh(arrays, mesh, offset):
    """tri with v0 + offset for the mesh's triangles (one f32 add per component)."""
    tri = np.ascontiguousarray(arrays["tri"], f32).copy()
    sel = tri_mesh(arrays) == mesh
    tri[sel, 0:3] = (tri[sel, 0:3] + np.asarray(offset, f32)).astype(f32)
    return tri


def light_mesh(arrays):
    """The emissive mesh with the most triangles."""
    counts = np.bincount(tri_mesh(arrays), minlength=len(arrays["mesh_f"]))
    return int(np.argmax(counts * emissive_meshes(arrays)))


def wiped(arrays, first_word=0):
    """The arrays with light words first_word..12 and every light box NaN: what is read back
    afterwards can only have been restated.  (first_word=12 keeps words 0..11, which the map rule
    reads: such a scene can still opt in.)"""
    b = dict(arrays, light=arrays["light"].copy(), light_node=arrays["light_node"].copy())
    b["light"][:, first_word:13] = np.nan
    b["light_node"][:, 0:6] = np.nan
    return b
