"""Helpers of the movable-geometry tests (test_refit.py, test_gpu_refit.py): the numpy restatement of
the refit rule written from include/rt_hw.h (independent of csrc/rt_refit.h), the special-value
records on cornell's tree, and twins built by from_view."""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
DUMPS = ("cornell", "cornell_blob", "practice6_1", "geoedge")   # triangles / nodes / largest leaf: 36/19/8, 10036/6285/8, 16910/10661/11, 138/61/16
NZ = f32(-0.0)
PZ = f32(0.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def word(x):
    """The bit pattern of one float32."""
    return int(np.float32(x).view(np.uint32))


def smin(a, b):
    """std::min as a select: b < a ? b : a (np.minimum would propagate a NaN and rank -0 < +0)."""
    return np.where(b < a, b, a).astype(f32)


def smax(a, b):
    return np.where(a < b, b, a).astype(f32)


def np_tri_boxes(tri):
    """(n, 3) lo and hi of every triangle: the fold over v0, v0 + U, v0 + V from the empty box."""
    tri = np.ascontiguousarray(tri, f32).reshape(-1, 12)
    v0, U, V = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    lo = np.full(v0.shape, FLT_MAX, f32)
    hi = np.full(v0.shape, -FLT_MAX, f32)
    with np.errstate(all="ignore"):
        for p in (v0, (v0 + U).astype(f32), (v0 + V).astype(f32)):
            lo, hi = smin(lo, p), smax(hi, p)
    return lo, hi


def np_refit(tri, node):
    """The node array with every box recomputed: leaves fold their triangles' boxes in order,
    internal nodes grow(left) then grow(right), children after parents (one reverse sweep)."""
    node = np.ascontiguousarray(node, f32).reshape(-1, 8)
    out = node.copy()
    ab = bits(node)[:, 6:8]
    tlo, thi = np_tri_boxes(tri)
    with np.errstate(all="ignore"):
        for i in range(len(node) - 1, -1, -1):
            a, b = int(ab[i, 0]), int(ab[i, 1])
            lo, hi = np.full(3, FLT_MAX, f32), np.full(3, -FLT_MAX, f32)
            if b & 3 == 3:
                for t in range(a, a + (b >> 2)):
                    lo, hi = smin(lo, tlo[t]), smax(hi, thi[t])
            else:
                for c in (a, a + 1):
                    lo, hi = smin(lo, out[c, 0:3]), smax(hi, out[c, 3:6])
            out[i, 0:3], out[i, 3:6] = lo, hi
    assert np.array_equal(bits(out)[:, 6:8], ab)
    return out


def emissive_meshes(arrays):
    return np.any(np.asarray(arrays["mesh_f"])[:, 3:6] != 0, axis=1)


def tri_mesh(arrays):
    return np.ascontiguousarray(arrays["tri_attr"], f32)[:, 15].view(np.int32)


def leaves(arrays):
    """[(node id, first, count)] of the leaves, and {child id: parent id}."""
    ab = bits(arrays["node"])[:, 6:8]
    out, parent = [], {}
    for i, (a, b) in enumerate(ab):
        if b & 3 == 3:
            out.append((i, int(a), int(b >> 2)))
        else:
            parent[int(a)] = parent[int(a) + 1] = i
    return out, parent


def zero_tri(rec, sign_x, sign_z, y):
    """A record whose box has min.x = sign_x * 0 and max.z = sign_z * 0 exactly: v0 = (+-0, y, -+0),
    U = (1, 0, -1), V = (+0, 1, +0).  x: s0, s0 + 1, s0 + 0 (-0 + +0 = +0, which is not < -0);
    z: s0, s0 - 1, s0 + 0 (no point is above s0)."""
    r = np.array(rec, f32)
    r[0:9] = [sign_x, y, sign_z, 1, 0, -1, 0, 1, 0]
    return r


def special_records(arrays):
    """cornell's triangles with special values in non-emissive leaves (include/rt_hw.h, movable
    geometry).  Found on the tree as it is: two sibling pairs of leaves with at least two triangles
    each, no emissive triangle, and one more leaf of at least four.
      pair 1: left leaf  min.x attained by +0 then -0 (stays +0), max.z by -0 then +0 (stays -0);
              right leaf the reverse order (-0, +0);
              so across the pair the parent sees +0 then -0 in min.x and -0 then +0 in max.z
      pair 2: the mirror image (left -0 / +0, right +0 / -0)
      big leaf: one vertex with a NaN component, one all-NaN triangle, +-inf and FLT_MAX components
      one more leaf, if there is one: every triangle all NaN (its box is the empty box)
    Returns (tri, expectations) with expectations = [(node id, word, expected bits)]."""
    tri = np.ascontiguousarray(arrays["tri"], f32).copy()
    em = emissive_meshes(arrays)
    mesh = tri_mesh(arrays)
    lv, parent = leaves(arrays)
    ok = {i: (a, n) for i, a, n in lv if not em[mesh[a:a + n]].any()}
    pairs = [(i, i + 1) for i in ok if i + 1 in ok and parent.get(i) == parent.get(i + 1) and i == bits(arrays["node"])[parent[i], 6]
             and ok[i][1] >= 2 and ok[i + 1][1] >= 2]
    assert len(pairs) >= 2, "cornell's tree no longer has two sibling pairs of non-emissive leaves"
    used, expect = set(), []
    pz, nz = word(PZ), word(NZ)
    for (l, r), (s_first, s_second) in zip(pairs[:2], ((PZ, NZ), (NZ, PZ))):
        for leaf, (sa, sb) in ((l, (s_first, s_second)), (r, (s_second, s_first))):
            a, n = ok[leaf]
            for k in range(n):
                sx = sa if k == 0 else sb
                tri[a + k] = zero_tri(tri[a + k], sx, -sx, f32(0.125) * k)
            expect += [(leaf, 0, word(sa)), (leaf, 5, word(-sa))]
            used.add(leaf)
        expect += [(parent[l], 0, word(s_first)), (parent[l], 5, word(-s_first))]
    assert {e[2] for e in expect} == {pz, nz}
    big = max((i for i in ok if i not in used), key=lambda i: ok[i][1])
    a, n = ok[big]
    assert n >= 4
    tri[a + 1, 1] = np.nan                       # one vertex component
    tri[a + 2, 0:12] = np.nan                    # a whole record
    tri[a + 3, 0:9] = [0.25, FLT_MAX, 0.25, 0, FLT_MAX, -np.inf, 0, -np.inf, 0]   # y: FLT_MAX, +inf, -inf; z: 0.25, -inf, 0.25
    used.add(big)
    expect += [(big, 1, word(-np.inf)), (big, 4, word(np.inf)), (big, 2, word(-np.inf))]
    rest = [i for i in ok if i not in used]
    if rest:
        a, n = ok[rest[0]]
        tri[a:a + n, 0:12] = np.nan
        expect += [(rest[0], 0, word(FLT_MAX)), (rest[0], 3, word(-FLT_MAX))]
    return tri, expect


def changed_runs(old, new):
    """[(first, count)] runs of records that differ bit for bit (NaN payloads included)."""
    d = np.flatnonzero((bits(old) != bits(new)).any(axis=1))
    if not len(d):
        return []
    return [(int(r[0]), len(r)) for r in np.split(d, np.flatnonzero(np.diff(d) != 1) + 1)]


def twin_arrays(arrays, tri, attr=None, tan=None):
    """The arrays of the scene an update must equal: the new records, node = the restatement's."""
    a = dict(arrays)
    a["tri"] = np.ascontiguousarray(tri, f32)
    if attr is not None:
        a["tri_attr"] = np.ascontiguousarray(attr, f32)
    if tan is not None:
        a["tri_tan"] = np.ascontiguousarray(tan, f32)
    a["node"] = np_refit(a["tri"], arrays["node"])
    return a


def same_view(a, b, keys=("tri", "tri_attr", "tri_tan", "node", "light", "light_node", "mesh_f")):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys) and a["bvh_depth"] == b["bvh_depth"]


def box_mesh(arrays):
    """A non-emissive mesh of 12 triangles (a box), the last such mesh id."""
    em = emissive_meshes(arrays)
    mesh = tri_mesh(arrays)
    ids = [m for m in range(len(em)) if not em[m] and (mesh == m).sum() == 12]
    assert ids, "no non-emissive box mesh"
    return ids[-1]


def translated(arrays, mesh, offset):
    """tri with v0 + offset for the mesh's triangles: one f32 add per component."""
    tri = np.ascontiguousarray(arrays["tri"], f32).copy()
    sel = tri_mesh(arrays) == mesh
    tri[sel, 0:3] = (tri[sel, 0:3] + np.asarray(offset, f32)).astype(f32)
    return tri
