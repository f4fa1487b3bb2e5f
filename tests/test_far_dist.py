"""The traversal's cull without a square root (rt_wavefront.h far_gt, kFarMax2, box_dist2
frames; tests/native/far_dist_host.cpp): the predicate against sqrtf at the rounding boundary,
and the cull's equality case on a scene whose entry distances are perfect squares, against
closest_hit in rt_path.h, which keeps the sqrt form.  Both settings of RT_FAR_DIST2."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "far_dist_host.cpp")


def _build(tmp_path_factory, dist2):
    out = str(tmp_path_factory.mktemp(f"fd{dist2}") / "libfd.so")
    subprocess.run(["g++", "-O2", "-fno-tree-vectorize", "-fno-tree-slp-vectorize", "-ffp-contract=off", "-fopenmp",
                    "-std=c++17", "-shared", "-fPIC", f"-DRT_FAR_DIST2={dist2}", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    for f in ("fd_far_gt_check", "fd_case_spread", "fd_const_check"):
        getattr(lib, f).argtypes = []
        getattr(lib, f).restype = ctypes.c_int64
    lib.fd_far_dist2.restype = ctypes.c_int
    lib.fd_trace.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 5
    lib.fd_trace.restype = ctypes.c_int64
    return lib


@pytest.fixture(scope="module", params=[1, 0], ids=["dist2", "sqrt"])
def fd(request, tmp_path_factory):
    lib = _build(tmp_path_factory, request.param)
    assert lib.fd_far_dist2() == request.param
    return lib


# (x, z) of the quads.  Quads one above the other at distinct z give the builder disjoint
# boxes, and a near subtree's best can then never lie on the far box; with two columns and
# repeated z the builder also splits along x, sibling boxes share the plane x = 1 and z
# planes, and rays along that plane enter far boxes exactly at the near subtree's best.
STACK = [(0, 0), (1, 1), (0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (0, 4)]


def stack_scene(rt, directory):
    """A stack of 8 axis-aligned unit quads (16 triangles) at integer z in two columns, loaded
    through the package (its own BVH builder); returns the scene's arrays."""
    sc = rtref.scenes_module()
    b = sc.GltfBuilder()
    b.cameras = [dict(sc.CORNELL_CAMERA)]
    b.extensions_used.add("KHR_materials_emissive_strength")
    b.materials = [dict(sc.CORNELL_MATERIALS[0]), dict(sc.CORNELL_MATERIALS[3])]   # wall, light
    b.nodes = [{"camera": 0, "name": "Camera", "translation": [0.5, 0.5, 12]}]
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (4, 1))
    idx = np.array([0, 1, 3, 0, 3, 2], np.uint32)
    m = [b.mesh("quad", [b.primitive(pos, nrm, idx, 0)]), b.mesh("lamp", [b.primitive(pos, nrm, idx, 1)])]
    for k, (x, z) in enumerate(STACK):   # (the two topmost quads emit: a render of it is not black)
        b.nodes.append({"mesh": m[k >= 6], "name": f"quad{k}", "translation": [x, 0, z]})
    return rt.Scene.load(b.write(str(directory), "stack"), 8, 8, 1).view()


def stack_rays():
    """64 rays along +z and -z from integer origins: the quads' corners and points beside them,
    from outside the stack, from on a quad and from between two (inside the boxes that span
    them).  x and y of every direction are zero."""
    org, dirs = [], []
    for x, y in [(0, 0), (1, 1), (1, 0), (0, 1), (2, 0), (0, -1), (1, 2), (-1, -1)]:
        for z, dz in [(-3, 1), (10, -1), (3, 1), (3, -1), (-3, -1), (0, 1), (7, -1), (12, -1)]:
            org.append([x, y, z])
            dirs.append([0, 0, dz])
    return np.array(org, np.float32), np.array(dirs, np.float32)


def test_far_gt_equals_sqrt_compare(fd):
    assert fd.fd_case_spread() == 0
    assert fd.fd_far_gt_check() == 0


def test_squared_1e9_constant(fd):
    assert fd.fd_const_check() == 0


def test_cull_equality_case_matches_closest_hit(rt, fd, oracle, tmp_path):
    arrays = stack_scene(rt, tmp_path)
    assert len(arrays["tri"]) == 16
    v, keep = rt.make_view(arrays)
    org, dirs = stack_rays()
    n = len(org)
    assert n == 64
    out_i = np.zeros((n, 3), np.int32)
    out_t = np.zeros(n, np.float32)
    equal = ctypes.c_int64(0)
    bad = fd.fd_trace(ctypes.addressof(v), n, org.ctypes.data, dirs.ctypes.data, out_i.ctypes.data, out_t.ctypes.data,
                      ctypes.addressof(equal))
    del keep
    assert bad == 0
    # the case this scene is for: far children entered at entry distance == near best
    assert equal.value > 0
    hit = out_i[:, 0] >= 0
    assert hit.sum() >= 24 and (~hit).sum() >= 16
    t = out_t[hit]
    assert np.array_equal(t, np.round(t))   # integer distances: perfect squares under the root
    # and the CPU oracle (its own restatement of the reference's traversal) on the same rays
    wf, wi = oracle.rays(arrays, org, dirs)
    assert np.array_equal(wi[:, 0].astype(bool), hit)
    assert np.array_equal(wi[hit, 1], out_i[hit, 0])
    assert np.array_equal(rtref.bits(wf[hit, 0]), rtref.bits(t))
    assert np.array_equal(wi[:, 2:4], out_i[:, 1:3])
