"""Helpers of the posable-mesh tests (test_pose.py, test_gpu_pose.py): the poses, the variant glTF
files that carry them in their nodes (what the reference's loader was run on to make
tests/golden/pose_*_dump.rtd, tools/make_pose_goldens.py), and the matching of a posed scene's
triangles with a variant's through tri_source."""
import json
import os
import shutil

import numpy as np

import rtdump
import rtref

f32 = np.float32


def _f(v):
    return [float(f32(x)) for x in v]


# variant -> (base fixture, {node name: (translation, rotation, scale)}).  Every pose is a rotation about
# a direction that is no axis (a unit quaternion x y z w, written out in float32 so that the goldens do
# not depend on a sine), a scale with three different factors and a translation; Cube.001's has a
# negative determinant.  The values are float32, so the file's decimal text gives them back exactly.
# The blob's angle was searched for (24000 angles tried): at this one a build that fuses a product of
# the transforms with the add after it gets words of the expected records wrong (test_pose.py,
# test_the_inputs_tell_a_fused_build_from_the_rule); at most angles no word of 40000 shows it.
VARIANTS = {
    "pose_cornell": ("cornell", {
        # about (1, 2, 3) by 0.7 rad
        "Cube": (_f([-0.61, -0.93, -0.52]), [0.09164329618215561, 0.18328659236431122, 0.27492988109588623, 0.939372718334198],
                 _f([0.45, 0.9, 0.55])),
        # about (-2, 1, 0.5) by 1.1 rad
        "Cube.001": (_f([0.9, -1.3, 0.2]), [-0.4562388062477112, 0.2281194031238556, 0.1140597015619278, 0.8525245189666748],
                     _f([-0.5, 0.45, 0.4])),
    }),
    "pose_cornell_blob": ("cornell_blob", {
        # about (1, 2, 3) by 1.8877 rad
        "blob": (_f([0.15, -1.0, 0.25]), [0.21643424034118652, 0.43286848068237305, 0.6493027210235596, 0.5866745710372925],
                 _f([0.7, 0.85, 0.6])),
    }),
    "pose_texedge": ("texedge", {
        # about (2, -1, 1) by 0.35 rad
        "Floor": (_f([0.1, 0.12, -0.2]), [0.14215870201587677, -0.07107935100793839, 0.07107935100793839, 0.9847265481948853],
                  _f([0.9, 0.8, 1.1])),
    }),
}
# the cornell lamp (an emissive mesh) for the light tests: no golden, the light rule is rt_relight.h's;
# about (1, 5, 2) by 0.6 rad
LAMP = ("Plane.005", (_f([0.2, 1.9, -0.3]), [0.053954362869262695, 0.2697718143463135, 0.10790872573852539, 0.9553365111351013],
                      _f([1.3, 1.0, 0.7])))


def golden_name(variant, second=False):
    """The variant's golden; second: the file that holds the rest where one file would pass the size
    limit for a committed file (tools/make_pose_goldens.py)."""
    return f"{variant}_dump_b.rtd" if second else f"{variant}_dump.rtd"


def load_golden(variant):
    d = dict(rtdump.load(os.path.join(rtref.GOLD, golden_name(variant))))
    second = os.path.join(rtref.GOLD, golden_name(variant, second=True))
    if os.path.exists(second):
        d.update(rtdump.load(second))
    return d


def mesh_ids(gltf_path):
    """{node name: [mesh ids]}: a mesh id counts primitives over the nodes in file order, as the loader does."""
    doc = json.load(open(gltf_path))
    out, k = {}, 0
    for node in doc["nodes"]:
        if "mesh" not in node:
            continue
        n = len(doc["meshes"][node["mesh"]]["primitives"])
        out.setdefault(node.get("name", ""), []).extend(range(k, k + n))
        k += n
    return out


def write_variant(variant, directory):
    """A copy of the base fixture under `directory` whose named nodes carry the variant's
    translation / rotation / scale; returns the .gltf path."""
    base, poses = VARIANTS[variant]
    src = os.path.dirname(rtref.scene_path(base))
    dst = os.path.join(str(directory), variant)
    if os.path.isdir(dst):
        shutil.rmtree(dst)
    shutil.copytree(src, dst)
    path = os.path.join(dst, base + ".gltf")
    doc = json.load(open(path))
    left = set(poses)
    for node in doc["nodes"]:
        if node.get("name") in poses and "mesh" in node:
            t, r, s = poses[node["name"]]
            node.pop("matrix", None)
            node["translation"], node["rotation"], node["scale"] = list(t), list(r), list(s)
            left.discard(node["name"])
    assert not left, f"{base} has no node {sorted(left)}"
    with open(path, "w") as f:
        json.dump(doc, f)
    return path


def pose_matrices(rt, variant):
    """{mesh id: M} of the variant's poses on the base fixture (rt.trs: the loader's matrix4::TRS)."""
    base, poses = VARIANTS[variant]
    ids = mesh_ids(rtref.scene_path(base))
    return {m: rt.trs(*poses[name]) for name in poses for m in ids[name]}


def lamp_pose(rt):
    ids = mesh_ids(rtref.scene_path("cornell"))
    return {m: rt.trs(*LAMP[1]) for m in ids[LAMP[0]]}


_golden_cache = {}


def variant_golden(rt, variant, directory):
    """(arrays of the reference's load of the variant in this build's layout, the variant's .gltf path);
    computed once per variant and shared (treat as read-only)."""
    if variant not in _golden_cache:
        base = VARIANTS[variant][0]
        path = write_variant(variant, directory)
        _golden_cache[variant] = (rtref.ref_arrays(rt, base, 64, 64, 1, dump=load_golden(variant), path=path), path)
    return _golden_cache[variant]


def through_source(src_posed, src_variant):
    """For every triangle of the posed scene the index of the same triangle (same load-order index) in the
    variant's post-build order."""
    place = np.empty(len(src_variant), np.int64)
    place[np.asarray(src_variant, np.int64)] = np.arange(len(src_variant))
    return place[np.asarray(src_posed, np.int64)]
