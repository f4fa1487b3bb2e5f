#!/usr/bin/env python3
"""Generate tests/golden/pose_*_dump.rtd from the REFERENCE ITSELF: its loader (oracle/ref_harness
`dump`, the reference's sources compiled as its CMake build compiles them) run on the variant glTF files
of tests/pose_util.py, whose nodes carry the poses the tests apply with Scene.pose.  Needs the reference
build (make -C oracle ref).  Nothing here is computed by this build's code.

    python tools/make_pose_goldens.py

A golden keeps the fields tests/rtref.py ref_arrays reads (tools/make_goldens.py compact_dump), all-zero
texcoord / tangent blocks dropped.  The repository's size limit for a committed file is 1 MiB: a golden
over it (the blob's) is written as two files, <variant>_dump.rtd and <variant>_dump_b.rtd (the tree and
the attributes a pose does not touch), which tests/pose_util.py reads back as one.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_util  # noqa: E402
import rtdump  # noqa: E402

LIMIT = 1 << 20
# what ref_arrays and the loader tests read
KEEP = ("obj_position", "obj_geo_normal", "obj_normal", "obj_texcoord", "obj_tangent", "obj_mesh_id", "node_aabb", "node_meta",
        "light_position", "light_geo_normal", "light_area", "light_mesh_id", "lnode_aabb", "lnode_meta", "mesh_f", "mesh_tex",
        "mesh_normal_transform", "camera", "ray_depth")
# a golden over the limit is written as two files (pose_util.variant_golden reads both): these fields
# go to the second
SECOND = ("node_aabb", "node_meta", "obj_texcoord", "obj_tangent")


def pack(d):
    out = {}
    for k in KEEP:
        if k not in d:
            continue
        v = d[k]
        if k in ("obj_texcoord", "obj_tangent") and not np.any(v):
            continue   # (ref_arrays fills zeros in)
        if v.dtype.kind in "iu" and v.size and v.dtype.itemsize > 4 and np.abs(v.astype(np.int64)).max() < 2 ** 31:
            v = v.astype(np.int32)
        out[k] = v
    return out


def main():
    if not os.path.exists(HARNESS):
        sys.exit("build the reference harness first: make -C oracle ref")
    with tempfile.TemporaryDirectory() as tmp:
        for variant in pose_util.VARIANTS:
            path = pose_util.write_variant(variant, tmp)
            raw = os.path.join(tmp, variant + "_full.rtd")
            subprocess.run([HARNESS, "dump", path, "64", "64", raw], check=True, capture_output=True)
            d = rtdump.load(raw)
            out = os.path.join(GOLD, pose_util.golden_name(variant))
            second = os.path.join(GOLD, pose_util.golden_name(variant, second=True))
            p = pack(d)
            rtdump.save(out, p)
            if os.path.exists(second):
                os.remove(second)
            if os.path.getsize(out) > LIMIT:   # two files: the tree and the pose-independent attributes apart
                b = {k: p.pop(k) for k in SECOND if k in p}
                rtdump.save(out, p)
                rtdump.save(second, b)
            for f in (out, second):
                if os.path.exists(f):
                    print(variant, os.path.basename(f), os.path.getsize(f))
                    if os.path.getsize(f) > LIMIT:
                        sys.exit(f"{f}: over the limit for a committed file")


if __name__ == "__main__":
    main()
