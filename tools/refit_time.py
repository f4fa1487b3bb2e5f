#!/usr/bin/env python3
"""What moving geometry costs.  On the headline scene (sponza proxy, one GPU) it takes, per
repetition, the HIP-event time (and the wall time) of

  a  every movable triangle through the device entry (rt_scene_update_tris_device): one call per run
     of triangles between the emissive ones, each call a scatter, a refit of the whole tree and the
     read-back of the changed range and the node array into the host arrays
  b  one mesh through the device entry: the range from its first to its last triangle, cut at the
     emissive ones (the same refit; a smaller scatter and read-back)
  c  what a caller had to do before: rt_scene_free, rt_scene_from_view of the new arrays, rt_scene_upload

and appends one JSON line per repetition to profiles/refit_time.jsonl.  The records moved are the
scene's own (offset 0 keeps every later repetition on the same geometry).  Fails when a is not below
c in any repetition.

    python tools/refit_time.py [--reps N] [--mesh M] [--label NAME] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from denoise_passes import commit  # noqa: E402


def runs_of(ids):
    return [(int(r[0]), len(r)) for r in np.split(ids, np.flatnonzero(np.diff(ids) != 1) + 1)] if len(ids) else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mesh", type=int, default=-1, help="the mesh of measurement b (default: the largest non-emissive one)")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--commit", default=None, help="the commit the figures come from (default: HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_time.jsonl"))
    args = ap.parse_args()
    path = bench.load_scenes_module().ensure_scene(args.scene, os.environ.get("RT_SCENE_DIR", "/tmp/rt_scenes"))
    import torch  # (shares its HIP runtime with librt_hw_amd.so)
    torch.zeros(1, device="cuda")
    rt = bench.import_pkg()
    scene = rt.Scene.load(path, 64, 36, 1)
    scene.upload(0)
    v = scene.view()
    mesh_of = v["tri_attr"][:, 15].view(np.int32)
    emissive = np.any(v["mesh_f"][:, 3:6] != 0, axis=1)
    whole = runs_of(np.flatnonzero(~emissive[mesh_of]))
    sizes = np.bincount(mesh_of, minlength=len(emissive)) * ~emissive
    mesh = args.mesh if args.mesh >= 0 else int(np.argmax(sizes))
    # (a mesh's triangles lie scattered in post-build order and every call refits the whole tree: its
    # covering range, cut at the emissive triangles, is the way to move it; Scene.translated_records cover=True)
    own = np.flatnonzero(mesh_of == mesh)
    span = np.arange(own[0], own[-1] + 1)
    part = runs_of(span[~emissive[mesh_of[span]]])
    d_tri = torch.from_numpy(v["tri"]).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    base = {"what": "refit_time", "label": args.label, "commit": args.commit or commit(), "scene": args.scene, "n_tris": int(len(v["tri"])),
            "n_nodes": int(len(v["node"])), "levels": int(v["bvh_depth"]) + 1,
            "launches_per_refit": int(v["bvh_depth"]) + 2,   # the scatter and one launch per level
            "a_calls": len(whole), "a_tris": int(sum(n for _, n in whole)), "b_mesh": mesh, "b_mesh_tris": int(len(own)), "b_mesh_runs": len(runs_of(own)), "b_calls": len(part),
            "b_tris": int(sum(n for _, n in part)), "lib": os.environ.get("RT_LIB", "default")}

    def update(runs):
        for first, n in runs:
            scene.update_triangles(first, d_tri[first:first + n], device=0, stream_ptr=stream)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return round(a.elapsed_time(b), 4), round((time.perf_counter() - t0) * 1e3, 4)

    def rebuild():
        nonlocal scene
        scene = None   # rt_scene_free: the device copy goes with it
        scene = rt.Scene.from_view(v)
        scene.upload(0)

    update(whole)   # warm-up: the plan, the kernels' first launch
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    ok = True
    with open(args.out, "a") as f:
        for rep in range(args.reps):
            a_ms, a_wall = timed(lambda: update(whole))
            b_ms, b_wall = timed(lambda: update(part))
            c_ms, c_wall = timed(rebuild)
            rec = dict(base, rep=rep, a_whole_ms=a_ms, a_whole_wall_ms=a_wall, b_mesh_ms=b_ms, b_mesh_wall_ms=b_wall,
                       c_rebuild_ms=c_ms, c_rebuild_wall_ms=c_wall)
            line = json.dumps(rec)
            f.write(line + "\n")
            print(line, flush=True)
            ok = ok and a_ms < c_ms and a_wall < c_wall
    # the boxes after all of it are still the loader's
    assert np.array_equal(scene.read_device()["node"].view(np.uint32), v["node"].view(np.uint32))
    if not ok:
        sys.exit("refit_time: a whole-scene update was not faster than free + from_view + upload")


if __name__ == "__main__":
    main()
