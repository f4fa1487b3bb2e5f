#!/usr/bin/env python3
"""What a pose costs.  On the headline scene (sponza proxy, one GPU) it takes, per repetition, the
HIP-event time and the wall time of

  pose_all   rt_scene_pose_meshes of every non-emissive mesh in one call (each to the matrix it has: the
             work does not depend on the matrix, and every later repetition sees the same geometry)
  pose_one   the same for one mesh (--mesh, default 0)
  old_all    the same change made without the entry: the records computed on the host (rt_pose_view),
  old_one    copied to the device, and put in place through rt_scene_update_tris_device, one call per run
             between the emissive triangles of the covering range (rows a and b of tools/refit_time.py)
  twin_all   the host twin alone: the same pose on a scene that is on no device (wall time only), so
  twin_one   pose - twin is the device half: image patch, table upload, the kernels and the wait

and appends one JSON line per repetition to profiles/pose_time.jsonl.  The split of the device half
into its launches is not taken here (a kernel trace gives it).

    python tools/pose_time.py [--reps N] [--mesh M] [--label NAME] [--out FILE]
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
from refit_time import runs_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mesh", type=int, default=0)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_time.jsonl"))
    args = ap.parse_args()
    path = bench.load_scenes_module().ensure_scene(args.scene, os.environ.get("RT_SCENE_DIR", "/tmp/rt_scenes"))
    import torch  # (shares its HIP runtime with librt_hw_amd.so)
    torch.zeros(1, device="cuda")
    rt = bench.import_pkg()
    scene = rt.Scene.load(path, 64, 36, 1)
    twin = rt.Scene.load(path, 64, 36, 1)   # never uploaded
    scene.upload(0)
    for s in (scene, twin):
        s.enable_poses()
    v = scene.view()
    rest = scene.rest()
    mesh_of = v["tri_attr"][:, 15].view(np.int32)
    emissive = np.any(v["mesh_f"][:, 3:6] != 0, axis=1)
    every = {int(m): rest["mesh_matrix"][m] for m in np.flatnonzero(~emissive)}
    one = {args.mesh: rest["mesh_matrix"][args.mesh]}
    assert not emissive[args.mesh]

    def cover(meshes):
        own = np.flatnonzero(np.isin(mesh_of, list(meshes)))
        span = np.arange(own[0], own[-1] + 1)
        return runs_of(span[~emissive[mesh_of[span]]]), len(own)

    stream = torch.cuda.current_stream().cuda_stream

    def old(poses, runs):
        tri, attr, _ = rt.pose_view(v, rest["rest"], poses)
        for first, n in runs:
            d_tri = torch.from_numpy(tri[first:first + n]).cuda()
            d_attr = torch.from_numpy(attr[first:first + n]).cuda()
            scene.update_triangles(first, d_tri, attr=d_attr, device=0, stream_ptr=stream)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return round(a.elapsed_time(b), 4), round((time.perf_counter() - t0) * 1e3, 4)

    runs_all, n_all = cover(every)
    runs_one, n_one = cover(one)
    base = {"what": "pose_time", "label": args.label, "commit": args.commit or commit(), "scene": args.scene,
            "n_tris": int(len(v["tri"])), "n_nodes": int(len(v["node"])), "levels": int(v["bvh_depth"]) + 1,
            "n_meshes": int(len(emissive)), "all_meshes": len(every), "all_tris": n_all, "all_cover": int(sum(n for _, n in runs_all)),
            "all_old_calls": len(runs_all), "one_mesh": args.mesh, "one_tris": n_one, "one_cover": int(sum(n for _, n in runs_one)),
            "one_old_calls": len(runs_one), "lib": os.environ.get("RT_LIB", "default")}
    scene.pose(every)   # warm-up: the plan, the kernels' first launch
    old(one, runs_one)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for rep in range(args.reps):
            rec = dict(base, rep=rep)
            for tag, poses, runs in (("all", every, runs_all), ("one", one, runs_one)):
                rec[f"pose_{tag}_ms"], rec[f"pose_{tag}_wall_ms"] = timed(lambda: scene.pose(poses))
                rec[f"old_{tag}_ms"], rec[f"old_{tag}_wall_ms"] = timed(lambda: old(poses, runs))
                _, rec[f"twin_{tag}_wall_ms"] = timed(lambda: twin.pose(poses))
            line = json.dumps(rec)
            f.write(line + "\n")
            print(line, flush=True)
    # the arrays after all of it are still the loader's
    d = scene.read_device()
    for k in ("tri", "tri_attr", "node"):
        assert np.array_equal(d[k].view(np.uint32), v[k].view(np.uint32)), k


if __name__ == "__main__":
    main()
