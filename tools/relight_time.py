#!/usr/bin/env python3
"""What moving lights costs (include/rt_hw.h rt_scene_enable_light_updates).  On one GPU it takes, per
repetition, the HIP-event time (and the wall time) through the device entry
(rt_scene_update_tris_device) of

  a  practice6_1 (1,152 lights, 777 light nodes): its emissive mesh through the covering range, one
     call: the triangle scatter, the node refit, the light scatter, one launch per light-tree level,
     and the read-back of the range, the node array and both light arrays
  b  the headline scene (sponza proxy): every triangle as ONE call on the opted-in scene, against the
     calls around the light's triangles that a scene without the opt-in needs (refit_time.py's a)
  c  the headline scene: a range without a light triangle (the largest non-emissive mesh's covering
     range, cut at the emissive ones) without and with the opt-in: the same kernels are launched

and appends one JSON line per repetition to profiles/relight_time.jsonl.  The records moved are the
scene's own (every repetition works on the same geometry).

    python tools/relight_time.py [--reps N] [--label NAME] [--out FILE]
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
    ap.add_argument("--label", default="tree")
    ap.add_argument("--commit", default=None, help="the commit the figures come from (default: HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relight_time.jsonl"))
    args = ap.parse_args()
    path = bench.load_scenes_module().ensure_scene(args.scene, os.environ.get("RT_SCENE_DIR", "/tmp/rt_scenes"))
    import torch  # (shares its HIP runtime with librt_hw_amd.so)
    torch.zeros(1, device="cuda")
    rt = bench.import_pkg()
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return round(a.elapsed_time(b), 4), round((time.perf_counter() - t0) * 1e3, 4)

    def opened(scene_path, w, h):
        scene = rt.Scene.load(scene_path, w, h, 1)
        scene.upload(0)
        v = scene.view()
        d_tri = torch.from_numpy(v["tri"]).cuda()
        torch.cuda.synchronize()

        def update(runs):
            for first, n in runs:
                scene.update_triangles(first, d_tri[first:first + n], device=0, stream_ptr=stream)
        return scene, v, update

    # a: practice6_1
    small, sv, small_update = opened(os.path.join(ROOT, "tests", "golden", "scenes", "practice6_1", "practice6_1.gltf"), 24, 16)
    small.enable_light_updates()
    s_mesh_of = sv["tri_attr"][:, 15].view(np.int32)
    s_lit = np.any(sv["mesh_f"][:, 3:6] != 0, axis=1)[s_mesh_of]
    s_ids = np.flatnonzero(s_lit)
    a_run = [(int(s_ids[0]), int(s_ids[-1] - s_ids[0] + 1))]
    # b, c: the headline scene, first as it is, then opted in
    scene, v, update = opened(path, 64, 36)
    mesh_of = v["tri_attr"][:, 15].view(np.int32)
    emissive = np.any(v["mesh_f"][:, 3:6] != 0, axis=1)
    around = runs_of(np.flatnonzero(~emissive[mesh_of]))
    whole = [(0, len(v["tri"]))]
    mesh = int(np.argmax(np.bincount(mesh_of, minlength=len(emissive)) * ~emissive))
    own = np.flatnonzero(mesh_of == mesh)
    span = np.arange(own[0], own[-1] + 1)
    part = runs_of(span[~emissive[mesh_of[span]]])
    base = {"what": "relight_time", "label": args.label, "commit": args.commit or commit(), "lib": os.environ.get("RT_LIB", "default"),
            "a_scene": "practice6_1", "a_first": a_run[0][0], "a_tris": a_run[0][1], "a_lights": int(len(sv["light"])),
            "a_light_nodes": int(len(sv["light_node"])), "a_light_levels": int(sv["light_bvh_depth"]) + 1,
            "a_launches": int(sv["bvh_depth"]) + 2 + int(sv["light_bvh_depth"]) + 2,
            "scene": args.scene, "n_tris": int(len(v["tri"])), "n_lights": int(len(v["light"])), "levels": int(v["bvh_depth"]) + 1,
            "light_levels": int(v["light_bvh_depth"]) + 1, "b_around_calls": len(around), "b_around_tris": int(sum(n for _, n in around)),
            "b_one_call_tris": whole[0][1], "b_one_call_launches": int(v["bvh_depth"]) + 2 + int(v["light_bvh_depth"]) + 2,
            "c_mesh": mesh, "c_calls": len(part), "c_tris": int(sum(n for _, n in part)), "c_launches_per_call": int(v["bvh_depth"]) + 2}
    small_update(a_run)   # warm-ups: the plans, the small allocation, the kernels' first launch
    update(around)
    update(part)
    torch.cuda.synchronize()
    before = [timed(lambda: update(around)) + timed(lambda: update(part)) for _ in range(args.reps)]
    scene.enable_light_updates()
    update(whole)
    update(part)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for rep in range(args.reps):
            a_ms, a_wall = timed(lambda: small_update(a_run))
            b_ms, b_wall = timed(lambda: update(whole))
            c_ms, c_wall = timed(lambda: update(part))
            rec = dict(base, rep=rep, a_lights_ms=a_ms, a_lights_wall_ms=a_wall, b_around_ms=before[rep][0], b_around_wall_ms=before[rep][1],
                       b_one_call_ms=b_ms, b_one_call_wall_ms=b_wall, c_without_ms=before[rep][2], c_without_wall_ms=before[rep][3],
                       c_with_ms=c_ms, c_with_wall_ms=c_wall)
            line = json.dumps(rec)
            f.write(line + "\n")
            print(line, flush=True)
    # the arrays after all of it are still the loader's
    for s, w in ((small, sv), (scene, v)):
        d = s.read_device_lights()
        assert np.array_equal(s.read_device()["node"].view(np.uint32), w["node"].view(np.uint32))
        assert np.array_equal(d["light"].view(np.uint32), w["light"].view(np.uint32))
        assert np.array_equal(d["light_node"].view(np.uint32), w["light_node"].view(np.uint32))


if __name__ == "__main__":
    main()
