#!/usr/bin/env python3
"""What progressive passes cost: the headline frame (sponza proxy 1920x1080x256, one GPU) as one
shot (rt_render_device), as 4 x 64 passes and as 16 x 16 passes of an accumulator
(rt_accum_add).  Each pass has its own tail, and from 128 samples its own order pre-pass, so
passes cost more than one shot; this measures how much, next to a one-shot render of the
pass's own sample count (the cost of a short render as such).  Same bits in all three (sha1 of the
float sums).  Writes profiles/accum_ab.json (per-pass render_ms and order_ms).

    python tools/accum_ab.py [--reps 3] [--out profiles/accum_ab.json]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--splits", default="4,16", help="numbers of equal passes to time")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_ab.json"))
    args = ap.parse_args()
    rt = bench.import_pkg()
    path = bench.load_scenes_module().ensure_scene(args.scene, os.environ.get("RT_SCENE_DIR", "/tmp/rt_scenes"))
    W, H, S = args.width, args.height, args.spp
    scene = rt.Scene.load(path, W, H, S)
    scene.upload(0)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    res = {"scene": args.scene, "width": W, "height": H, "spp": S, "reps": args.reps,
           "lib": os.environ.get("RT_LIB", "default"), "gpu": torch.cuda.get_device_name(0)}

    scene.render_device(out.data_ptr(), stream, spp=S, stats=True)   # warm
    one = [scene.render_device(out.data_ptr(), stream, spp=S, stats=True) for _ in range(args.reps)]
    torch.cuda.synchronize()
    res["one_shot"] = {"render_ms": [round(st["render_ms"], 2) for st in one],
                       "order_ms": [round(st["order_ms"], 2) for st in one],
                       "sha1": hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:16]}
    best = min(st["render_ms"] for st in one)
    for k in [int(x) for x in args.splits.split(",")]:
        n = S // k
        assert n * k == S, "splits must divide spp"
        runs = []
        for _ in range(args.reps):
            acc = scene.accumulator()
            sts = [acc.add(n) for _ in range(k)]
            runs.append({"render_ms": [round(st["render_ms"], 2) for st in sts],
                         "order_ms": [round(st["order_ms"], 2) for st in sts],
                         "total_ms": round(sum(st["render_ms"] for st in sts), 2)})
            sums = acc.sums()
            acc.free()
        tot = min(r["total_ms"] for r in runs)
        # a one-shot render of the pass's own sample count: what a pass costs without the accumulator
        alone = [scene.render_device(out.data_ptr(), stream, spp=n, stats=True)["render_ms"] for _ in range(args.reps)]
        res[f"passes_{k}x{n}"] = {"runs": runs, "best_total_ms": tot, "over_one_shot": round(tot / best, 4),
                                  "one_shot_at_pass_spp_ms": [round(x, 2) for x in alone],
                                  "sha1": hashlib.sha1(np.ascontiguousarray(sums).tobytes()).hexdigest()[:16]}
    res["one_shot"]["best_ms"] = round(best, 2)
    res["same_bits"] = len({v["sha1"] for v in res.values() if isinstance(v, dict) and "sha1" in v}) == 1
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "runs"})
                      for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
