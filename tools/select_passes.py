#!/usr/bin/env python3
"""What subset passes cost, on the headline frame (sponza proxy 1920x1080, one GPU).  Appends
JSON lines to profiles/select_passes.jsonl:

  full     an 8-sample rt_accum_add on a fresh accumulator, --reps times after one warm-up (the
           full-pass regression figure: run it with --pkg-dir on the parent's build and without
           on this one in the same session)
  subset   after add(8), 8 more samples (a) under a random 25% mask and (b) in a centred
           50% x 50% window: ms, samples/s, the ratio to the full pass's samples/s of the same
           call, the schedule chosen; no threshold
  cli      rt_solution with RT_ADAPT (max 256, step 16, --threshold) against the uniform
           256-spp progressive run (RT_PASS_SPP=16): rounds, samples spent, wall time

    python tools/select_passes.py full|subset|cli [--label NAME] [--out FILE]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def commit():
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
    return r.stdout.strip() or "unknown"


def full_pass(scene, reps):
    acc = scene.accumulator()
    acc.add(8)   # warm-up: first launch of the CHAIN kernels, workspace
    acc.free()
    ms = []
    for _ in range(reps):
        acc = scene.accumulator()
        st = acc.add(8)
        ms.append(st["render_ms"])
        acc.free()
    return ms, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["full", "subset", "cli"])
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.25)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--pkg-dir", default=None, help="full: a directory holding another build's __init__.py and "
                                                      "librt_hw_amd.so (the parent's, whose library lacks the new symbols)")
    ap.add_argument("--commit", default=None, help="the commit the figures come from (default: HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_passes.jsonl"))
    args = ap.parse_args()
    path = bench.load_scenes_module().ensure_scene(args.scene, os.environ.get("RT_SCENE_DIR", "/tmp/rt_scenes"))
    W, H = args.width, args.height
    rec = {"what": args.what, "label": args.label, "commit": args.commit or commit(), "scene": args.scene, "width": W,
           "height": H, "lib": os.environ.get("RT_LIB", "default")}
    if args.what == "cli":
        exe = os.path.join(ROOT, "raytracing-hw_amd", "rt_solution")
        out = "/tmp/select_passes"
        os.makedirs(out, exist_ok=True)

        def run(**env_add):
            env = {k: v for k, v in os.environ.items() if k not in ("RT_ADAPT", "RT_COUNTS_OUT", "RT_CHECKPOINT")}
            env.update(RT_GPUS="1", RT_PASS_SPP="16", **env_add)
            t0 = time.perf_counter()
            r = subprocess.run([exe, path, str(W), str(H), "256", os.path.join(out, "frame.ppm")], env=env,
                               capture_output=True, text=True, check=True)
            return time.perf_counter() - t0, r.stdout

        uniform_s, _ = run()
        cnt = os.path.join(out, "counts.pgm")
        adaptive_s, stdout = run(RT_ADAPT=str(args.threshold), RT_COUNTS_OUT=cnt)
        rounds = [(int(a), int(b)) for a, b in re.findall(r"refined (\d+) pixels to (\d+) samples", stdout)]
        data = open(cnt, "rb").read()
        counts = np.frombuffer(data, ">u2", W * H, len(data) - 2 * W * H).astype(np.int64)
        rec.update(threshold=args.threshold, max_spp=256, step=16, rounds=len(rounds), refined_per_round=[a for a, _ in rounds],
                   samples=int(counts.sum()), uniform_samples=256 * W * H,
                   samples_share=round(float(counts.sum()) / (256 * W * H), 4), count_min=int(counts.min()),
                   count_max=int(counts.max()), wall_s_adaptive=round(adaptive_s, 3), wall_s_uniform_progressive=round(uniform_s, 3),
                   note="wall times include scene loading; image quality against the uniform frame not evaluated")
    else:
        import torch  # noqa: F401  (shares its HIP runtime with librt_hw_amd.so)
        if args.pkg_dir:
            import importlib.util
            spec = importlib.util.spec_from_file_location("rt_other", os.path.join(args.pkg_dir, "__init__.py"))
            rt = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(rt)
            rec["lib"] = rt.LIB_PATH
        else:
            rt = bench.import_pkg()
        rec["gpu"] = torch.cuda.get_device_name(0)
        scene = rt.Scene.load(path, W, H, 256)
        ms, st = full_pass(scene, args.reps)
        full_rate = W * H * 8 / (min(ms) * 1e-3)
        rec.update(full_pass_8spp_ms=[round(x, 3) for x in ms], mean_ms=round(float(np.mean(ms)), 3),
                   spread_ms=round(max(ms) - min(ms), 3), schedule=st["schedule"])
        if args.what == "subset":
            mask = (np.random.default_rng(1).random((H, W)) < 0.25).astype(np.uint8)
            window = (W // 4, H // 4, W // 4 + W // 2, H // 4 + H // 2)
            for name, kw in (("mask_25pct", dict(mask=mask)), ("window_50x50", dict(window=window))):
                runs = []
                for _ in range(args.reps):
                    acc = scene.accumulator()
                    acc.add(8)
                    n = acc.select(16, **kw)
                    s = acc.add_selected()
                    assert s["pixels"] == n and s["samples"] == 8 * n
                    runs.append(s)
                    acc.free()
                best = min(r["render_ms"] for r in runs)
                rate = runs[0]["samples"] / (best * 1e-3)
                rec[name] = {"pixels": runs[0]["pixels"], "samples": runs[0]["samples"],
                             "render_ms": [round(r["render_ms"], 3) for r in runs], "samples_per_s": round(rate),
                             "ratio_to_full_pass": round(rate / full_rate, 4), "schedule": runs[0]["schedule"]}
            rec["full_pass_samples_per_s"] = round(full_rate)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
