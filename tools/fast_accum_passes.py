#!/usr/bin/env python3
"""What fast-mode accumulators cost and gain, on the headline frame (sponza proxy 1920x1080, one
GPU).  Appends JSON lines to profiles/fast_accum_passes.jsonl:

  regress   the one-shot parity frame and the one-shot fast frame(s) (--fast-spp, default 256),
            --reps times each after one warm-up (run it with --pkg-dir on the parent's build,
            without on this one, then on the parent's again, in one session)
  overhead  the fast accumulator (--chunk, default 2) at 256 spp as 1 x 256, 4 x 64 and 16 x 16:
            the passes' render_ms summed, against the one-shot fast render of 256 and of each
            pass's sample count in the same process
  subset    after add(8), 8 more samples (a) under a random 25% mask and (b) in a centred
            50% x 50% window, on the fast accumulator and on the parity accumulator: ms,
            samples/s, and each mode's ratio to its own full pass of 8 samples; for the fast
            lists the share of queue items that start nothing (units past their pixel's own)
  cli       rt_solution with RT_ADAPT (max 256, step 16, --threshold) with and without
            RT_FAST=<chunk>: rounds, samples spent, wall time

    python tools/fast_accum_passes.py regress|overhead|subset|cli [--label NAME] [--out FILE]
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


def timed(fn, reps):
    """fn() -> stats; one warm-up, then `reps` render_ms."""
    fn()
    return [round(fn()["render_ms"], 3) for _ in range(reps)]


def spread(ms):
    return {"ms": ms, "mean_ms": round(float(np.mean(ms)), 3), "spread_ms": round(max(ms) - min(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["regress", "overhead", "subset", "cli"])
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=2)
    ap.add_argument("--fast-spp", default="256", help="regress: the one-shot fast frames' sample counts")
    ap.add_argument("--threshold", type=float, default=0.25)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--pkg-dir", default=None, help="regress: a directory holding another build's __init__.py and "
                                                      "librt_hw_amd.so (the parent's, whose library lacks the new symbols)")
    ap.add_argument("--commit", default=None, help="the commit the figures come from (default: HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fast_accum_passes.jsonl"))
    args = ap.parse_args()
    path = bench.load_scenes_module().ensure_scene(args.scene, os.environ.get("RT_SCENE_DIR", "/tmp/rt_scenes"))
    W, H, c = args.width, args.height, args.chunk
    rec = {"what": args.what, "label": args.label, "commit": args.commit or commit(), "scene": args.scene, "width": W,
           "height": H, "lib": os.environ.get("RT_LIB", "default")}
    if args.what == "cli":
        exe = os.path.join(ROOT, "raytracing-hw_amd", "rt_solution")
        out = "/tmp/fast_accum_passes"
        os.makedirs(out, exist_ok=True)
        cnt = os.path.join(out, "counts.pgm")
        rec.update(threshold=args.threshold, max_spp=256, step=16, chunk=c)
        for name, env_add in (("parity", {}), ("fast", {"RT_FAST": str(c)})):
            env = {k: v for k, v in os.environ.items() if k not in ("RT_CHECKPOINT", "RT_FAST")}
            env.update(RT_GPUS="1", RT_PASS_SPP="16", RT_ADAPT=str(args.threshold), RT_COUNTS_OUT=cnt, **env_add)
            t0 = time.perf_counter()
            r = subprocess.run([exe, path, str(W), str(H), "256", os.path.join(out, "frame.ppm")], env=env,
                               capture_output=True, text=True, check=True)
            wall = time.perf_counter() - t0
            rounds = [(int(a), int(b)) for a, b in re.findall(r"refined (\d+) pixels to (\d+) samples", r.stdout)]
            data = open(cnt, "rb").read()
            counts = np.frombuffer(data, ">u2", W * H, len(data) - 2 * W * H).astype(np.int64)
            rec[name] = {"rounds": len(rounds), "refined_per_round": [a for a, _ in rounds], "samples": int(counts.sum()),
                         "samples_share": round(float(counts.sum()) / (256 * W * H), 4), "count_min": int(counts.min()),
                         "count_max": int(counts.max()), "wall_s": round(wall, 3)}
        rec["note"] = "wall times include scene loading; image quality not evaluated"
    else:
        import torch  # noqa: F401  (shares its HIP runtime with librt_hw_amd.so)
        if args.pkg_dir:
            import importlib.util
            spec = importlib.util.spec_from_file_location("rt_other", os.path.join(args.pkg_dir, "__init__.py"))
            rt = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(rt)
            rec["lib"] = os.path.relpath(rt.LIB_PATH, ROOT)
        else:
            rt = bench.import_pkg()
        rec["gpu"] = torch.cuda.get_device_name(0)
        scene = rt.Scene.load(path, W, H, 256)
        one_shot_fast = lambda n: spread(timed(lambda: scene.render_sums(n, fast=True, fast_chunk=c)[1], args.reps))
        if args.what == "regress":
            rec["parity_256"] = spread(timed(lambda: scene.render_sums(256)[1], args.reps))
            for n in (int(x) for x in args.fast_spp.split(",")):
                rec[f"fast_{n}"] = one_shot_fast(n)
        elif args.what == "overhead":
            rec["chunk"] = c
            shots = {n: one_shot_fast(n) for n in (256, 64, 16)}
            rec["one_shot_fast"] = {str(n): v for n, v in shots.items()}
            for k, n in ((1, 256), (4, 64), (16, 16)):
                def passes():
                    acc = scene.accumulator(fast=True, fast_chunk=c)
                    ms = [acc.add(n)["render_ms"] for _ in range(k)]
                    acc.free()
                    return {"render_ms": sum(ms)}
                t = spread(timed(passes, args.reps))
                t["ratio_to_one_shot_256"] = round(min(t["ms"]) / min(shots[256]["ms"]), 4)
                t["ratio_to_passes_as_one_shots"] = round(min(t["ms"]) / (k * min(shots[n]["ms"])), 4)
                rec[f"{k}x{n}"] = t
        else:
            rec["chunk"] = c
            mask = (np.random.default_rng(1).random((H, W)) < 0.25).astype(np.uint8)
            window = (W // 4, H // 4, W // 4 + W // 2, H // 4 + H // 2)
            for mode, kw_acc in (("fast", dict(fast=True, fast_chunk=c)), ("parity", {})):
                def full():
                    acc = scene.accumulator(**kw_acc)
                    st = acc.add(8)
                    acc.free()
                    return st
                ms = timed(full, args.reps)
                full_rate = W * H * 8 / (min(ms) * 1e-3)
                res = {"full_pass_8spp": spread(ms), "full_pass_samples_per_s": round(full_rate)}
                for name, kw in (("mask_25pct", dict(mask=mask)), ("window_50x50", dict(window=window))):
                    runs = []
                    for _ in range(args.reps + 1):   # (the first is the warm-up)
                        acc = scene.accumulator(**kw_acc)
                        acc.add(8)
                        n = acc.select(16, **kw)
                        s = acc.add_selected()
                        assert s["pixels"] == n and s["samples"] == 8 * n
                        runs.append(s)
                        acc.free()
                    runs = runs[1:]
                    best = min(r["render_ms"] for r in runs)
                    rate = runs[0]["samples"] / (best * 1e-3)
                    res[name] = {"pixels": runs[0]["pixels"], "samples": runs[0]["samples"],
                                 "render_ms": [round(r["render_ms"], 3) for r in runs], "samples_per_s": round(rate),
                                 "ratio_to_full_pass": round(rate / full_rate, 4), "schedule": runs[0]["schedule"],
                                 # (every listed pixel starts at 8: all have the same units, none starts nothing)
                                 "noop_item_share": 0.0}
                rec[mode] = res
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
