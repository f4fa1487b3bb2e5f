#!/usr/bin/env python3
"""What the first-hit feature buffer and the frame denoiser cost and gain, on the headline frame
(sponza proxy 1920x1080, one GPU).  Appends JSON lines to profiles/denoise_passes.jsonl:

  full     an 8-sample rt_accum_add on a fresh accumulator, --reps times after one warm-up (the
           preview step the filter is compared with, and the full-pass regression figure: run it
           with --pkg-dir on the parent's build and without on this one in the same session)
  kernels  HIP-event times, best of --reps after a warm-up: rt_gbuffer_device, and
           rt_denoise_device at 1 .. 5 iterations (a level's time is the difference of two
           totals; iterations = 0 is prepare-free: the mean only).  RT_LIB selects another build.
           (The plain_* rows of the profile came from an A/B build with plain loads at strides 1
           and 2; its compile-time switch was deleted with the losing path, so those rows cannot
           be reproduced from this tree.)
  quality  RMSE against the 256-sample frame for 8 and 16 samples, raw and denoised (hit pixels
           with finite values, means clamped to [0, 4]); default parameters, which are picked,
           not tuned

    python tools/denoise_passes.py full|kernels|quality [--label NAME] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

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


def timed(torch, fn, reps):
    """Best and all of `reps` HIP-event times of fn() in ms, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), [round(x, 4) for x in ms]


def rmse(x, truth, use):
    d = np.clip(x[use].astype(np.float64), 0, 4) - np.clip(truth[use].astype(np.float64), 0, 4)
    return float(np.sqrt((d * d).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["full", "kernels", "quality"])
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--pkg-dir", default=None, help="full: a directory holding another build's __init__.py and "
                                                      "librt_hw_amd.so (the parent's, whose library lacks the new symbols)")
    ap.add_argument("--commit", default=None, help="the commit the figures come from (default: HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_passes.jsonl"))
    args = ap.parse_args()
    path = bench.load_scenes_module().ensure_scene(args.scene, os.environ.get("RT_SCENE_DIR", "/tmp/rt_scenes"))
    W, H = args.width, args.height
    rec = {"what": args.what, "label": args.label, "commit": args.commit or commit(), "scene": args.scene, "width": W,
           "height": H, "lib": os.environ.get("RT_LIB", "default")}
    import torch  # (shares its HIP runtime with librt_hw_amd.so)
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
    if args.what == "full":
        ms, st = full_pass(scene, args.reps)
        rec.update(full_pass_8spp_ms=[round(x, 3) for x in ms], mean_ms=round(float(np.mean(ms)), 3),
                   spread_ms=round(max(ms) - min(ms), 3), schedule=st["schedule"])
    elif args.what == "kernels":
        scene.upload(0)
        stream = torch.cuda.current_stream().cuda_stream
        d_g = torch.empty((H, W, 16), dtype=torch.float32, device="cuda")
        best, runs = timed(torch, lambda: scene.gbuffer_device(d_g.data_ptr(), stream), args.reps)
        rec.update(gbuffer_ms=round(best, 4), gbuffer_runs_ms=runs)
        acc = scene.accumulator()
        st = acc.add(8)
        rec["full_pass_8spp_ms"] = round(st["render_ms"], 3)
        d_s = torch.from_numpy(acc.sums()).cuda()
        acc.free()
        d_o = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        totals = {}
        for it in range(0, 6):
            best, runs = timed(torch, lambda: rt.denoise_device(d_s.data_ptr(), 0, 8, W, H, d_g.data_ptr(), d_o.data_ptr(),
                                                                 stream, iterations=it), args.reps)
            totals[it] = best
            rec[f"denoise_{it}_iterations_ms"] = round(best, 4)
            rec[f"denoise_{it}_iterations_runs_ms"] = runs
        rec["level_ms_by_difference"] = [round(totals[k + 1] - totals[k], 4) for k in range(1, 5)]
        rec["prepare_level0_resolve_ms"] = round(totals[1], 4)
        rec["denoise_share_of_preview_step"] = round(totals[5] / (totals[5] + st["render_ms"]), 4)
    else:
        g = scene.gbuffer()
        truth = scene.render_sums(256)[0] * (np.float32(1) / np.float32(256))
        rows = []
        for spp in (8, 16):
            sums = scene.render_sums(spp)[0]
            raw = sums * (np.float32(1) / np.float32(spp))
            den = rt.denoise(sums, spp, g)
            use = (g["prim"] >= 0) & np.isfinite(raw).all(-1) & np.isfinite(den).all(-1) & np.isfinite(truth).all(-1)
            a, b = rmse(raw, truth, use), rmse(den, truth, use)
            rows.append({"spp": spp, "rmse_raw": round(a, 5), "rmse_denoised": round(b, 5), "ratio": round(b / a, 4),
                         "pixels": int(use.sum())})
        rec.update(truth_spp=256, quality=rows, parameters="defaults (picked, not tuned)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
