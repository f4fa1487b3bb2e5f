#!/usr/bin/env python3
"""What the denoiser's variance-guided mode costs and gains (one GPU).  Appends JSON lines to
profiles/denoise_guided_passes.jsonl:

  kernels  on the headline frame (sponza proxy 1920x1080), HIP-event times, best of --reps after a
           warm-up, all in one session: rt_denoise_device at 5 iterations; rt_denoise_guided_device
           at 0 .. 5 iterations, with the clamp off, and with a caller's variance in place of the
           estimate (so the clamp, the variance estimate and each level are differences of two
           totals); and the 8-sample rt_accum_add the filter is compared with.  RT_LIB selects
           another build.  (The kernels_ab rows of the profile are this mode on the tree and on an
           A/B build with plain loads in place of LDS staging; its compile-time switch was deleted
           with the losing path, so the plain rows cannot be reproduced from this tree.)
  quality  RMSE and brightness of raw, plain (rt_denoise) and guided frames against a converged
           frame: the headline at 8 and 16 samples against 256, cornell 64x64, sponza_mini 64x36 and
           cornell_blob 48x48 at 8 against 2048 (hit pixels with finite values, means clamped to
           [0, 4]; `mean_ratio` is the clamped frame's mean over the clamped truth's).  Default
           parameters.  The filters run on the device; their bits are the host functions'.

    python tools/denoise_guided_passes.py kernels|quality [--label NAME] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from denoise_passes import commit, timed  # noqa: E402

SMALL = [("cornell", 64, 64), ("sponza_mini", 64, 36), ("cornell_blob", 48, 48)]


def on_device(torch, rt, sums, spp, rec, guided):
    h, w = sums.shape[:2]
    d_s, d_g = torch.from_numpy(np.ascontiguousarray(sums)).cuda(), torch.from_numpy(np.ascontiguousarray(rec)).cuda()
    d_o = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    fn = rt.denoise_guided_device if guided else rt.denoise_device
    fn(d_s.data_ptr(), 0, spp, w, h, d_g.data_ptr(), d_o.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_o.cpu().numpy()


def quality_rows(torch, rt, scene, name, spps, truth_spp):
    g = scene.gbuffer()
    rec = g["records"]
    truth = scene.render_sums(truth_spp)[0] * (np.float32(1) / np.float32(truth_spp))
    rows = []
    for spp in spps:
        sums = scene.render_sums(spp)[0]
        frames = {"raw": sums * (np.float32(1) / np.float32(spp)), "plain": on_device(torch, rt, sums, spp, rec, False),
                  "guided": on_device(torch, rt, sums, spp, rec, True)}
        use = (g["prim"] >= 0) & np.isfinite(truth).all(-1)
        for x in frames.values():
            use = use & np.isfinite(x).all(-1)
        t = np.clip(truth[use].astype(np.float64), 0, 4)
        row = {"frame": name, "spp": spp, "truth_spp": truth_spp, "pixels": int(use.sum())}
        for k, x in frames.items():
            c = np.clip(x[use].astype(np.float64), 0, 4)
            row[f"rmse_{k}"] = round(float(np.sqrt(((c - t) ** 2).mean())), 5)
            row[f"mean_ratio_{k}"] = round(float(c.mean() / t.mean()), 4)
        row["guided_over_raw"] = round(row["rmse_guided"] / row["rmse_raw"], 4)
        row["plain_over_raw"] = round(row["rmse_plain"] / row["rmse_raw"], 4)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "quality"])
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--commit", default=None, help="the commit the figures come from (default: HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_guided_passes.jsonl"))
    args = ap.parse_args()
    path = bench.load_scenes_module().ensure_scene(args.scene, os.environ.get("RT_SCENE_DIR", "/tmp/rt_scenes"))
    W, H = args.width, args.height
    rec = {"what": args.what, "label": args.label, "commit": args.commit or commit(), "scene": args.scene, "width": W, "height": H,
           "lib": os.environ.get("RT_LIB", "default")}
    import torch  # (shares its HIP runtime with librt_hw_amd.so)
    rt = bench.import_pkg()
    rec["gpu"] = torch.cuda.get_device_name(0)
    scene = rt.Scene.load(path, W, H, 256)
    if args.what == "kernels":
        scene.upload(0)
        stream = torch.cuda.current_stream().cuda_stream
        d_g = torch.empty((H, W, 16), dtype=torch.float32, device="cuda")
        scene.gbuffer_device(d_g.data_ptr(), stream)
        acc = scene.accumulator()
        acc.add(8)   # warm-up
        acc.free()
        passes = []
        for _ in range(args.reps):
            acc = scene.accumulator()
            passes.append(acc.add(8)["render_ms"])
            sums = acc.sums()
            acc.free()
        rec["full_pass_8spp_ms"] = round(min(passes), 3)
        rec["full_pass_8spp_runs_ms"] = [round(x, 3) for x in passes]
        d_s = torch.from_numpy(sums).cuda()
        d_o = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        d_v = torch.rand((H, W), dtype=torch.float32, device="cuda")

        def plain():
            rt.denoise_device(d_s.data_ptr(), 0, 8, W, H, d_g.data_ptr(), d_o.data_ptr(), stream, iterations=5)

        def guided(**kw):
            return lambda: rt.denoise_guided_device(d_s.data_ptr(), 0, 8, W, H, d_g.data_ptr(), d_o.data_ptr(), stream, **kw)

        best, runs = timed(torch, plain, args.reps)
        rec.update(denoise_5_iterations_ms=round(best, 4), denoise_5_iterations_runs_ms=runs)
        totals = {}
        for it in range(0, 6):
            totals[it], runs = timed(torch, guided(iterations=it), args.reps)
            rec[f"guided_{it}_iterations_ms"] = round(totals[it], 4)
            rec[f"guided_{it}_iterations_runs_ms"] = runs
        no_clamp, runs = timed(torch, guided(iterations=5, firefly=-1.0), args.reps)
        rec.update(guided_5_no_clamp_ms=round(no_clamp, 4), guided_5_no_clamp_runs_ms=runs)
        given, runs = timed(torch, guided(iterations=5, d_variance_ptr=d_v.data_ptr()), args.reps)
        rec.update(guided_5_given_variance_ms=round(given, 4), guided_5_given_variance_runs_ms=runs)
        rec["clamp_ms_by_difference"] = round(totals[5] - no_clamp, 4)
        rec["variance_estimate_less_copy_ms_by_difference"] = round(totals[5] - given, 4)
        rec["level_ms_by_difference"] = [round(totals[k + 1] - totals[k], 4) for k in range(1, 5)]
        rec["prepare_clamp_variance_level0_resolve_ms"] = round(totals[1], 4)
        rec["guided_over_plain"] = round(totals[5] / best, 3)
        rec["guided_share_of_full_pass"] = round(totals[5] / min(passes), 4)
    else:
        rows = quality_rows(torch, rt, scene, f"{args.scene} {W}x{H}", (8, 16), 256)
        for name, w, h in SMALL:
            gltf = os.path.join(ROOT, "tests", "golden", "scenes", name, name + ".gltf")
            rows += quality_rows(torch, rt, rt.Scene.load(gltf, w, h, 8), f"{name} {w}x{h}", (8,), 2048)
        rec.update(quality=rows, parameters="defaults")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
