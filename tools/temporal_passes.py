#!/usr/bin/env python3
"""What the reprojected temporal history costs and gains.  Appends JSON lines to
profiles/temporal_passes.jsonl:

  kernels  on the headline frame (sponza proxy 1920x1080, one GPU), HIP-event times, the minimum of
           --reps (at least 3) timed runs after a warm-up: rt_history_push, and its two parts alone,
           the G-buffer launch (rt_gbuffer_device) and the temporal kernel (rt_temporal_device
           against a previous frame from a camera moved and turned a little); for scale, in the same
           run, rt_denoise_device at 4 and 5 iterations (a level's time is their difference)
  quality  cornell 64x64, 1 sample per frame, an 8-frame orbit of 1 degree per frame about the
           point the camera looks at: clamped RMSE (hit pixels with finite values, means clamped to
           [0, 4]) against a 256-sample render of the last view, of the raw last frame, the temporal
           result, and the temporal result through rt_denoise_guided with its spatial variance
           estimate and with the step's out_variance; default parameters, which are picked

    python tools/temporal_passes.py kernels|quality [--label NAME] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from denoise_passes import commit, rmse, timed  # noqa: E402


def orbit(cam, angle):
    """`cam` turned by `angle` radians about the vertical through the point it looks at (taken
    at the camera's distance from the origin along its forward axis)."""
    p, ax = np.asarray(cam["pos"], np.float64), np.asarray(cam["axes"], np.float64)
    target = p + ax[2] * np.linalg.norm(p)
    c, s = math.cos(angle), math.sin(angle)
    rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return {"pos": (target + rot @ (p - target)).astype(np.float32), "axes": (ax @ rot.T).astype(np.float32),
            "tan_half_fov": np.asarray(cam["tan_half_fov"], np.float32).copy()}


def kernels(rt, torch, args, rec):
    path = bench.load_scenes_module().ensure_scene(args.scene, os.environ.get("RT_SCENE_DIR", "/tmp/rt_scenes"))
    W, H, spp = args.width, args.height, 1
    rec.update(scene=args.scene, width=W, height=H)
    scene = rt.Scene.load(path, W, H, spp)
    scene.upload(0)
    stream = torch.cuda.current_stream().cuda_stream
    c0 = scene.camera()
    c1 = orbit(c0, math.radians(0.5))
    c1["pos"] = (c1["pos"] + np.float32(0.01) * c0["axes"][0]).astype(np.float32)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")   # noqa: E731
    d_g0, d_g1, d_h0, d_h1, d_mean, d_var = new(H, W, 16), new(H, W, 16), new(3, H, W, 4), new(3, H, W, 4), new(H, W, 3), new(H, W)
    # the previous frame (camera c0) and the new one (camera c1)
    d_s0 = torch.from_numpy(scene.render_sums(spp)[0]).cuda()
    scene.gbuffer_device(d_g0.data_ptr(), stream)
    rt.temporal_device(d_s0.data_ptr(), 0, spp, W, H, d_g0.data_ptr(), d_h0.data_ptr(), stream_ptr=stream)
    scene.set_camera(**c1)
    d_s1 = torch.from_numpy(scene.render_sums(spp)[0]).cuda()
    best, runs = timed(torch, lambda: scene.gbuffer_device(d_g1.data_ptr(), stream), args.reps)
    rec.update(gbuffer_ms=round(best, 4), gbuffer_runs_ms=runs)
    best, runs = timed(torch, lambda: rt.temporal_device(d_s1.data_ptr(), 0, spp, W, H, d_g1.data_ptr(), d_h1.data_ptr(), d_mean.data_ptr(),
                                                         d_var.data_ptr(), cam_prev=c0, d_gbuffer_prev_ptr=d_g0.data_ptr(),
                                                         d_history_prev_ptr=d_h0.data_ptr(), stream_ptr=stream), args.reps)
    rec.update(temporal_kernel_ms=round(best, 4), temporal_kernel_runs_ms=runs)
    torch.cuda.synchronize()
    n = d_h1[0, :, :, 3].cpu().numpy()
    rec["pixels_with_history"] = round(float((n >= 2).mean()), 4)
    first, _ = timed(torch, lambda: rt.temporal_device(d_s1.data_ptr(), 0, spp, W, H, d_g1.data_ptr(), d_h1.data_ptr(), d_mean.data_ptr(),
                                                       d_var.data_ptr(), stream_ptr=stream), args.reps)
    rec["temporal_kernel_first_frame_ms"] = round(first, 4)
    hist = scene.history()
    cams = [c0, c1]

    def push():   # (alternating cameras: every timed push has a history to look up)
        cams.reverse()
        scene.set_camera(**cams[0])
        hist.push(d_s1.data_ptr(), 0, spp, d_mean.data_ptr(), d_var.data_ptr(), stream)

    best, runs = timed(torch, push, args.reps)
    rec.update(history_push_ms=round(best, 4), history_push_runs_ms=runs)
    d_o = new(H, W, 3)
    totals = {}
    for it in (4, 5):
        totals[it], runs = timed(torch, lambda: rt.denoise_device(d_mean.data_ptr(), 0, 1, W, H, d_g1.data_ptr(), d_o.data_ptr(), stream,
                                                                  iterations=it), args.reps)
        rec[f"denoise_{it}_iterations_ms"] = round(totals[it], 4)
    rec["denoise_level_ms_by_difference"] = round(totals[5] - totals[4], 4)
    rec["denoise_level_ms_mean_of_5"] = round(totals[5] / 5, 4)
    rec["temporal_kernel_in_levels"] = round(rec["temporal_kernel_ms"] / max(totals[5] - totals[4], 1e-6), 3)
    rec["bytes_per_pixel_estimate"] = 230
    rec["temporal_kernel_GBps_at_230B"] = round(230.0 * W * H / (rec["temporal_kernel_ms"] * 1e-3) / 1e9, 1)
    hist.free()


def quality(rt, args, rec):
    W = H = 64
    path = os.path.join(ROOT, "tests", "golden", "scenes", "cornell", "cornell.gltf")
    scene = rt.Scene.load(path, W, H, 1)
    c0 = scene.camera()
    hist, prev = None, None
    for k in range(8):
        cam = orbit(c0, math.radians(1.0 * k))
        scene.set_camera(**cam)
        frame, g = scene.render_sums(1)[0], scene.gbuffer()["records"]
        hist, mean, var = rt.temporal(frame, 1, g, prev[0] if prev else None, prev[1] if prev else None, hist)
        prev = (cam, g)
    truth = scene.render_sums(256)[0] * (np.float32(1) / np.float32(256))
    outs = {"raw_last_frame": frame, "temporal": mean, "temporal_guided_spatial_variance": rt.denoise_guided(mean, 1, g),
            "temporal_guided_out_variance": rt.denoise_guided(mean, 1, g, variance=var), "guided_alone": rt.denoise_guided(frame, 1, g)}
    use = (g.view(np.int32)[..., 7] >= 0) & np.isfinite(truth).all(-1)
    for x in outs.values():
        use = use & np.isfinite(x).all(-1)
    rec.update(scene="cornell", width=W, height=H, frames=8, degrees_per_frame=1.0, spp_per_frame=1, truth_spp=256,
               pixels=int(use.sum()), history_lengths_mean=round(float(hist[0][..., 3][use].mean()), 3),
               rmse={k: round(rmse(x, truth, use), 5) for k, x in outs.items()}, parameters="defaults (picked, not measured)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "quality"])
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--commit", default=None, help="the commit the figures come from (default: HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_passes.jsonl"))
    args = ap.parse_args()
    args.reps = max(args.reps, 3)
    rec = {"what": args.what, "label": args.label, "commit": args.commit or commit(), "lib": os.environ.get("RT_LIB", "default")}
    import torch  # (shares its HIP runtime with librt_hw_amd.so)
    rt = bench.import_pkg()
    rec["gpu"] = torch.cuda.get_device_name(0)
    if args.what == "kernels":
        kernels(rt, torch, args, rec)
    else:
        quality(rt, args, rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
