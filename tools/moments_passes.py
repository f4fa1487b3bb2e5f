#!/usr/bin/env python3
"""What per-sample second moments cost and gain, on the headline frame (sponza proxy 1920x1080, one
GPU).  Appends JSON lines to profiles/moments_passes.jsonl:

  cost      16 samples as 4 passes of 4 on a fast accumulator (--chunk, default 2) with and without
            moments, the same build, alternating runs: the passes' render_ms summed (HIP events
            inside the library), best of --reps after a warm-up of each.  The plain fast path is
            untouched code, so it is the baseline.  RT_LIB selects another build (the A/B of where
            the second partial lives: make variant VFLAGS=-DRT_MOMENT_HOME=n, while that switch
            existed).
  variance  rt_variance_from_moments_device on the accumulator's own device buffers: HIP-event
            time, best of --reps after a warm-up.
  quality   at 8, 16 and 32 samples against the 256-sample frame of the same fast accumulator kind:
            clamped RMSE and mean brightness ratio (hit pixels with finite values, means clamped
            to [0, 4]) of the raw frame, of the guided filter (5 iterations, defaults) with its
            spatial variance estimate, and of the same filter with the measured variance.

  adaptive  the variance rule (select_variance, no mark) against the mark rule (select after a mark)
            on fast accumulators: minimum 16, maximum 256, step 16.  The mark rule runs at
            --threshold; the variance rule's threshold is bisected until its run spends the same
            total samples (within 0.5%); then the clamped RMSE of each run's frame (every pixel
            divided by its own count) against the 256-sample frame.

    python tools/moments_passes.py cost|variance|quality|adaptive [--label NAME] [--out FILE]
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


def passes_ms(scene, c, moments, k=4, n=4):
    acc = scene.accumulator(fast=True, fast_chunk=c, moments=moments)
    ms = [acc.add(n)["render_ms"] for _ in range(k)]
    acc.free()
    return sum(ms)


def guided(torch, rt, sums, spp, records, variance):
    """rt_denoise_guided_device (the host function's bits) with a given variance or its own estimate."""
    h, w = sums.shape[:2]
    d_s, d_g = torch.from_numpy(np.ascontiguousarray(sums)).cuda(), torch.from_numpy(np.ascontiguousarray(records)).cuda()
    d_v = torch.from_numpy(np.ascontiguousarray(variance)).cuda() if variance is not None else None
    d_o = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    rt.denoise_guided_device(d_s.data_ptr(), 0, spp, w, h, d_g.data_ptr(), d_o.data_ptr(), torch.cuda.current_stream().cuda_stream,
                             d_variance_ptr=d_v.data_ptr() if d_v is not None else 0)
    torch.cuda.synchronize()
    return d_o.cpu().numpy()


def adaptive_run(scene, c, threshold, variance_rule, lo=16, hi=256, step=16):
    """One adaptive run (Scene.render_adaptive's two loops, with the rounds counted):
    (mean frame, total samples, rounds, render ms)."""
    acc = scene.accumulator(fast=True, fast_chunk=c, moments=variance_rule)
    ms = 0.0
    if variance_rule:
        ms += acc.add(lo)["render_ms"]
    else:
        ms += acc.add(lo // 2)["render_ms"]
        acc.mark()
        ms += acc.add(lo - lo // 2)["render_ms"]
    rounds = 0
    while acc.samples < hi:
        target = min(hi, acc.samples + step)
        n = acc.select_variance(target, threshold=threshold) if variance_rule else acc.select(target, threshold=threshold)
        if n == 0:
            break
        if not variance_rule:
            acc.mark()
        ms += acc.add_selected()["render_ms"]
        rounds += 1
    sums, counts = acc.sums(), acc.counts()
    acc.free()
    mean = sums / np.maximum(counts, 1)[..., None].astype(np.float32)
    return mean, int(counts.sum(dtype=np.int64)), rounds, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["cost", "variance", "quality", "adaptive"])
    ap.add_argument("--threshold", type=float, default=0.25, help="adaptive: the mark rule's threshold")
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=2)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--commit", default=None, help="the commit the figures come from (default: HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_passes.jsonl"))
    args = ap.parse_args()
    path = bench.load_scenes_module().ensure_scene(args.scene, os.environ.get("RT_SCENE_DIR", "/tmp/rt_scenes"))
    W, H, c = args.width, args.height, args.chunk
    rec = {"what": args.what, "label": args.label, "commit": args.commit or commit(), "scene": args.scene, "width": W, "height": H,
           "chunk": c, "lib": os.environ.get("RT_LIB", "default")}
    import torch  # (shares its HIP runtime with librt_hw_amd.so)
    rt = bench.import_pkg()
    rec["gpu"] = torch.cuda.get_device_name(0)
    scene = rt.Scene.load(path, W, H, 256)
    if args.what == "cost":
        passes_ms(scene, c, False)   # warm-up of each kind
        passes_ms(scene, c, True)
        plain, moments = [], []
        for _ in range(args.reps):   # alternating
            plain.append(round(passes_ms(scene, c, False), 3))
            moments.append(round(passes_ms(scene, c, True), 3))
        rec.update(passes="4 x 4 samples", fast_ms=plain, moments_ms=moments, fast_best_ms=min(plain), moments_best_ms=min(moments),
                   gap_ms=round(min(moments) - min(plain), 3), ratio=round(min(moments) / min(plain), 4))
    elif args.what == "variance":
        stream = torch.cuda.current_stream().cuda_stream
        d_g = torch.empty((H, W, 16), dtype=torch.float32, device="cuda")
        scene.upload(0)
        scene.gbuffer_device(d_g.data_ptr(), stream)
        acc = scene.accumulator(fast=True, fast_chunk=c, moments=True)
        rec["full_pass_8spp_ms"] = round(acc.add(8)["render_ms"], 3)
        d_o = torch.empty((H, W), dtype=torch.float32, device="cuda")
        d_c = torch.from_numpy(acc.counts()).cuda()
        for name, counts in (("spp", 0), ("counts", d_c.data_ptr())):
            best, runs = timed(torch, lambda: rt.variance_from_moments_device(acc.device_sums_ptr, acc.device_moments_ptr, counts, 8, W, H,
                                                                              d_g.data_ptr(), d_o.data_ptr(), stream), args.reps)
            rec[f"variance_kernel_{name}_ms"] = round(best, 4)
            rec[f"variance_kernel_{name}_runs_ms"] = runs
        acc.free()
    elif args.what == "adaptive":
        g = scene.gbuffer()
        acc = scene.accumulator(fast=True, fast_chunk=c)
        acc.add(256)
        truth = acc.sums() * (np.float32(1) / np.float32(256))
        acc.free()

        def row(mean, total, rounds, ms, threshold):
            use = (g["prim"] >= 0) & np.isfinite(truth).all(-1) & np.isfinite(mean).all(-1)
            d = np.clip(mean[use].astype(np.float64), 0, 4) - np.clip(truth[use].astype(np.float64), 0, 4)
            return {"threshold": threshold, "samples": total, "samples_share_of_256": round(total / (256.0 * W * H), 4), "rounds": rounds,
                    "render_ms": round(ms, 2), "rmse": round(float(np.sqrt((d * d).mean())), 5)}

        mark = adaptive_run(scene, c, args.threshold, False)
        rec["mark_rule"] = row(*mark, args.threshold)
        lo_t, hi_t, tries = 0.01, 4.0, []   # (a larger threshold spends fewer samples)
        best = None
        for _ in range(10):
            t = float(np.sqrt(lo_t * hi_t))
            run = adaptive_run(scene, c, t, True)
            tries.append({"threshold": round(t, 5), "samples": run[1]})
            if best is None or abs(run[1] - mark[1]) < abs(best[0][1] - mark[1]):
                best = (run, t)
            if abs(run[1] - mark[1]) <= 0.005 * mark[1]:
                break
            if run[1] > mark[1]:
                lo_t = t
            else:
                hi_t = t
        rec["variance_rule"] = row(*best[0], round(best[1], 5))
        rec["bisection"] = tries
        rec["note"] = "the truth is a plain fast accumulator's 256-sample frame: the same samples the adaptive runs draw from"
    else:
        g = scene.gbuffer()
        records = g["records"]
        acc = scene.accumulator(fast=True, fast_chunk=c, moments=True)
        frames = {}
        for spp in (8, 16, 32, 256):
            acc.add(spp - acc.samples)
            sums = acc.sums()
            if spp == 256:
                truth = sums * (np.float32(1) / np.float32(256))
                break
            V = acc.variance()
            frames[spp] = {"raw": sums * (np.float32(1) / np.float32(spp)), "guided_spatial": guided(torch, rt, sums, spp, records, None),
                           "guided_measured": guided(torch, rt, sums, spp, records, V)}
        acc.free()
        rows = []
        for spp, fr in frames.items():
            use = (g["prim"] >= 0) & np.isfinite(truth).all(-1)
            for x in fr.values():
                use = use & np.isfinite(x).all(-1)
            t = np.clip(truth[use].astype(np.float64), 0, 4)
            row = {"spp": spp, "truth_spp": 256, "pixels": int(use.sum())}
            for k, x in fr.items():
                v = np.clip(x[use].astype(np.float64), 0, 4)
                row[f"rmse_{k}"] = round(float(np.sqrt(((v - t) ** 2).mean())), 5)
                row[f"mean_ratio_{k}"] = round(float(v.mean() / t.mean()), 4)
            row["measured_over_spatial"] = round(row["rmse_guided_measured"] / row["rmse_guided_spatial"], 4)
            rows.append(row)
        rec.update(quality=rows, parameters="defaults (5 iterations, sigma_var 2, firefly 8)",
                   note="the truth is this accumulator's own 256-sample fast frame, which contains the samples of the noisy frames")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
