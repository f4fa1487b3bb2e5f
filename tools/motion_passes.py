#!/usr/bin/env python3
"""What the per-pixel motion records cost and gain.  Appends JSON lines to
profiles/motion_passes.jsonl:

  kernels  on the headline frame (sponza proxy 1920x1080, one GPU) with one mesh translated between
           the two frames, HIP-event times, the minimum of --reps (at least 5) timed runs after a
           warm-up, all in one process: the motion kernel (rt_motion_device), the temporal kernel with
           the records (rt_temporal_motion_device) and without them (rt_temporal_device) on the same
           frames, the snapshot copy (the scene's triangles, device to device), and the whole
           rt_history_push of an opted-in history after a move and of one on an unmoved scene (the
           update itself is outside the timed region)
  quality  cornell 64x64, 1 sample per frame, eight frames of the short box translating one pixel per
           frame along the camera's right axis, still camera: clamped RMSE (hit pixels with finite
           values, means clamped to [0, 4]) against a 256-sample render of the last frame, of the raw
           last frame, the history without and with motion records, and the latter through
           rt_denoise_guided with the step's variance; over all pixels and over the box's alone

    python tools/motion_passes.py kernels|quality [--label NAME] [--out FILE]
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
from denoise_passes import commit, rmse, timed  # noqa: E402


def movable_mesh(view, wanted):
    """`wanted` if it is not emissive, else the first mesh that is not."""
    lit = np.any(np.asarray(view["mesh_f"])[:, 3:6] != 0, axis=1)
    return wanted if not lit[wanted] else int(np.flatnonzero(~lit)[0])


def place(scene, records):
    for first, tri in records:
        scene.update_triangles(first, tri)


def kernels(rt, torch, args, rec):
    path = bench.load_scenes_module().ensure_scene(args.scene, os.environ.get("RT_SCENE_DIR", "/tmp/rt_scenes"))
    W, H, spp = args.width, args.height, 1
    scene = rt.Scene.load(path, W, H, spp)
    scene.upload(0)
    stream = torch.cuda.current_stream().cuda_stream
    cam = scene.camera()
    view = scene.view()
    mesh = movable_mesh(view, args.mesh)
    tri0 = np.ascontiguousarray(view["tri"], np.float32).copy()
    n_tris = len(tri0)
    there = scene.translated_records(mesh, (0.05, 0.0, 0.02), cover=True)
    back = [(first, tri0[first:first + len(t)].copy()) for first, t in there]
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")   # noqa: E731
    d_g0, d_g1, d_h0, d_h1, d_mean, d_var, d_mo = (new(H, W, 16), new(H, W, 16), new(3, H, W, 4), new(3, H, W, 4), new(H, W, 3),
                                                   new(H, W), new(H, W, 8))
    d_s0 = torch.from_numpy(scene.render_sums(spp)[0]).cuda()
    scene.gbuffer_device(d_g0.data_ptr(), stream)
    rt.temporal_device(d_s0.data_ptr(), 0, spp, W, H, d_g0.data_ptr(), d_h0.data_ptr(), stream_ptr=stream)
    place(scene, there)
    tri1 = np.ascontiguousarray(scene.view()["tri"], np.float32)
    d_t0, d_t1 = torch.from_numpy(tri0).cuda(), torch.from_numpy(tri1).cuda()
    d_s1 = torch.from_numpy(scene.render_sums(spp)[0]).cuda()
    scene.gbuffer_device(d_g1.data_ptr(), stream)
    torch.cuda.synchronize()
    ids = d_g1[..., 7].cpu().numpy().view(np.int32)
    moved = (np.asarray(view["tri_attr"], np.float32)[:, 15].view(np.int32) == mesh)
    rec.update(scene=args.scene, width=W, height=H, mesh=mesh, n_tris=n_tris, tri_bytes=int(tri0.nbytes),
               moved_triangles=int(moved.sum()), pixels_on_moved_triangles=round(float(moved[np.where(ids >= 0, ids, 0)][ids >= 0].sum()) / (W * H), 4))
    best, runs = timed(torch, lambda: rt.motion_device(d_g1.data_ptr(), W, H, d_t1.data_ptr(), d_t0.data_ptr(), n_tris, d_mo.data_ptr(), stream),
                       args.reps)
    rec.update(motion_kernel_ms=round(best, 4), motion_kernel_runs_ms=runs)
    torch.cuda.synchronize()
    state = d_mo[..., 3].cpu().numpy().view(np.int32)
    rec["states"] = {str(k): int((state == k).sum()) for k in (0, 1, 2)}

    def step(d_motion):
        rt.temporal_device(d_s1.data_ptr(), 0, spp, W, H, d_g1.data_ptr(), d_h1.data_ptr(), d_mean.data_ptr(), d_var.data_ptr(), cam_prev=cam,
                           d_gbuffer_prev_ptr=d_g0.data_ptr(), d_history_prev_ptr=d_h0.data_ptr(), stream_ptr=stream, d_motion_ptr=d_motion)

    best, runs = timed(torch, lambda: step(d_mo.data_ptr()), args.reps)
    rec.update(temporal_motion_kernel_ms=round(best, 4), temporal_motion_kernel_runs_ms=runs)
    torch.cuda.synchronize()
    rec["pixels_with_history_motion"] = round(float((d_h1[0, :, :, 3] >= 2).float().mean().item()), 4)
    best, runs = timed(torch, lambda: step(None), args.reps)
    rec.update(temporal_kernel_ms=round(best, 4), temporal_kernel_runs_ms=runs)
    torch.cuda.synchronize()
    rec["pixels_with_history_plain"] = round(float((d_h1[0, :, :, 3] >= 2).float().mean().item()), 4)
    d_copy = torch.empty_like(d_t0)
    best, runs = timed(torch, lambda: d_copy.copy_(d_t1), args.reps)
    rec.update(snapshot_copy_ms=round(best, 4), snapshot_copy_runs_ms=runs)

    def pushes(motion, move):
        """HIP-event times of rt_history_push alone; with `move` the mesh changes place before each."""
        hist = scene.history(motion=motion)
        ms, where = [], [back, there]
        for k in range(args.reps + 2):
            if move:
                place(scene, where[k % 2])
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            hist.push(d_s1.data_ptr(), 0, spp, d_mean.data_ptr(), d_var.data_ptr(), stream)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        had = hist.motion_ptr() != 0
        hist.free()
        return min(ms[2:]), [round(x, 4) for x in ms[2:]], had   # (the first push has no history, the second warms up)

    for key, motion, move in (("push_plain_unmoved", False, False), ("push_motion_unmoved", True, False),
                              ("push_plain_moved", False, True), ("push_motion_moved", True, True)):
        best, runs, had = pushes(motion, move)
        rec.update({key + "_ms": round(best, 4), key + "_runs_ms": runs, key + "_had_records": had})
    rec["record_traffic_bytes_per_pixel"] = 64   # 32 B written by the motion kernel, 32 B read by the step
    rec["record_traffic_MB"] = round(64.0 * W * H / 1e6, 1)


def quality(rt, args, rec):
    W = H = 64
    path = os.path.join(ROOT, "tests", "golden", "scenes", "cornell", "cornell.gltf")
    scene = rt.Scene.load(path, W, H, 1)
    cam = scene.camera()
    view = scene.view()
    mesh_of = np.asarray(view["tri_attr"], np.float32)[:, 15].view(np.int32)
    lit = np.any(np.asarray(view["mesh_f"])[:, 3:6] != 0, axis=1)
    boxes = [m for m in range(len(lit)) if not lit[m] and (mesh_of == m).sum() == 12]
    mesh = boxes[-1]
    base = np.ascontiguousarray(view["tri"], np.float32).copy()
    g0 = scene.gbuffer()["records"]
    on0 = g0.view(np.int32)[..., 11] == mesh
    P = g0[..., 12:15]
    pair = on0[:, 1:] & on0[:, :-1]
    pixel = float(np.median(np.linalg.norm(P[:, 1:][pair] - P[:, :-1][pair], axis=-1)))
    right = np.asarray(cam["axes"], np.float32).reshape(3, 3)[0]
    sel = mesh_of == mesh
    ids = np.flatnonzero(sel)
    hist_p, hist_m, prev = None, None, None
    for k in range(8):
        tri = base.copy()
        tri[sel, 0:3] = (tri[sel, 0:3] + (np.float32(k * pixel) * right).astype(np.float32)).astype(np.float32)
        for run in np.split(ids, np.flatnonzero(np.diff(ids) != 1) + 1):
            scene.update_triangles(int(run[0]), tri[run])
        frame, g = scene.render_sums(1)[0], scene.gbuffer()["records"]
        mo = rt.motion(g, tri, prev[1]) if prev else None
        hist_p, mean_p, _ = rt.temporal(frame, 1, g, cam if prev else None, prev[0] if prev else None, hist_p)
        hist_m, mean_m, var_m = rt.temporal(frame, 1, g, cam if prev else None, prev[0] if prev else None, hist_m, motion=mo)
        prev = (g, tri)
    truth = scene.render_sums(256)[0] * (np.float32(1) / np.float32(256))
    outs = {"raw_last_frame": frame, "history_without_motion": mean_p, "history_with_motion": mean_m,
            "history_with_motion_guided": rt.denoise_guided(mean_m, 1, g, variance=var_m)}
    use = (g.view(np.int32)[..., 7] >= 0) & np.isfinite(truth).all(-1)
    for x in outs.values():
        use = use & np.isfinite(x).all(-1)
    on = use & (g.view(np.int32)[..., 11] == mesh)
    rec.update(scene="cornell", width=W, height=H, frames=8, mesh=int(mesh), pixels_per_frame=1.0, world_units_per_pixel=round(pixel, 5),
               spp_per_frame=1, truth_spp=256, pixels=int(use.sum()), box_pixels=int(on.sum()),
               box_history_length_mean={"without_motion": round(float(hist_p[0][..., 3][on].mean()), 3),
                                        "with_motion": round(float(hist_m[0][..., 3][on].mean()), 3)},
               rmse={k: round(rmse(x, truth, use), 5) for k, x in outs.items()},
               rmse_box={k: round(rmse(x, truth, on), 5) for k, x in outs.items()}, parameters="defaults (picked, not measured)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "quality"])
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--mesh", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--commit", default=None, help="the commit the figures come from (default: HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_passes.jsonl"))
    args = ap.parse_args()
    args.reps = max(args.reps, 5)
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
