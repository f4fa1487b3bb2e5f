"""Posable meshes on the GPU (include/rt_hw.h rt_scene_pose_meshes; the kernels are rt_pose_kernel and
rt_pose_nt_kernel, raytracing-hw_amd/csrc/rt_pose_device.h): the device copy against the host twin (which
tests/test_pose.py pins to the reference's own loads of the poses), a posed scene against a scene built
with the posed arrays (every entry, bit for bit) and against the CPU oracle, mesh_nt on a normal-mapped
mesh, the way back to the reference's golden, special values, epochs and motion records, a later upload,
and the CLI's RT_POSES end to end.  Every equality is bit equality."""
import os
import subprocess

import numpy as np
import pytest

import pose_util
import rtref
from motion_util import CARRIED
from refit_util import bits, tri_mesh
from test_gpu_accum import gpu   # noqa: F401  (fixture)
from test_pose import special_matrices

pytestmark = pytest.mark.gpu
SOLUTION = os.path.join(rtref.ROOT, "raytracing-hw_amd", "rt_solution")
NAME, W, H, S = "cornell", 33, 17, 3
COUNTERS = ("rays", "aabb_tests", "tri_tests", "light_queries", "light_aabb_tests", "light_tri_tests", "shading_hits")
ARRAYS = ("tri", "tri_attr", "tri_tan", "node")


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_f64(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def load(gpu, name, w=W, h=H):
    return gpu.Scene.load(rtref.scene_path(name), w, h, S)


def wiped(gpu, name, w=W, h=H):
    """(the fixture as a from_view scene on device 0 with its rest data, every box wiped to NaN; the loaded arrays)."""
    loaded = load(gpu, name, w, h)
    a = loaded.view()
    b = dict(a, node=a["node"].copy())
    b["node"][:, 0:6] = np.nan
    s = gpu.Scene.from_view(b)
    s.set_rest(loaded.rest())
    s.upload(0)
    assert np.isnan(s.read_device()["node"][:, 0:6]).all()
    return s, a


def device_is_the_host(s, lights=False):
    d, v = s.read_device(), s.view()
    for k in ARRAYS:
        diff = (bits(d[k]) != bits(v[k])).any(axis=1).sum()
        assert diff == 0, f"{k}: {diff} records of the device copy differ from the host twin's"
    if lights:
        dl = s.read_device_lights()
        assert same_bits(dl["light"], v["light"]) and same_bits(dl["light_node"], v["light_node"])
    return d, v


# ------------------------------------------------------------------------ 1. the device copy is the host twin's
@pytest.mark.parametrize("variant", list(pose_util.VARIANTS))
def test_device_copy_is_the_host_twins(gpu, variant):
    name = pose_util.VARIANTS[variant][0]
    poses = pose_util.pose_matrices(gpu, variant)
    host = load(gpu, name)   # never uploaded: the host twin alone
    host.enable_poses()
    host.pose(poses)
    want = host.view()
    s, a = wiped(gpu, name)
    s.enable_poses()
    s.pose(poses)
    d, v = device_is_the_host(s)
    for k in ("tri", "tri_attr", "tri_tan"):
        assert same_bits(v[k], want[k]), k
    assert same_bits(v["node"], want["node"]) and same_f64(v["mesh_normal_transform"], want["mesh_normal_transform"])
    assert same_bits(d["tri_attr"][:, 9:16], a["tri_attr"][:, 9:16]) and same_bits(d["tri_tan"], a["tri_tan"])
    assert not same_bits(d["tri"], a["tri"])
    assert not np.isnan(d["node"][:, 0:6]).any()


def test_one_mesh_per_call_and_the_lamp(gpu):
    """The two cubes and the lamp in three calls, then all three back at once: after every call the
    device copy (lights included) is the host twin's."""
    poses = {**pose_util.pose_matrices(gpu, "pose_cornell"), **pose_util.lamp_pose(gpu)}
    s, a = wiped(gpu, NAME)
    s.enable_light_updates()
    s.enable_poses()
    host = load(gpu, NAME)
    host.enable_light_updates()
    host.enable_poses()
    loaded = {m: host.mesh_transform(m) for m in poses}
    for m, M in poses.items():
        s.pose({m: M})
        host.pose({m: M})
        d, v = device_is_the_host(s, lights=True)
        assert same_bits(v["tri"], host.view()["tri"]) and same_bits(v["light"], host.view()["light"])
    assert not same_bits(s.read_device_lights()["light"], a["light"])
    s.pose(loaded)
    d, v = device_is_the_host(s, lights=True)
    assert same_bits(d["tri"], a["tri"]) and same_bits(d["node"], a["node"]) and same_bits(d["tri_attr"], a["tri_attr"])
    dl = s.read_device_lights()
    assert same_bits(dl["light"], a["light"]) and same_bits(dl["light_node"], a["light_node"])


# ------------------------------------------------------------------------ 2. render parity
def posed_pair(gpu, variant="pose_cornell", w=W, h=H):
    """(the base fixture posed after an upload and a render of the loaded geometry, the twin built by
    from_view of the posed view, the twin's arrays, the frame before)."""
    b = load(gpu, pose_util.VARIANTS[variant][0], w, h)
    b.upload(0)
    old, _ = b.render_sums(1)
    b.enable_poses()
    b.pose(pose_util.pose_matrices(gpu, variant))
    want = b.view()
    return b, gpu.Scene.from_view(want), want, old


def test_posed_cornell_is_a_scene_built_with_it(gpu, oracle):
    b, a, want_arrays, old = posed_pair(gpu)
    want, _ = a.render_sums(S)
    got, _ = b.render_sums(S)
    assert same_bits(got, want) and not same_bits(old, a.render_sums(1)[0])
    cpu, cnt, _ = oracle.render(want_arrays, S)
    assert same_bits(cpu.reshape(want.shape), want)
    assert same_bits(b.render_sums(S, kernel=4)[0], want) and same_bits(a.render_sums(S, kernel=4)[0], want)
    assert same_bits(b.render_sums(S, runahead=False)[0], want)
    assert same_bits(b.render_sums(S, fast=True)[0], a.render_sums(S, fast=True)[0])
    for kernel in (0, 4):
        (gc, sc), (wc, swc) = b.render_sums(S, count=True, kernel=kernel), a.render_sums(S, count=True, kernel=kernel)
        assert same_bits(gc, want) and same_bits(wc, want)
        for k in COUNTERS:
            assert sc[k] == swc[k] and sc["rays"] > 0, (kernel, k)
        assert [sc[k] for k in COUNTERS[:6]] == [int(x) for x in cnt], kernel
    assert same_bits(b.gbuffer()["records"], a.gbuffer()["records"])
    assert same_bits(b.render_frame(S, n_shards=1)[1], want)


# ------------------------------------------------------------------------ 3. mesh_nt follows
def test_mesh_nt_follows_the_pose(gpu, oracle):
    """texedge's floor has a normal texture: its shading takes tangents through mesh_normal_transform.
    The posed scene renders as its from_view twin and as the oracle; with the loaded transform in place
    of the posed one the oracle's frame is another one."""
    w, h = 40, 24
    b, a, want_arrays, _ = posed_pair(gpu, "pose_texedge", w, h)
    (mesh, _), = pose_util.pose_matrices(gpu, "pose_texedge").items()
    assert want_arrays["mesh_tex"][mesh, 1] >= 0
    want, _ = a.render_sums(S)
    assert same_bits(b.render_sums(S)[0], want) and same_bits(b.render_sums(S, kernel=4)[0], want)
    cpu, _, _ = oracle.render(want_arrays, S)
    assert same_bits(cpu.reshape(want.shape), want)
    stale = dict(want_arrays, mesh_normal_transform=load(gpu, "texedge", w, h).view()["mesh_normal_transform"])
    other, _, _ = oracle.render(stale, S)
    differ = int((bits(other.reshape(want.shape)) != bits(want)).any(axis=-1).sum())
    assert differ >= 8, f"only {differ} pixels show the normal transform"


# ------------------------------------------------------------------------ 4. back to the golden
def test_posing_back_gives_the_reference_frame(gpu):
    b, _, _, _ = posed_pair(gpu)
    a = load(gpu, NAME).view()
    rest = b.rest()
    loaded = load(gpu, NAME).rest()["mesh_matrix"]
    assert not np.array_equal(rest["mesh_matrix"], loaded)
    b.pose({m: loaded[m] for m in range(len(loaded)) if not np.any(a["mesh_f"][m, 3:6] != 0)})
    gold = rtref.golden(f"{NAME}_sums_{W}x{H}x{S}.rtd")
    got, st = b.render_sums(S, count=True)
    assert same_bits(got, gold["sums"].reshape(got.shape)) and st["rays"] == int(gold["counters"][0])
    assert same_bits(b.render_sums(S)[0], got)
    assert same_bits(b.read_device()["node"], a["node"]) and same_bits(b.read_device()["tri"], a["tri"])


# ------------------------------------------------------------------------ 5. special values
@pytest.mark.parametrize("which", ["nan", "inf"])
def test_special_values_on_the_device(gpu, which):
    s, a = wiped(gpu, NAME)
    s.enable_poses()
    mesh, nan, inf = special_matrices(gpu)
    s.pose({mesh: nan if which == "nan" else inf})
    d, v = s.read_device(), s.view()
    assert not np.isfinite(v["tri"][tri_mesh(v) == mesh]).all()
    for k in ARRAYS:   # (a NaN word may differ in its bits between host and device: rtref.same)
        assert rtref.same(d[k], v[k]).all(), k
    assert same_bits(d["node"], v["node"]) and not np.isnan(d["node"][:, 0:6]).any()


# ------------------------------------------------------------------------ 6. epochs and histories
def test_accumulators_go_stale_and_reset(gpu):
    b = load(gpu, NAME)
    b.enable_poses()
    acc = b.accumulator()
    acc.add(2)
    was = acc.sums()
    b.pose(pose_util.pose_matrices(gpu, "pose_cornell"))
    lib = gpu.lib()
    assert lib.rt_accum_add(acc._h, 1, None, None) == -1 and b"rt_accum_reset" in lib.rt_last_error()
    assert same_bits(acc.sums(), was) and acc.samples == 2
    acc.reset()
    acc.add(3)
    twin = gpu.Scene.from_view(b.view())
    assert same_bits(acc.sums(), twin.render_sums(3)[0])


def test_history_with_motion_follows_a_posed_mesh(gpu):
    import torch
    from test_gpu_motion import push
    b = load(gpu, NAME)
    b.enable_poses()
    hist = b.history(motion=True)
    d_mean = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    d_var = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    tri_prev = b.view()["tri"]
    push(hist, b.render_sums(S)[0], S, d_mean, d_var)
    assert hist.motion() is None
    poses = pose_util.pose_matrices(gpu, "pose_cornell")
    (m0, M0) = next(iter(poses.items()))
    nudged = M0.copy()
    nudged[12:15] = b.mesh_transform(m0)[12:15]
    b.pose({m0: b.mesh_transform(m0) * 1.0})       # (a pose to the matrix it has moves nothing but counts as an update)
    b.pose({m0: nudged})                           # rotated and scaled about its loaded place
    tri = b.view()["tri"]
    rec = b.gbuffer()["records"]
    push(hist, b.render_sums(S)[0], S, d_mean, d_var)
    want = gpu.motion(rec, tri, tri_prev)
    got = hist.motion()
    assert got is not None and same_bits(got["records"], want["records"])
    on = rec.view(np.int32)[..., 11] == m0
    assert on.sum() >= 4 and (want["state"][on] == CARRIED).any() and not same_bits(tri, tri_prev)
    hist.free()


# ------------------------------------------------------------------------ 7. devices
def test_later_uploads_of_a_posed_scene_are_current(gpu):
    if gpu.device_count() < 2:
        pytest.skip("needs two GPUs")
    b, _, want, _ = posed_pair(gpu)
    b.upload(1)
    d1 = b.read_device(1)
    for k in ARRAYS:
        assert same_bits(d1[k], want[k]), k
    loaded = load(gpu, NAME)
    b.pose({m: loaded.mesh_transform(m) for m in pose_util.pose_matrices(gpu, "pose_cornell")})   # both copies
    for dev in (0, 1):
        assert same_bits(b.read_device(dev)["tri"], loaded.view()["tri"]) and same_bits(b.read_device(dev)["node"], loaded.view()["node"])
    assert same_bits(b.render_sums(S, device=1)[0], loaded.render_sums(S)[0])


# ------------------------------------------------------------------------ 8. CLI
def frame_bytes(path):
    data = path.read_bytes()
    header = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(header)
    return np.frombuffer(data[len(header):], np.uint8).reshape(H, W, 3)


def test_cli_poses(gpu, tmp_path):
    base, named = pose_util.VARIANTS["pose_cornell"]
    ids = pose_util.mesh_ids(rtref.scene_path(base))
    (n0, p0), (n1, p1) = named.items()

    def group(name, trs):
        t, r, s = trs
        return " ".join([str(ids[name][0])] + [repr(float(x)) for x in (*t, *r, *s)])

    lines = [group(n0, p0), group(n0, p1) + "  " + group(n1, p0)]
    poses = tmp_path / "poses.txt"
    poses.write_text("# mesh tx ty tz qx qy qz qw sx sy sz\n" + lines[0] + "\n\n" + lines[1] + "\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}
    r = subprocess.run([SOLUTION, rtref.scene_path(NAME), str(W), str(H), str(S), str(tmp_path / "out.ppm")],
                       env=dict(env, RT_GPUS="1", RT_POSES=str(poses)), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert not (tmp_path / "out.ppm").exists() and not (tmp_path / "out.0002.ppm").exists()
    scene = load(gpu, NAME)
    scene.enable_poses()
    frames = []
    for frame in ({ids[n0][0]: gpu.trs(*p0)}, {ids[n0][0]: gpu.trs(*p1), ids[n1][0]: gpu.trs(*p0)}):
        scene.pose(frame)
        rgb = scene.render_frame(S, n_shards=1)[0]
        frames.append(np.asarray(rgb).reshape(H, W, 3))
    for k in (0, 1):
        assert np.array_equal(frame_bytes(tmp_path / f"out.{k:04d}.ppm"), frames[k]), k
    assert not np.array_equal(frames[0], frames[1])
    r = subprocess.run([SOLUTION, rtref.scene_path(NAME), str(W), str(H), str(S), str(tmp_path / "both.ppm")],
                       env=dict(env, RT_GPUS="1", RT_POSES=str(poses), RT_MOVES=str(poses)), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "RT_POSES and RT_MOVES" in r.stderr
