"""The traversal's frame rule on the CPU (rt_wavefront.h trav_pop ELIDE: a far child that survives
pushes the node's best frame only if the near subtree found a hit; tests/native/acc_elide_host.cpp):
a stand-alone program, built with AddressSanitizer and UBSan, runs trav_step with every best frame,
trav_step with the rule and closest_hit over the committed fixtures (cornell, sponza_mini, geoedge), the
perfect-squares scene of test_far_dist.py, and random plus special-value rays (the geoedge rays, which
hold zero, denormal, huge, infinite and NaN components, go to every scene).  Per ray, primitive, t bits
and both test counts are equal across the three; a counting stack shows that the rule never writes a best
frame holding 1e9, never pushes more or goes deeper, and pushes strictly fewer frames per scene.  Then
the host emulation of the lane-resident kernel renders one cornell frame with its per-lane step in either
form (two builds of the program): the same sums and counters, byte for byte.  No GPU is touched."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rtref
from test_far_dist import stack_rays, stack_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "acc_elide_host.cpp")
N_RANDOM = 1536


def case_blob(a, org, dirs):
    """A scene's arrays (the dict of Scene.view()) and rays as acc_elide_host.cpp's load() reads them."""
    def arr(name, dtype):
        return np.ascontiguousarray(a[name], dtype).reshape(-1)

    org, dirs = np.ascontiguousarray(org, np.float32), np.ascontiguousarray(dirs, np.float32)
    texels = arr("texels", np.uint8)
    head = struct.pack("<12i", int(a["width"]), int(a["height"]), int(a["samples"]), int(a["ray_depth"]), len(a["tri"]),
                       len(a["node"]), len(a["light"]), len(a["light_node"]), len(a["mesh_f"]), len(a["tex_info"]), len(org), 0)
    cam = np.concatenate([[np.float32(a["max_distance"])], arr("cam_pos", np.float32), arr("cam_axes", np.float32),
                          arr("cam_fov", np.float32), arr("tan_half_fov", np.float32)]).astype(np.float32)
    assert cam.size == 17
    parts = [head, cam.tobytes(), struct.pack("<Q", texels.size)]
    for name, dtype in (("tri", np.float32), ("tri_attr", np.float32), ("tri_tan", np.float32), ("node", np.float32),
                        ("light", np.float32), ("light_node", np.float32), ("mesh_f", np.float32), ("mesh_tex", np.int32),
                        ("mesh_normal_transform", np.float64), ("tex_info", np.uint32)):
        parts.append(arr(name, dtype).tobytes())
    parts += [texels.tobytes(), org.tobytes(), dirs.tobytes()]
    return b"".join(parts)


def random_rays(a, seed):
    """Origins uniform in the root box (cut to 8 units around the origin, where a fixture's box is huge)
    and, for a third of them, a little outside it; directions uniform on the sphere."""
    rng = np.random.default_rng(seed)
    root = np.asarray(a["node"], np.float32).reshape(-1, 8)[0]
    lo = np.maximum(np.nan_to_num(root[0:3], nan=-8.0, posinf=8.0, neginf=-8.0), -8.0).astype(np.float64)
    hi = np.minimum(np.nan_to_num(root[3:6], nan=8.0, posinf=8.0, neginf=-8.0), 8.0).astype(np.float64)
    hi = np.maximum(hi, lo)
    u = rng.random((N_RANDOM, 3))
    u[::3] = u[::3] * 1.5 - 0.25
    org = lo + u * (hi - lo)
    d = rng.normal(size=(N_RANDOM, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return org.astype(np.float32), d.astype(np.float32)


def _compile(out, *defines):
    return subprocess.Popen(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                             "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", *defines, SRC, "-o", out])


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    """The program with the emulation's per-lane step pushing every best frame (as built for the device),
    and with the rule."""
    d = tmp_path_factory.mktemp("acc_elide")
    outs = [str(d / "acc_elide_host"), str(d / "acc_elide_host_rule")]
    builds = [_compile(outs[0]), _compile(outs[1], "-DRT_LANE_ACC_ELIDE=1")]
    assert [b.wait() for b in builds] == [0, 0]
    return outs


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_both_frame_rules_and_closest_hit_agree(rt, progs, tmp_path):
    special = rtref.golden("geoedge_rays_in.rtd")
    s_org, s_dir = special["origin"], special["direction"]
    assert not np.isfinite(s_dir).all() and np.isnan(s_org).any() and (s_dir == 0).all(1).any()
    scenes = [("cornell", rt.Scene.load(rtref.scene_path("cornell"), 16, 16, 1).view()),
              ("sponza_mini", rt.Scene.load(rtref.scene_path("sponza_mini"), 16, 16, 1).view()),
              ("geoedge", rtref.ref_arrays(rt, "geoedge", 64, 64, 1)),
              ("stack", stack_scene(rt, tmp_path))]
    sq_org, sq_dir = stack_rays()
    files = []
    for k, (name, a) in enumerate(scenes):
        r_org, r_dir = random_rays(a, 20261021 + k)
        org, dirs = [r_org, s_org], [r_dir, s_dir]
        if name == "stack":
            org.append(sq_org)
            dirs.append(sq_dir)
        path = str(tmp_path / (name + ".bin"))
        with open(path, "wb") as f:
            f.write(case_blob(a, np.concatenate(org), np.concatenate(dirs)))
        files.append(path)
    out = _run([progs[0], "trace"] + files)
    assert out.count(": equal") == len(files), out
    assert "no geometry" not in out


def test_emulated_frame_is_the_same_under_either_rule(rt, progs, tmp_path):
    a = rt.Scene.load(rtref.scene_path("cornell"), 16, 16, 4).view()
    case = str(tmp_path / "cornell_16x16x4.bin")
    with open(case, "wb") as f:
        f.write(case_blob(a, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)))
    got = []
    for prog, text in zip(progs, ("with every best frame", "with the rule")):
        out = str(tmp_path / (os.path.basename(prog) + ".out"))
        assert text in _run([prog, "emu", case, out])
        with open(out, "rb") as f:
            got.append(f.read())
    assert len(got[0]) == 16 * 16 * 3 * 4 + 7 * 8
    assert got[0] == got[1]
    sums = np.frombuffer(got[0][:16 * 16 * 12], np.float32)
    assert np.isfinite(sums).all() and sums.max() > 0
