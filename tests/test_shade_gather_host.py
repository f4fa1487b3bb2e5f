"""The shading gather's addressing, proved on the CPU (tests/native/shade_gather_host.cpp): a
stand-alone program, built with AddressSanitizer and UBSan, that builds the material records
with the upload's own builder and runs the gather's address function for every (mesh, slot) of
its built-in scenes (no textures, a single 1x1 texture, the last texture in every slot) and of
the scenes given to it: the four fixtures and the edited scenes of test_gpu_shade_gather.py.
Every tap must lie inside the texel array and tex_taps + tex_decode must be tex_sample_ti bit
for bit.  No GPU is touched."""
import os
import subprocess

import pytest

import gather_scenes
import rtref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "shade_gather_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gather") / "shade_gather_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", SRC, "-o", out], check=True)
    return out


def _run(prog, files):
    r = subprocess.run([prog] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_builtin_scenes(prog):
    out = _run(prog, [])
    for name in ("zero-texture", "single 1x1", "last texture in every slot"):
        assert name + ":" in out


def test_fixtures_and_edited_scenes(rt, prog, tmp_path):
    files = []

    def add(tag, arrays):
        path = str(tmp_path / (tag + ".bin"))
        with open(path, "wb") as f:
            f.write(gather_scenes.tables_blob(arrays))
        files.append(path)

    for name in ("cornell", "cornell_blob", "practice6_1", "sponza_mini"):
        add(name, rt.Scene.load(rtref.scene_path(name), 48, 27, 4).view())
    base = rtref.ref_arrays(rt, "sponza_mini", 48, 27, 4)
    for edit in (gather_scenes.deal16, gather_scenes.shared, gather_scenes.no_normal_maps, gather_scenes.single_1x1):
        add(edit.__name__, edit(base))
    out = _run(prog, files)
    assert out.count("samples bit-equal") == 3 + len(files)
