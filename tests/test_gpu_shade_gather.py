"""GPU parity of the shading pass's gather (rt_path.h shade_pre, RT_SHADE_GATHER: the per-mesh
material record, the texels of every slot issued together, the wave-uniform skips) on scenes
whose meshes differ in which texture slots they have.

As in test_gpu_edges.py, every assertion is bit equality of the float32 sums (and of the six
traversal counters where the schedule counts) against the CPU oracle on the same arrays,
through every schedule (lane-resident, natural order, wavefront, light-split, runahead, 8-way
shards), and every edited case first shows that the edit changes at least 10% of the oracle's
pixels.  The device self-check 4 compares every uploaded material record with the scene's
tables on the device."""
import numpy as np
import pytest

import gather_scenes
import rtref
from test_gpu_edges import _changed, _check_variants, _many_meshes, _same, cornell_base, gpu, sponza_base  # noqa: F401

pytestmark = pytest.mark.gpu

W, H, S = 48, 27, 4


def _case(gpu, oracle, sponza_base, arrays, tag, selfcheck=False):
    base, base_ref = sponza_base
    ref, cnt, _ = oracle.render(arrays, S)
    assert _changed(ref, base_ref) >= 0.10
    scene = gpu.Scene.from_view(arrays)
    _check_variants(gpu, scene, S, ref.reshape(H, W, 3), cnt, tag)
    if selfcheck:
        assert gpu.device_selfcheck(4) == 0


def test_sixteen_slot_subsets(gpu, oracle, sponza_base):
    """All 16 subsets of the four slots, dealt by mesh index % 16: lanes of one wave diverge on
    every slot, emission-only and base-only meshes included."""
    a = gather_scenes.deal16(sponza_base[0])
    present = (a["mesh_tex"] >= 0) @ (1 << np.arange(4))
    assert set(present.tolist()) == set(range(16))
    _case(gpu, oracle, sponza_base, a, "sponza_mini 16 slot subsets", selfcheck=True)


def test_shared_and_last_texture(gpu, oracle, sponza_base):
    """One texture in all four slots of a mesh; the last texture index in every slot."""
    a = gather_scenes.shared(sponza_base[0])
    assert (a["mesh_tex"][1] == len(a["tex_info"]) - 1).all() and len(set(a["mesh_tex"][2])) == 1
    _case(gpu, oracle, sponza_base, a, "sponza_mini shared textures")


def test_no_normal_map_anywhere(gpu, oracle, sponza_base):
    """Textures but no normal map in the scene: the gather's tangent loads are skipped."""
    a = gather_scenes.no_normal_maps(sponza_base[0])
    assert (a["mesh_tex"][:, 1] < 0).all() and (a["mesh_tex"][:, 0] >= 0).any()
    _case(gpu, oracle, sponza_base, a, "sponza_mini without normal maps")


def test_single_1x1_texture(gpu, oracle, sponza_base):
    """A scene whose only texture is one texel, in every subset of the slots."""
    _case(gpu, oracle, sponza_base, gather_scenes.single_1x1(sponza_base[0]), "sponza_mini single 1x1 texture")


def test_cornell_unchanged(gpu, oracle, cornell_base):
    """No textures at all: the gather issues no texel load; the fixture as it is."""
    a, ref = cornell_base
    cnt = oracle.render(a, 8)[1]
    _check_variants(gpu, gpu.Scene.from_view(a), 8, ref.reshape(17, 33, 3), cnt, "cornell")


def test_200_meshes_sixteen_subsets(gpu, oracle, sponza_base):
    """Material records indexed beyond 64 meshes, with the 16-subset deal."""
    a = gather_scenes.deal16(_many_meshes(sponza_base[0], 200))
    assert len(a["mesh_f"]) == 200
    _case(gpu, oracle, sponza_base, a, "sponza_mini 200 meshes, 16 slot subsets", selfcheck=True)


def test_selfcheck_fixture(gpu):
    """The uploaded records of the fixture itself."""
    scene = gpu.Scene.load(rtref.scene_path("sponza_mini"), W, H, S)
    scene.render_sums(S)
    assert gpu.device_selfcheck(4) == 0


@pytest.mark.parametrize("chunk", [1, 2])
def test_fast_mode_sixteen_subsets(gpu, oracle, sponza_base, chunk):
    """Fast mode (per-sample Philox streams) on the 16-subset scene against the oracle's
    restatement of it."""
    a = gather_scenes.deal16(sponza_base[0])
    ref, _ = oracle.render_fast(a, S, chunk)
    assert _changed(ref, oracle.render_fast(sponza_base[0], S, chunk)[0]) >= 0.10
    out, st = gpu.Scene.from_view(a).render_sums(S, fast=True, fast_chunk=chunk, count=True)
    _same(out, ref, f"16 slot subsets fast chunk {chunk}")
    assert st["schedule"] == gpu.SCHED_FAST and st["samples"] == W * H * S
