"""The accumulator's per-pixel records on the GPU, as a checkpoint holds them, against what the
entries report (raytracing-hw_amd/csrc/rt_records.h: one layout for the kernels, rt_accum_state
and the file).  The file's words are read with numpy by the documented positions, not through the
header under test.  Every comparison is bit-exact."""
import numpy as np
import pytest

import rtref
from test_gpu_accum import gpu   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
bits = rtref.bits
f32 = np.float32
W, H, C = 33, 17, 2
KINDS = {"parity": dict(), "fast": dict(fast=True, fast_chunk=C), "moments": dict(fast=True, fast_chunk=C, moments=True)}


def reported(nxt, total, opn):
    """(P, 3) words: `total` on a chunk boundary, f32(total + open) off it (rt_fast_units.h reported)."""
    with np.errstate(invalid="ignore", over="ignore"):
        both = total.view(f32) + opn.view(f32)
    assert both.dtype == f32
    return np.where((nxt % C == 0)[:, None], total, bits(both))


@pytest.mark.parametrize("kind", list(KINDS))
def test_saved_records_are_what_the_entries_report(gpu, tmp_path, kind):
    scene = gpu.Scene.load(rtref.scene_path("cornell"), W, H, 3)
    acc = scene.accumulator(**KINDS[kind])
    try:
        acc.add(3)
        assert acc.select(6, window=(0, 0, 16, H)) == 16 * H
        acc.add_selected()
        path = str(tmp_path / "records.acc")
        acc.save(path)
        counts, state, sums = acc.counts().reshape(-1), acc.state(), bits(acc.sums().reshape(-1, 3))
        moments = bits(acc.moments().reshape(-1, 3)) if kind == "moments" else None
    finally:
        acc.free()
    P = W * H
    raw = open(path, "rb").read()
    assert len(raw) == 128 + (64 if kind == "moments" else 32) * P
    rec = np.frombuffer(raw, "<u4", 8 * P, 128).reshape(P, 8)
    want = np.where(np.arange(P) % W < 16, 6, 3)   # the left columns at 6 (a chunk boundary), the rest at 3 (an open chunk)
    assert np.array_equal(counts, want)
    assert np.array_equal(rec[:, 0], np.arange(P))
    assert np.array_equal(rec[:, 1], counts) and np.array_equal(state[:, 0], rec[:, 1])
    if kind == "parity":
        assert np.array_equal(state[:, 1], rec[:, 2] & 0x7fffffff) and np.array_equal(state[:, 2], rec[:, 2] >> 31)
        assert np.array_equal(state[:, 3], rec[:, 3])
        assert np.array_equal(sums, rec[:, 4:7])
        assert not rec[:, 7].any()
        return
    nxt = rec[:, 1]
    assert np.array_equal(state[:, 1:4], rec[:, 5:8])
    # (a pixel's open partial may itself be +0: zero words are required on a boundary, non-zero ones only somewhere off it)
    assert not rec[nxt % C == 0, 5:8].any() and rec[nxt % C != 0, 5:8].any()
    assert np.array_equal(sums, reported(nxt, rec[:, 2:5], rec[:, 5:8]))
    if kind == "moments":
        mom = np.frombuffer(raw, "<u4", 8 * P, 128 + 32 * P).reshape(P, 8)
        assert not mom[nxt % C == 0, 3:6].any() and mom[nxt % C != 0, 3:6].any()
        assert np.array_equal(moments, reported(nxt, mom[:, 0:3], mom[:, 3:6]))
        assert not mom[:, 6:8].any()
