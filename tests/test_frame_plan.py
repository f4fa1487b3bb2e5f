"""The whole-frame render's plan without a GPU (raytracing-hw_amd/csrc/rt_frame_plan.h behind
tests/native/frame_plan_host.cpp): which device renders which shard and which is the root, the
row partition and where a shard's rows land in the root's staging buffer, the byte layout of
the root buffer, every device's shard buffers, what rt_render_frame refuses, and how the
shards' stats fold into the frame's.  The visible device count is an input, so the arithmetic
of shards on several devices runs here although no such machine has run it."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "frame_plan_host.cpp")
ERR_ARG, ERR_DEVICE = -1, -4
_ull, _ll, _int = ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_int
_p = ctypes.POINTER
SCALARS = ("row_u8", "row_f", "o_stage_u8", "o_frame_u8", "o_stage_f", "o_frame_f", "o_row_map", "root_bytes")


class In(ctypes.Structure):
    _fields_ = [("width", _int), ("height", _int), ("n_shards", _int), ("devices", _p(ctypes.c_int32)),
                ("row_block", _int), ("spp", _int), ("visible_devices", _int), ("want_sums", _int)]


class Out(ctypes.Structure):
    _fields_ = [("err", _int), ("msg", ctypes.c_char * 192), ("n", _int), ("n_uniq", _int), ("root", _int),
                ("dev_of", _p(_int)), ("uniq", _p(_int)), ("dev_index", _p(_int)),
                ("rows", _p(_ll)), ("base", _p(_ll)), ("frame_row_of", _p(ctypes.c_int32))] + \
               [(k, _ull) for k in SCALARS] + \
               [("max_rows", _p(_ll)), ("sum_bytes", _p(_ull)), ("buf_bytes", _p(_ull))]


class Plan:
    pass


@pytest.fixture(scope="module")
def fp(tmp_path_factory, rt):
    out = str(tmp_path_factory.mktemp("fp") / "libfp.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-shared", "-fPIC", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.fp_plan.argtypes = [_p(In), _int, _p(Out)]
    lib.fp_plan.restype = _int
    lib.fp_merge.argtypes = [_p(In), _p(rt.RtStats), ctypes.c_double, _p(rt.RtStats)]
    lib.fp_merge.restype = _int

    def make_in(W=33, H=17, n=0, devices=None, rb=4, spp=1, visible=1, sums=True):
        arr = (ctypes.c_int32 * len(devices))(*devices) if devices is not None else None
        i = In(W, H, n, arr, rb, spp, visible, int(sums))
        i._keep = arr
        return i

    def plan(**kw):
        i = make_in(**kw)
        cap = max(i.n_shards, i.visible_devices, 1) if i.n_shards <= 64 else 0
        bufs = dict(dev_of=(_int * cap)(), uniq=(_int * 64)(), dev_index=(_int * cap)(), rows=(_ll * cap)(),
                    base=(_ll * (cap + 1))(), frame_row_of=(ctypes.c_int32 * max(i.height, 1))(),
                    max_rows=(_ll * 64)(), sum_bytes=(_ull * 64)(), buf_bytes=(_ull * 64)())
        o = Out()
        for k, v in bufs.items():
            setattr(o, k, ctypes.cast(v, type(getattr(o, k))))
        rc = lib.fp_plan(ctypes.byref(i), cap, ctypes.byref(o))
        assert rc == o.err
        q = Plan()
        q.err, q.msg = o.err, o.msg.decode()
        if rc == 0:
            q.n, q.root = o.n, o.root
            for k in SCALARS:
                setattr(q, k, getattr(o, k))
            if o.n <= cap:
                for k in ("dev_of", "dev_index", "rows"):
                    setattr(q, k, list(bufs[k])[:o.n])
                q.base = list(bufs["base"])[:o.n + 1]
                q.frame_row_of = list(bufs["frame_row_of"])[:i.height]
                for k in ("uniq", "max_rows", "sum_bytes", "buf_bytes"):
                    setattr(q, k, list(bufs[k])[:o.n_uniq])
        return q

    plan.lib, plan.make_in = lib, make_in
    return plan


def test_partition_eight_shards_on_one_device(fp):
    """The GPU test's shape: 17 rows in blocks of 4 over 8 shards leaves shards 5-7 empty."""
    q = fp(H=17, rb=4, n=8, devices=[0] * 8)
    assert q.err == 0 and q.n == 8
    assert q.rows == [4, 4, 4, 4, 1, 0, 0, 0]
    assert q.base == [0, 4, 8, 12, 16, 17, 17, 17, 17]
    assert q.frame_row_of == list(range(17))
    assert q.uniq == [0] and q.root == 0 and q.dev_index == [0] * 8


def test_partition_three_shards(fp):
    q = fp(H=17, rb=4, n=3, visible=3)
    assert q.rows == [8, 5, 4]
    assert q.base == [0, 8, 13, 17]
    assert q.frame_row_of == [0, 1, 2, 3, 12, 13, 14, 15, 4, 5, 6, 7, 16, 8, 9, 10, 11]


def test_partition_36_rows(fp):
    assert fp(W=64, H=36, rb=4, n=8, devices=[0] * 8).rows == [8, 4, 4, 4, 4, 4, 4, 4]


@pytest.mark.parametrize("height,world,rb", [(1080, 1, 8), (1080, 2, 8), (1080, 3, 8), (1080, 8, 8), (17, 3, 4),
                                            (7, 8, 8), (33, 5, 1), (36, 8, 4), (17, 8, 4)])
def test_partition_agrees_with_rt_shard_rows(fp, rt, height, world, rb):
    """The plan's partition is the ABI's (rt_shard_rows, which the shard renders use)."""
    lib = rt.lib()
    q = fp(H=height, rb=rb, n=world, devices=[0] * world)
    assert q.err == 0 and q.base[0] == 0 and q.base[world] == height
    for r in range(world):
        buf = (ctypes.c_int32 * max(height, 1))()
        n = lib.rt_shard_rows(height, r, world, rb, buf)
        assert q.rows[r] == n == q.base[r + 1] - q.base[r]
        assert q.frame_row_of[q.base[r]:q.base[r + 1]] == list(buf)[:n]


def test_device_mapping(fp):
    q = fp(n=3, devices=[0, 1, 0], visible=2)
    assert (q.dev_of, q.uniq, q.root, q.dev_index) == ([0, 1, 0], [0, 1], 0, [0, 1, 0])
    q = fp(n=5, devices=[3, 2, 1, 0, 3], visible=4)
    assert (q.uniq, q.root, q.dev_index) == ([3, 2, 1, 0], 3, [0, 1, 2, 3, 0])
    q = fp(n=4, visible=4)
    assert q.dev_of == [0, 1, 2, 3] and q.uniq == [0, 1, 2, 3] and q.root == 0
    q = fp(n=0, visible=2)
    assert q.n == 2 and q.dev_of == [0, 1]


def test_root_layout(fp):
    q = fp(W=33, H=17, n=1, sums=True)
    assert (q.row_u8, q.row_f) == (99, 396)
    assert (q.o_stage_u8, q.o_frame_u8, q.o_stage_f, q.o_frame_f, q.o_row_map) == (0, 1792, 3584, 10496, 17408)
    assert q.root_bytes == 17664
    q = fp(W=33, H=17, n=1, sums=False)
    assert (q.o_stage_u8, q.o_frame_u8, q.o_stage_f, q.o_frame_f, q.o_row_map) == (0, 1792, 3584, 3584, 3584)
    assert q.root_bytes == 3840
    for sums in (True, False):
        for W, H in ((33, 17), (64, 36), (1, 1), (1920, 1080), (5, 1000)):
            q = fp(W=W, H=H, n=1, sums=sums)
            offs = [q.o_stage_u8, q.o_frame_u8, q.o_stage_f, q.o_frame_f, q.o_row_map, q.root_bytes]
            assert all(o % 256 == 0 for o in offs) and offs == sorted(offs)
            assert offs[1] - offs[0] >= 3 * W * H and offs[2] - offs[1] >= 3 * W * H   # every part holds its rows
            assert offs[3] - offs[2] == offs[4] - offs[3] == (-(-12 * W * H // 256) * 256 if sums else 0)
            assert offs[5] - offs[4] >= 4 * H


@pytest.mark.parametrize("sums", [True, False])
def test_device_buffers(fp, sums):
    q = fp(W=33, H=17, rb=4, n=3, devices=[0, 1, 0], visible=2, sums=sums)
    assert q.rows == [8, 5, 4]
    assert q.max_rows == [8, 5]
    assert q.sum_bytes == [3328, 2048]
    assert q.buf_bytes == [4120, 2543]


@pytest.mark.parametrize("kw,code,word", [
    (dict(n=0, devices=[0, 0]), ERR_ARG, "n_shards"),
    (dict(n=65537), ERR_ARG, "shard count 65537"),
    (dict(n=0, visible=0), ERR_ARG, "shard count 0"),
    (dict(n=2, devices=[0, 2], visible=2), ERR_DEVICE, "shard 1 on device 2, 2 visible"),
    (dict(n=1, devices=[64], visible=128), ERR_DEVICE, "shard 0 on device 64, 128 visible"),
    (dict(n=2, devices=[0, -1], visible=2), ERR_DEVICE, "shard 1 on device -1"),
    (dict(n=1, spp=0), ERR_ARG, "samples per pixel"),
    (dict(n=1, H=0), ERR_ARG, "row partition (height 0, row_block 4)"),
])
def test_refusals(fp, kw, code, word):
    q = fp(**kw)
    assert q.err == code
    assert q.msg.startswith("rt_render_frame: ") and word in q.msg


def test_refusals_keep_their_order(fp):
    """devices without n_shards, the shard count, the device ids, spp, then the partition."""
    assert "n_shards" in fp(n=0, devices=[9], visible=0, spp=0, H=0).msg
    assert "shard count" in fp(n=0, visible=0, spp=0, H=0).msg
    assert "on device" in fp(n=2, visible=1, spp=0, H=0).msg
    assert "samples per pixel" in fp(n=1, spp=0, H=0).msg


def test_stats_merge(fp, rt):
    i = fp.make_in(n=3, devices=[0, 1, 0], visible=2)
    counters = ["pixels", "samples", "rays", "aabb_tests", "tri_tests", "light_queries", "light_aabb_tests",
                "light_tri_tests", "shading_hits", "extend_rays"]
    sts = (rt.RtStats * 3)()
    for r in range(3):
        for k, name in enumerate(counters):
            setattr(sts[r], name, 1000 * (k + 1) + 10 ** r)
        sts[r].render_ms, sts[r].order_ms, sts[r].schedule = [10, 25, 7][r], [1, 2, 3][r], [2, 1, 2][r]
        # what a frame does not report, and a shard's own gather_ms / devices, must not leak through
        sts[r].extend_ms, sts[r].shade_ms, sts[r].extend_launches, sts[r].shade_launches = 5.0, 6.0, 7, 8
        sts[r].gather_ms, sts[r].devices = 99.0, 1
    out = rt.RtStats()
    ctypes.memset(ctypes.byref(out), 0xFF, ctypes.sizeof(out))
    assert fp.lib.fp_merge(ctypes.byref(i), sts, 1.5, ctypes.byref(out)) == 0
    for k, name in enumerate(counters):
        assert getattr(out, name) == 3 * 1000 * (k + 1) + 111
    assert out.render_ms == 25.0    # device 1's one shard against device 0's 10 + 7
    assert out.order_ms == 4.0      # device 0's 1 + 3 against device 1's 2
    assert out.schedule == 3 and out.devices == 2 and out.gather_ms == 1.5
    assert (out.extend_ms, out.shade_ms, out.extend_launches, out.shade_launches) == (0.0, 0.0, 0, 0)
