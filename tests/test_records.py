"""The accumulator's 32-byte per-pixel records (raytracing-hw_amd/csrc/rt_records.h behind
tests/native/records_host.cpp) without a GPU: pack and unpack of the three kinds round-trip, every
field lies where the hand-built records of the checkpoint tests put it (test_accum.py _records,
test_fast_accum.py fast_records, moments_util.py moment_records: numpy's statement of the format,
written from include/rt_hw.h and not from the header under test), and the two checkpoint checks
give what the shims of test_fast_accum.py and test_moments.py give on those tests' cases."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from moments_util import moment_records, twin
from test_accum import _records
from test_fast_accum import GXX, fast_records, fu  # noqa: F401  (fu: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "records_host.cpp")
N = 1000


@pytest.fixture(scope="module")
def rh(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rh") / "librh.so")
    subprocess.run(GXX + ["-shared", "-fPIC", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    V, I, L, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint
    for name in ("parity", "fast", "moment"):
        for way in ("pack", "unpack"):
            f = getattr(lib, f"rh_{name}_{way}")
            f.argtypes, f.restype = [L, V, V], None
    lib.rh_next_of.argtypes, lib.rh_next_of.restype = [V, L], U
    lib.rh_open_words_fit.argtypes = [U, I, V]
    lib.rh_record_words_fit.argtypes = [U, I, V]
    return lib


@pytest.fixture(scope="module")
def words():
    """N random records, then the all-zero record and one whose state word (word 2) is all ones."""
    w = np.random.default_rng(17).integers(0, 1 << 32, (N + 2, 8), dtype=np.uint64).astype(np.uint32)
    w[N] = 0
    w[N + 1] = 0
    w[N + 1, 2] = 0xffffffff
    w.setflags(write=False)
    return w


def call(f, src, width):
    src = np.ascontiguousarray(src, np.uint32)
    out = np.full((len(src), width), 0xdeadbeef, np.uint32)
    f(len(src), src.ctypes.data, out.ctypes.data)
    return out


def open_where(is_open, value):
    """(P, 3) float32: `value` in the rows where a chunk is open, +0 elsewhere."""
    return np.where(is_open[:, None], np.float32(value), np.float32(0)) * np.ones((1, 3), np.float32)


def test_parity_records(rh, words):
    assert rh.rh_words() == 8
    f = call(rh.rh_parity_unpack, words, 8)
    # pixel, next | engine state, cache flag (bit 31 of word 2) | cached value | sum
    assert np.array_equal(f[:, 0], words[:, 0]) and np.array_equal(f[:, 1], words[:, 1])
    assert np.array_equal(f[:, 2], words[:, 2] & 0x7fffffff) and np.array_equal(f[:, 3], words[:, 2] >> 31)
    assert np.array_equal(f[:, 4], words[:, 3]) and np.array_equal(f[:, 5:8], words[:, 4:7])
    assert f[N + 1, 2] == 0x7fffffff and f[N + 1, 3] == 1
    back = call(rh.rh_parity_pack, f, 8)
    assert np.array_equal(back[:, :7], words[:, :7]) and not back[:, 7].any()
    # the hand-built records of test_accum.py: pixel k at `samples`, engine state k + 1, nothing else
    rec = np.frombuffer(_records(50, 3), "<u4").reshape(50, 8)
    f = call(rh.rh_parity_unpack, rec, 8)
    assert np.array_equal(f[:, 0], np.arange(50)) and (f[:, 1] == 3).all() and np.array_equal(f[:, 2], np.arange(50) + 1)
    assert not f[:, 3:].any() and np.array_equal(call(rh.rh_parity_pack, f, 8), rec)


def test_fast_records(rh, words):
    f = call(rh.rh_fast_unpack, words, 8)
    assert np.array_equal(f, words)   # pixel, next, total (words 2-4), open (words 5-7): the words in order
    assert np.array_equal(call(rh.rh_fast_pack, f, 8), words)
    nxt = np.where(np.arange(50) % 3 == 0, 7, 6)
    rec = fast_records(50, nxt, 3)   # total 1.5 everywhere, open 0.25 where next % 3 != 0
    f = call(rh.rh_fast_unpack, rec, 8)
    assert np.array_equal(f[:, 0], np.arange(50)) and np.array_equal(f[:, 1], nxt)
    assert np.array_equal(f[:, 2:5].view(np.float32), np.full((50, 3), 1.5, np.float32))
    assert np.array_equal(f[:, 5:8].view(np.float32), open_where(nxt % 3 != 0, 0.25))
    assert np.array_equal(call(rh.rh_fast_pack, f, 8), rec)
    flat = np.ascontiguousarray(rec)
    assert [rh.rh_next_of(flat.ctypes.data, p) for p in (0, 1, 49)] == [7, 6, 6]


def test_moment_records(rh, words):
    f = call(rh.rh_moment_unpack, words, 6)
    assert np.array_equal(f, words[:, :6])   # total2 (words 0-2), open2 (words 3-5)
    back = call(rh.rh_moment_pack, f, 8)
    assert np.array_equal(back[:, :6], words[:, :6]) and not back[:, 6:].any()
    nxt = np.where(np.arange(50) % 3 == 0, 7, 6)
    rec = moment_records(50, nxt, 3)   # total2 2.25 everywhere, open2 0.0625 where next % 3 != 0
    f = call(rh.rh_moment_unpack, rec, 6)
    assert np.array_equal(f[:, 0:3].view(np.float32), np.full((50, 3), 2.25, np.float32))
    assert np.array_equal(f[:, 3:6].view(np.float32), open_where(nxt % 3 != 0, 0.0625))
    assert np.array_equal(call(rh.rh_moment_pack, f, 8), rec)


def test_checkpoint_checks_agree_with_the_shims(rh, fu, tmp_path_factory):  # noqa: F811
    mh = twin(tmp_path_factory)
    # test_fast_accum.py test_open_words_rule's cases, the open words at their place in a whole record
    z, nz = np.zeros(3, np.uint32), np.array([0, 0, 1], np.uint32)
    for nxt, c, opn in ((6, 3, z), (6, 3, nz), (7, 3, z), (7, 3, nz), (0, 1, nz)):
        rec = fast_records(1, nxt, c)[0]
        rec[5:8] = opn
        want = bool(fu.fu_open_words_fit(nxt, c, opn.ctypes.data))
        assert bool(rh.rh_open_words_fit(nxt, c, rec.ctypes.data)) == want == (nxt % c != 0 or not opn.any()), (nxt, c, opn)
    # test_moments.py test_record_words_rule's cases
    zero = np.zeros(8, np.uint32)
    cases = [zero, np.array([5, 5, 5, 0, 0, 0, 0, 0], np.uint32)]
    for word in (3, 4, 5, 6, 7):
        cases.append(zero.copy())
        cases[-1][word] = 1
    for rec in cases:
        for nxt in (6, 7):
            want = bool(mh.mh_record_words_fit(nxt, 3, rec.ctypes.data))
            assert bool(rh.rh_record_words_fit(nxt, 3, rec.ctypes.data)) == want == (nxt % 3 != 0 or not rec[3:].any()), (nxt, rec)
