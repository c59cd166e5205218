"""hpgv_lines_partition_dev: a stable partition of variable-length lines on the device (the kept lines back to back in line
order, then the others in line order), byte for byte against a numpy partition, at every alignment of the source and the
destination, with canary bytes on both sides of the output range (nothing stored outside it)."""
import ctypes as C

import numpy as np
import pytest

from helpers import hpgv

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 64


@pytest.fixture(scope="module")
def dev():
    L = hpgv.load()
    vp, sz = C.c_void_p, C.c_size_t
    L.hpgv_lines_partition_scratch_bytes.argtypes = [C.c_int]
    L.hpgv_lines_partition_scratch_bytes.restype = sz
    L.hpgv_lines_partition_dev.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    ctx = vp()
    assert L.hpgv_create(0, C.byref(ctx)) == 0
    yield L, ctx
    L.hpgv_destroy(ctx)


class _Dev:
    """device buffers of one call, freed at the end"""

    def __init__(self, L, ctx):
        self.L, self.ctx, self.ptrs = L, ctx, []

    def alloc(self, n):
        p = C.c_void_p()
        assert self.L.hpgv_dev_alloc(self.ctx, max(n, 16), C.byref(p)) == 0
        self.ptrs.append(p)
        return p.value

    def put(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes:
            assert self.L.hpgv_memcpy_h2d(self.ctx, dptr, arr.ctypes.data, arr.nbytes, None) == 0

    def get(self, dptr, n, dtype=np.uint8):
        out = np.empty(n, dtype)
        if out.nbytes:
            assert self.L.hpgv_memcpy_d2h(self.ctx, out.ctypes.data, dptr, out.nbytes, None) == 0
        return out

    def free(self):
        for p in self.ptrs:
            self.L.hpgv_dev_free(self.ctx, p)


def _partition(dev, lens, keep, src_off=0, dst_off=0, lead=0, seed=0):
    """lines of the given lengths (random bytes, each ending in '\\n'), `lead` bytes of something else in front of the first
    line (line_off[0] = lead), the text at d_text + src_off and the output at d_out + dst_off"""
    L, ctx = dev
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    keep = np.asarray(keep, np.uint8)
    n = len(lens)
    line_off = np.zeros(n + 1, np.uint64)
    line_off[0] = lead
    line_off[1:] = lead + np.cumsum(lens)
    total = int(lens.sum())
    text = rng.integers(0, 255, size=lead + total, dtype=np.uint8)
    if n:
        text[(line_off[1:] - 1).astype(np.int64)] = ord("\n")
    D = _Dev(L, ctx)
    try:
        d_text = D.alloc(src_off + len(text) + 16)
        D.put(d_text + src_off, text)
        d_line_off = D.alloc(8 * (n + 1))
        D.put(d_line_off, line_off)
        d_keep = D.alloc(n)
        D.put(d_keep, keep)
        d_out = D.alloc(PAD + 16 + total + PAD)
        D.put(d_out, np.full(PAD + 16 + total + PAD, CANARY, np.uint8))
        d_kept = D.alloc(8)
        D.put(d_kept, np.array([0xDEADBEEF], np.uint64))
        scratch = L.hpgv_lines_partition_scratch_bytes(n)
        d_scratch = D.alloc(scratch)
        rc = L.hpgv_lines_partition_dev(ctx, d_text + src_off, d_line_off, n, d_keep, d_out + PAD + dst_off, d_kept, d_scratch, None)
        assert rc == 0, hpgv.load().hpgv_last_error(ctx)
        assert L.hpgv_stream_sync(ctx, None) == 0
        got = D.get(d_out, PAD + 16 + total + PAD)
        kept_bytes = int(D.get(d_kept, 1, np.uint64)[0])
    finally:
        D.free()
    lines = [text[int(line_off[i]):int(line_off[i + 1])] for i in range(n)]
    exp = np.concatenate([l for l, k in zip(lines, keep) if k] + [l for l, k in zip(lines, keep) if not k] + [np.zeros(0, np.uint8)])
    lo = PAD + dst_off
    assert (got[:lo] == CANARY).all(), "stored in front of the output"
    assert (got[lo + total:] == CANARY).all(), "stored behind the output"
    assert np.array_equal(got[lo:lo + total], exp)
    assert kept_bytes == int(lens[keep.astype(bool)].sum())


@pytest.mark.parametrize("length", [1, 15, 16, 17, 63, 64, 65])
def test_fixed_lengths_at_every_alignment(dev, length):
    rng = np.random.default_rng(length)
    n = 300
    keep = rng.integers(0, 2, n)
    for src_off in range(16):
        for dst_off in range(16):
            _partition(dev, [length] * n, keep, src_off, dst_off, seed=src_off * 16 + dst_off)


def test_random_lengths_up_to_256k(dev):
    rng = np.random.default_rng(5)
    for trial, (src_off, dst_off) in enumerate([(0, 0), (3, 11), (15, 1), (8, 8), (1, 15)]):
        lens = rng.integers(1, 256 << 10, size=24)
        lens[::5] = rng.integers(1, 200, size=len(lens[::5]))        # short ones among them
        _partition(dev, lens, rng.integers(0, 2, len(lens)), src_off, dst_off, lead=trial * 7, seed=trial)


def test_mixed_lengths_and_a_leading_offset(dev):
    rng = np.random.default_rng(9)
    lens = np.concatenate([rng.integers(1, 130, 3000), rng.integers(1000, 20000, 40), rng.integers(1, 18, 3000)])
    rng.shuffle(lens)
    for src_off, dst_off in [(0, 5), (7, 0), (13, 9)]:
        _partition(dev, lens, rng.integers(0, 2, len(lens)), src_off, dst_off, lead=33, seed=src_off)


def test_one_million_short_lines(dev):
    rng = np.random.default_rng(11)
    lens = rng.integers(1, 40, 1_000_000)
    _partition(dev, lens, rng.integers(0, 2, len(lens)), 5, 3, seed=1)


@pytest.mark.parametrize("which", ["all", "none"])
def test_all_kept_or_none(dev, which):
    rng = np.random.default_rng(2)
    lens = rng.integers(1, 3000, 5000)
    keep = np.ones(len(lens)) if which == "all" else np.zeros(len(lens))
    _partition(dev, lens, keep, 6, 10)


def test_zero_and_one_line(dev):
    _partition(dev, [], [], 3, 4)
    for length in (1, 17, 5000):
        for k in (0, 1):
            _partition(dev, [length], [k], 9, 2)
