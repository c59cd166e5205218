"""hpgv_lines_multisplit_dev: a multi-way stable partition of variable-length lines on the device (bucket 0's lines back to
back in line order, then bucket 1's, ...; ids >= n_buckets go nowhere), byte for byte against a numpy stable argsort, with
d_bucket_off checked exactly and canary bytes on both sides of the output range (nothing stored outside it)."""
import ctypes as C

import numpy as np
import pytest

from helpers import hpgv
from test_lines_partition_gpu import CANARY, PAD, _Dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    L = hpgv.load()
    vp, sz = C.c_void_p, C.c_size_t
    L.hpgv_lines_multisplit_scratch_bytes.argtypes = [C.c_int, C.c_int]
    L.hpgv_lines_multisplit_scratch_bytes.restype = sz
    L.hpgv_lines_multisplit_dev.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.hpgv_lines_partition_scratch_bytes.argtypes = [C.c_int]
    L.hpgv_lines_partition_scratch_bytes.restype = sz
    L.hpgv_lines_partition_dev.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    ctx = vp()
    assert L.hpgv_create(0, C.byref(ctx)) == 0
    yield L, ctx
    L.hpgv_destroy(ctx)


def _text(lens, lead, seed):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    line_off = np.zeros(n + 1, np.uint64)
    line_off[0] = lead
    line_off[1:] = lead + np.cumsum(lens)
    text = rng.integers(0, 255, size=lead + int(lens.sum()), dtype=np.uint8)
    if n:
        text[(line_off[1:] - 1).astype(np.int64)] = ord("\n")
    return text, line_off


def _multisplit(dev, lens, bucket, n_buckets, src_off=0, dst_off=0, lead=0, seed=0, against_partition=False):
    """the lines at d_text + src_off, the output at d_out + dst_off; returns the output bytes"""
    L, ctx = dev
    bucket = np.asarray(bucket, np.uint8)
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    text, line_off = _text(lens, lead, seed)
    lines = [text[int(line_off[i]):int(line_off[i + 1])] for i in range(n)]
    order = np.argsort(bucket, kind="stable")
    exp = np.concatenate([lines[i] for i in order if bucket[i] < n_buckets] + [np.zeros(0, np.uint8)])
    sizes = np.array([int(lens[bucket == b].sum()) for b in range(n_buckets)], np.uint64)
    exp_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    kept = len(exp)
    span = PAD + 16 + int(lens.sum()) + PAD
    D = _Dev(L, ctx)
    try:
        d_text = D.alloc(src_off + len(text) + 16)
        D.put(d_text + src_off, text)
        d_line_off = D.alloc(8 * (n + 1))
        D.put(d_line_off, line_off)
        d_bucket = D.alloc(n)
        D.put(d_bucket, bucket)
        d_out = D.alloc(span)
        D.put(d_out, np.full(span, CANARY, np.uint8))
        d_boff = D.alloc(8 * (n_buckets + 3))
        D.put(d_boff, np.full(n_buckets + 3, 0xDEADBEEF, np.uint64))
        d_scratch = D.alloc(L.hpgv_lines_multisplit_scratch_bytes(n, n_buckets))
        rc = L.hpgv_lines_multisplit_dev(ctx, d_text + src_off, d_line_off, n, d_bucket, n_buckets, d_out + PAD + dst_off,
                                         d_boff + 8, d_scratch, None)
        assert rc == 0, L.hpgv_last_error(ctx)
        assert L.hpgv_stream_sync(ctx, None) == 0
        got = D.get(d_out, span)
        boff = D.get(d_boff, n_buckets + 3, np.uint64)
        if against_partition:
            d_out2, d_kept = D.alloc(span), D.alloc(8)
            D.put(d_out2, np.full(span, CANARY, np.uint8))
            d_keep = D.alloc(n)
            D.put(d_keep, (bucket == 0).astype(np.uint8))
            d_scr2 = D.alloc(L.hpgv_lines_partition_scratch_bytes(n))
            assert L.hpgv_lines_partition_dev(ctx, d_text + src_off, d_line_off, n, d_keep, d_out2 + PAD + dst_off, d_kept, d_scr2, None) == 0
            assert L.hpgv_stream_sync(ctx, None) == 0
            assert np.array_equal(D.get(d_out2, span), got)
    finally:
        D.free()
    lo = PAD + dst_off
    assert (got[:lo] == CANARY).all(), "stored in front of the output"
    assert (got[lo + kept:] == CANARY).all(), "stored behind the output"
    assert np.array_equal(got[lo:lo + kept], exp)
    assert boff[0] == 0xDEADBEEF and boff[n_buckets + 2] == 0xDEADBEEF, "bucket_off written outside its n_buckets + 1 entries"
    assert np.array_equal(boff[1:n_buckets + 2], exp_off)
    return got[lo:lo + kept]


@pytest.mark.parametrize("length", [1, 15, 16, 17, 64, 65])
def test_fixed_lengths_at_every_alignment(dev, length):
    rng = np.random.default_rng(length)
    n = 300
    bucket = rng.integers(0, 3, n)
    for src_off in range(16):
        for dst_off in range(16):
            _multisplit(dev, [length] * n, bucket, 3, src_off, dst_off, seed=src_off * 16 + dst_off)


@pytest.mark.parametrize("n_buckets", [1, 2, 3, 25, 255, 256])
@pytest.mark.parametrize("n_lines", [1, 63, 64, 65, 1023, 1025])
def test_bucket_counts_and_line_counts(dev, n_buckets, n_lines):
    rng = np.random.default_rng(n_buckets * 7919 + n_lines)
    lens = rng.integers(1, 300, n_lines)
    bucket = rng.integers(0, n_buckets, n_lines)
    _multisplit(dev, lens, bucket, n_buckets, n_lines % 16, n_buckets % 16, lead=n_lines % 5, seed=n_lines)


@pytest.mark.parametrize("n_buckets", [3, 25, 256])
def test_sorted_runs_and_empty_buckets(dev, n_buckets):
    rng = np.random.default_rng(3)
    lens = rng.integers(1, 2000, 5000)
    used = np.sort(rng.choice(n_buckets, size=max(1, n_buckets // 3), replace=False))
    bucket = np.repeat(used, -(-len(lens) // len(used)))[:len(lens)]
    _multisplit(dev, lens, bucket, n_buckets, 7, 9)


def test_everything_in_one_bucket(dev):
    rng = np.random.default_rng(4)
    lens = rng.integers(1, 5000, 3000)
    for b, nb in ((0, 1), (0, 25), (24, 25), (255, 256)):
        _multisplit(dev, lens, np.full(len(lens), b), nb, 3, 14)


def test_ids_at_or_past_n_buckets_go_nowhere(dev):
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 3000, 4000)
    for nb in (1, 2, 25, 255):
        bucket = rng.integers(0, 256, len(lens))
        _multisplit(dev, lens, bucket, nb, 11, 2, lead=9)
    _multisplit(dev, lens, np.full(len(lens), 200), 25, 1, 1)      # nothing at all stored


def test_mixed_lengths_1b_to_40kb(dev):
    rng = np.random.default_rng(9)
    lens = np.concatenate([rng.integers(1, 130, 3000), rng.integers(1000, 40000, 60), rng.integers(1, 18, 3000),
                           rng.integers(300, 3000, 500)])
    rng.shuffle(lens)
    for nb, (src_off, dst_off) in zip((2, 25, 255), [(0, 5), (7, 0), (13, 9)]):
        _multisplit(dev, lens, rng.integers(0, nb, len(lens)), nb, src_off, dst_off, lead=33, seed=src_off)
    for mean in (20, 200, 2000, 40000):                             # every lanes-per-line choice, with outliers among them
        lens = np.maximum(1, rng.normal(mean, mean / 3, 400)).astype(np.int64)
        lens[::37] = 1
        _multisplit(dev, lens, rng.integers(0, 25, len(lens)), 25, mean % 16, 3, seed=mean)


def test_one_hundred_thousand_lines(dev):
    rng = np.random.default_rng(11)
    lens = rng.integers(1, 200, 100_000)
    _multisplit(dev, lens, rng.integers(0, 255, len(lens)), 255, 5, 3, seed=1)
    _multisplit(dev, lens, np.sort(rng.integers(0, 25, len(lens))), 25, 0, 0, seed=2)


def test_two_buckets_equal_the_partition(dev):
    rng = np.random.default_rng(12)
    for trial, (lens, src_off, dst_off) in enumerate([(rng.integers(1, 40, 20000), 3, 5), (rng.integers(1, 5000, 3000), 0, 13),
                                                     (rng.integers(20000, 40000, 40), 9, 1)]):
        _multisplit(dev, lens, rng.integers(0, 2, len(lens)), 2, src_off, dst_off, lead=trial, seed=trial, against_partition=True)


def test_zero_lines(dev):
    L, ctx = dev
    D = _Dev(L, ctx)
    try:
        d_boff = D.alloc(8 * 26)
        D.put(d_boff, np.full(26, 7, np.uint64))
        assert L.hpgv_lines_multisplit_dev(ctx, None, None, 0, None, 25, None, d_boff, None, None) == 0
        assert L.hpgv_stream_sync(ctx, None) == 0
        assert (D.get(d_boff, 26, np.uint64) == 0).all()
    finally:
        D.free()
    assert L.hpgv_lines_multisplit_dev(ctx, None, None, 0, None, 0, None, None, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_lines_multisplit_dev(ctx, None, None, 0, None, 257, None, None, None, None) == hpgv.ERR_INVALID
