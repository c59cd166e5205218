"""hpgv_bgzf_deflate_dev / hpgv_bgzf_compress / the _bgzf twins of the partition and the multisplit: BGZF members deflated on
the device.  Every member is checked against the format in Python (header bytes, BSIZE, ISIZE, a raw DEFLATE payload that zlib
inflates to exactly the block's text, CRC-32), on text lengths around every block and window boundary and on contents that
reach the format's limits (distance 1 and 32 768, length 258, 9-bit literals, incompressible bytes); the segments' bounds, the
canaries around the output, the project's own decoder and determinism."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

from helpers import hpgv

pytestmark = pytest.mark.gpu

BLOCK = 65280
EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 258, 259, 260, 4095, 4096, 32767, 32768, 32769, 65279, 65280, 65281, 130560, 130561, 200000]
CANARY, PAD = 0xA5, 4096


@pytest.fixture(scope="module")
def eng():
    e = hpgv.Engine(0)
    yield e
    e.close()


def _genotype_text(n_bytes, seed, n_samples=200):
    """VCF records of n_samples genotypes, d/d, d|d or ./. drawn per line with a random allele frequency (as the runner tests)"""
    rng = np.random.default_rng(seed)
    out, size, v = [], 0, 0
    while size < n_bytes:
        af = rng.random() * 0.5
        a = rng.random((n_samples, 2)) < af
        sep = np.where(rng.random(n_samples) < 0.5, "/", "|")
        miss = rng.random(n_samples) < 0.02
        gts = ["./." if m else "%d%s%d" % (x, s, y) for (x, y), s, m in zip(a, sep, miss)]
        line = ("%d\t%d\trs%d\tA\tC\t%d\tPASS\tDP=%d\tGT\t%s\n" % (1 + v % 22, 1000 + 7 * v, v, 10 + v % 80, v % 300, "\t".join(gts))).encode()
        out.append(line); size += len(line); v += 1
    return b"".join(out)[:n_bytes]


def _no_repeat(n, width, alphabet, seed):
    """n random bytes of the alphabet in which no `width` consecutive bytes occur twice"""
    rng = np.random.default_rng(seed)
    draws = rng.integers(0, len(alphabet), size=4 * n + 64)
    seen, out, k = set(), bytearray(), 0
    while len(out) < n:
        c = alphabet[draws[k % len(draws)]]; k += 1
        if len(out) >= width - 1:
            key = bytes(out[len(out) - width + 1:]) + bytes([c])
            if key in seen:
                continue
            seen.add(key)
        out.append(c)
    return bytes(out)


@pytest.fixture(scope="module")
def contents():
    """the six kinds of text, each as long as the longest case; a case takes its first n bytes"""
    top = max(LENGTHS + [3 * BLOCK, 300000])
    rng = np.random.default_rng(17)
    p1, p2 = bytes(rng.integers(0, 256, 32768, dtype=np.uint8)), bytes(rng.integers(0, 256, 32769, dtype=np.uint8))
    every = _no_repeat(top, 3, list(range(256)), 3)               # (e): no three bytes twice
    assert set(every[:4096]) == set(range(256))
    threes = _no_repeat(top, 4, list(range(64, 104)), 4)          # (f): 40 symbols -- three bytes repeat all the time, four never
    tri = [threes[i:i + 3] for i in range(0, 30000)]
    assert len(set(tri)) < len(tri)
    return {"a": _genotype_text(top, 1), "b": b"G" * top, "c": bytes(rng.integers(0, 256, top, dtype=np.uint8)),
            "d1": (p1 * (top // len(p1) + 1))[:top], "d2": (p2 * (top // len(p2) + 1))[:top], "e": every, "f": threes}


def _deflate(e, text, cuts, src_off=0, dst_off=0):
    """the members of text cut at `cuts` (segment bounds, len n_segs + 1) -> (output bytes, seg_out_off); canaries checked"""
    L = e.L
    n_segs = len(cuts) - 1
    bound = L.hpgv_bgzf_deflate_bound(len(text), n_segs)
    scratch = L.hpgv_bgzf_deflate_scratch_bytes(len(text), n_segs)
    bufs = []
    try:
        d_text = e.alloc(src_off + len(text) + 16); bufs.append(d_text)
        if text:
            e.h2d(C.c_void_p(d_text.value + src_off), np.frombuffer(text, np.uint8))
        d_seg = e.alloc(8 * (n_segs + 1)); bufs.append(d_seg)
        e.h2d(d_seg, np.asarray(cuts, np.uint64))
        room = PAD + 16 + bound + PAD
        d_out = e.alloc(room); bufs.append(d_out)
        e.h2d(d_out, np.full(room, CANARY, np.uint8))
        d_so = e.alloc(8 * (n_segs + 1)); bufs.append(d_so)
        d_scr = e.alloc(max(scratch, 16)); bufs.append(d_scr)
        rc = L.hpgv_bgzf_deflate_dev(e.h, d_text.value + src_off, d_seg, n_segs, d_out.value + PAD + dst_off, d_so, d_scr, None)
        assert rc == 0, L.hpgv_last_error(e.h)
        e.sync()
        seg_out = [int(x) for x in e.d2h(d_so, (n_segs + 1,), np.uint64)]
        got = e.d2h(d_out, (room,), np.uint8)
    finally:
        for b in bufs:
            e.free(b)
    used = seg_out[-1]
    assert used <= bound
    lo = PAD + dst_off
    assert (got[:lo] == CANARY).all(), "stored in front of the output"
    assert (got[lo + used:] == CANARY).all(), "stored behind the output"
    return got[lo:lo + used].tobytes(), seg_out


def _members(data):
    """walks whole members by BSIZE -> [(member bytes, text)], every one checked against the format"""
    out, at = [], 0
    while at < len(data):
        assert len(data) - at >= 26
        assert data[at:at + 16] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]), at
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert size <= 65536 and at + size <= len(data)
        m = data[at:at + size]
        crc, isize = struct.unpack_from("<II", m, size - 8)
        assert isize <= BLOCK
        z = zlib.decompressobj(-15)
        text = z.decompress(m[18:])
        assert z.eof and z.unused_data == m[size - 8:], "the payload is one complete DEFLATE stream, the trailer right behind it"
        assert len(text) == isize and zlib.crc32(text) == crc
        out.append((m, text))
        at += size
    return out


@pytest.mark.parametrize("kind", ["a", "b", "c", "d1", "d2", "e", "f"])
def test_every_member_is_what_the_format_says(eng, contents, kind):
    for n in LENGTHS:
        text = contents[kind][:n]
        data, seg_out = _deflate(eng, text, [0, n])
        ms = _members(data)
        assert len(ms) == -(-n // BLOCK), n
        assert [t for _, t in ms] == [text[i:i + BLOCK] for i in range(0, n, BLOCK)], n
        assert gzip.decompress(data + EOF) == text, n
        assert seg_out == [0, len(data)] and len(data) <= eng.L.hpgv_bgzf_deflate_bound(n, 1)
        if kind == "c":                                            # incompressible: stored, never more than 31 bytes beyond the text
            assert all(len(m) <= len(t) + 31 for m, t in ms), n


def test_compressible_text_is_compressed(eng, contents):
    # a condition, not a measurement: "everything stored" must not pass (zlib level 1 with fixed codes: 0.19 - 0.22 on such text)
    for kind in ("a", "b"):
        text = contents[kind][:3 * BLOCK]
        data, _ = _deflate(eng, text, [0, len(text)])
        assert gzip.decompress(data + EOF) == text
        assert len(data) <= 0.5 * len(text), (kind, len(data), len(text))


def _cuts(n_segs, total, rng):
    if n_segs == 1:
        return [0, total]
    if n_segs == 2:
        return [0, 3 * BLOCK + 5, total]                           # more than two blocks, then the rest
    if n_segs == 7:                                                # two empty ones in front, four members, an empty one, one byte
        return [0, 0, 0, 3 * BLOCK + 77, 3 * BLOCK + 77, 3 * BLOCK + 78, 250000, total]
    cuts = [0] + sorted(int(x) for x in rng.integers(0, total, size=n_segs - 1)) + [total]
    cuts[2] = cuts[1]                                              # an empty segment, two adjacent empty ones, a one-byte segment
    cuts[5] = cuts[4] = cuts[3]
    cuts[6] = cuts[5] + 1
    return sorted(cuts)


@pytest.mark.parametrize("n_segs", [1, 2, 7, 256])
def test_segments(eng, contents, n_segs):
    text = contents["a"][:300000]
    cuts = _cuts(n_segs, len(text), np.random.default_rng(n_segs))
    lens = np.diff(cuts)
    if n_segs > 2:
        assert (lens == 0).any() and ((lens[:-1] == 0) & (lens[1:] == 0)).any() and (lens == 1).any()
    if n_segs in (2, 7):
        assert (lens > 2 * BLOCK).any()
    ref = None
    for src_off, dst_off in ((0, 0), (1, 0), (0, 1), (3, 7), (7, 3)):
        data, seg_out = _deflate(eng, text, cuts, src_off, dst_off)
        assert all(a <= b for a, b in zip(seg_out, seg_out[1:])) and seg_out[0] == 0 and seg_out[-1] == len(data)
        for s in range(n_segs):
            part = data[seg_out[s]:seg_out[s + 1]]
            if cuts[s] == cuts[s + 1]:
                assert part == b""
            else:
                assert b"".join(t for _, t in _members(part)) == text[cuts[s]:cuts[s + 1]], s
        assert ref is None or data == ref, "the bytes do not depend on the buffers' alignment"
        ref = data


def test_the_projects_own_reader_takes_it(eng, contents):
    e, L = eng, eng.L
    text = contents["a"][:200000] + contents["c"][:70000] + contents["b"][:1000] + contents["f"][:5000]
    data, _ = _deflate(e, text, [0, 200000, 270000, len(text)])
    n_mem = len(_members(data))
    size = len(data)
    d_comp = e.alloc(size + 16)
    e.h2d(d_comp, np.frombuffer(data + b"\0" * 16, np.uint8))
    cap = 64
    d_io, d_il, d_oo, d_ol = e.alloc(8 * cap), e.alloc(4 * cap), e.alloc(8 * cap), e.alloc(4 * cap)
    n, end, text_end, _ = e.bgzf_scan(d_comp, 0, size, 0, cap, d_io, d_il, d_oo, d_ol)
    assert (n, end, text_end) == (n_mem, size, len(text))
    d_text, d_st = e.alloc(len(text) + 16), e.alloc(4 * cap)
    e.h2d(d_st, np.full(cap, -1, np.int32))
    assert L.hpgv_inflate_blocks_dev(e.h, d_comp, d_io, d_il, d_oo, d_ol, n, d_text, d_st, None) == 0
    e.sync()
    assert (e.d2h(d_st, (n,), np.int32) == 0).all(), "a block was refused"
    e.bgzf_verify(d_comp, d_io, d_il, d_oo, d_ol, n, d_text, d_st)
    e.sync()
    assert (e.d2h(d_st, (n,), np.int32) == 0).all(), "a block's CRC-32 does not match"
    assert e.d2h(d_text, (len(text),), np.uint8).tobytes() == text
    for b in (d_comp, d_io, d_il, d_oo, d_ol, d_text, d_st):
        e.free(b)


def test_deterministic(eng, contents):
    text = contents["a"][:250000] + contents["c"][:1000]
    cuts = [0, 100, 100, 140000, len(text)]
    assert _deflate(eng, text, cuts)[0] == _deflate(eng, text, cuts)[0]


def test_compress_on_host_buffers(eng, contents):
    e, L = eng, eng.L
    for text in (contents["a"][:150000], contents["c"][:70000], b"x", b""):
        cap = L.hpgv_bgzf_deflate_bound(len(text), 1)
        out = np.full(cap + 8, CANARY, np.uint8)
        made = C.c_size_t(12345)
        src = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
        assert L.hpgv_bgzf_compress(e.h, src.ctypes.data, len(text), out.ctypes.data, cap, C.byref(made)) == 0, L.hpgv_last_error(e.h)
        assert made.value <= cap and (out[made.value:] == CANARY).all()
        assert gzip.decompress(out[:made.value].tobytes() + EOF) == text
        assert b"".join(t for _, t in _members(out[:made.value].tobytes())) == text
        if text:                                                   # one byte short: refused, nothing written
            out[:] = CANARY
            assert L.hpgv_bgzf_compress(e.h, src.ctypes.data, len(text), out.ctypes.data, made.value - 1, C.byref(made)) == hpgv.ERR_INVALID
            assert (out == CANARY).all()


def _vcf_batch(n_lines, seed):
    rng = np.random.default_rng(seed)
    lines = []
    for v in range(n_lines):
        gts = "\t".join(rng.choice(["0/0", "0/1", "1/1", "./."], size=60, p=[0.6, 0.25, 0.14, 0.01]))
        lines.append(("%d\t%d\trs%d\tA\tC\t50\tPASS\tDP=%d\tGT\t%s\n" % (1 + v % 5, 100 + v, v, v % 90, gts)).encode())
    return lines


def test_the_bgzf_twins_against_the_plain_twins(eng):
    e, L = eng, eng.L
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    L.hpgv_filter_text.argtypes = [vp, vp, sz, i32, C.POINTER(i32), vp, vp, vp]
    L.hpgv_text_partition.argtypes = [vp, vp, vp, i32, vp, sz, vp, vp]
    L.hpgv_text_multisplit.argtypes = [vp, vp, vp, i32, i32, i32, vp, sz, vp]
    lines = _vcf_batch(900, 8)                                     # ~230 KB: several blocks in a part
    n = len(lines)
    text = np.frombuffer(b"".join(lines), np.uint8).copy()
    assert L.hpgv_set_stats_cohort(e.h, 60) == 0
    rng = np.random.default_rng(9)
    keep = rng.integers(0, 2, n).astype(np.uint8)
    bucket = rng.integers(0, 5, n).astype(np.uint8)
    bucket[bucket == 3] = 4                                        # bucket 3 stays empty

    def hold():
        nl = i32(0)
        lo, fo, st = np.zeros(n + 1, np.uint64), np.zeros(10 * n, np.uint32), np.zeros(n, np.int32)
        assert L.hpgv_filter_text(e.h, text.ctypes.data, text.nbytes, n, C.byref(nl), lo.ctypes.data, fo.ctypes.data, st.ctypes.data) == 0, L.hpgv_last_error(e.h)
        assert nl.value == n

    # partition
    plain = np.zeros(text.nbytes, np.uint8)
    kb, tb = C.c_uint64(0), C.c_uint64(0)
    hold()
    assert L.hpgv_text_partition(e.h, text.ctypes.data, keep.ctypes.data, n, plain.ctypes.data, plain.nbytes, C.byref(kb), C.byref(tb)) == 0
    plain_kept, plain_rest = plain[:kb.value].tobytes(), plain[kb.value:tb.value].tobytes()
    cap = L.hpgv_bgzf_deflate_bound(text.nbytes, 2)
    for want_rest in (1, 0):
        out = np.full(cap, CANARY, np.uint8)
        comp, last = (C.c_uint64 * 2)(), (C.c_uint8 * 2)()
        kb2, tb2 = C.c_uint64(0), C.c_uint64(0)
        hold()
        assert L.hpgv_text_partition_bgzf(e.h, text.ctypes.data, keep.ctypes.data, n, out.ctypes.data, cap, want_rest,
                                          C.byref(kb2), C.byref(tb2), comp, last) == 0, L.hpgv_last_error(e.h)
        assert (kb2.value, tb2.value) == (kb.value, tb.value)
        assert b"".join(t for _, t in _members(out[:comp[0]].tobytes())) == plain_kept
        assert b"".join(t for _, t in _members(out[comp[0]:comp[0] + comp[1]].tobytes())) == (plain_rest if want_rest else b"")
        assert (out[comp[0] + comp[1]:] == CANARY).all() and bytes(last) == b"\n\n"
        made = comp[0] + comp[1]
    out[:] = CANARY                                                # one byte short (want_rest = 0: `made` is the kept members)
    hold()
    assert L.hpgv_text_partition_bgzf(e.h, text.ctypes.data, keep.ctypes.data, n, out.ctypes.data, made - 1, 0, None, None, None, None) == hpgv.ERR_INVALID
    assert (out == CANARY).all()

    # multisplit: lines [100, 800) into 6 buckets (ids 0, 1, 2, 4 used; 3 and 5 empty)
    first, m, nb = 100, 700, 6
    boff, boff2 = np.zeros(nb + 1, np.uint64), np.zeros(nb + 1, np.uint64)
    hold()
    assert L.hpgv_text_multisplit(e.h, text.ctypes.data, bucket[first:].ctypes.data, first, m, nb, plain.ctypes.data, plain.nbytes, boff.ctypes.data) == 0
    out[:] = CANARY
    last = (C.c_uint8 * nb)()
    assert L.hpgv_text_multisplit_bgzf(e.h, text.ctypes.data, bucket[first:].ctypes.data, first, m, nb, out.ctypes.data, cap, boff2.ctypes.data, last) == 0, L.hpgv_last_error(e.h)
    for b in range(nb):
        got = b"".join(t for _, t in _members(out[int(boff2[b]):int(boff2[b + 1])].tobytes()))
        assert got == plain[int(boff[b]):int(boff[b + 1])].tobytes(), b
    assert boff2[3] == boff2[4] and boff2[5] == boff2[6] and (out[int(boff2[nb]):] == CANARY).all() and bytes(last) == b"\n" * nb
    out[:] = CANARY
    assert L.hpgv_text_multisplit_bgzf(e.h, text.ctypes.data, bucket[first:].ctypes.data, first, m, nb, out.ctypes.data, int(boff2[nb]) - 1, boff2.ctypes.data, None) == hpgv.ERR_INVALID
    assert (out == CANARY).all()
    assert L.hpgv_text_partition(e.h, text.ctypes.data, None, 0, None, 0, None, None) == 0        # the hold released
