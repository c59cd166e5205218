"""GPU suite: the device inflate decoders (hpgv_inflate_blocks_dev) on DEFLATE streams that zlib's encoder never emits --
the hand-assembled corpus of tests/deflate_corpus.py, which tests/test_deflate_streams_cpu.py pins to zlib's inflate.  The
device decoder is the accelerator and zlib the arbiter: a legal stream of a must-take class comes back bit for bit, one of the two
may-refuse classes comes back right or with a status, and a stream is only ever taken if zlib takes the same bytes as the same
text."""
import numpy as np
import pytest

import deflate_corpus as dc
from helpers import hpgv, set_or_skip

pytestmark = pytest.mark.gpu

# The legal classes a device decoder may refuse (status != 0: the host decodes the block); every other legal class must be taken.
MAY_BE_REFUSED = ["no_distance_code", "single_litlen_code_length_1"]
GAP = 64                                              # guard bytes in front of and behind every text
FILL = 0xA5


@pytest.fixture(scope="module")
def cases():
    return dc.corpus()


@pytest.fixture(scope="module")
def plan(cases):
    buf, in_off, in_len, out_off, out_len, total = dc.layout(cases, GAP)
    return (np.frombuffer(buf, np.uint8), np.array(in_off, np.uint64), np.array(in_len, np.uint32), np.array(out_off, np.uint64),
            np.array(out_len, np.uint32), total)


@pytest.mark.parametrize("wave", [4, 2, 0, 3], ids=["wave_per_block_several_symbols", "wave_per_block", "lane_per_block", "lane_per_block_lds_tables"])
def test_inflate_hand_assembled_streams(cases, plan, wave):
    cbytes, in_off, in_len, out_off, out_len, total = plan
    n = len(cases)
    e = hpgv.Engine(0)
    set_or_skip(e, "inflate_wave", wave)
    d_comp, d_text = e.alloc(len(cbytes)), e.alloc(total + 16)         # (the streams end four bytes before the buffer does)
    d_io, d_il, d_oo, d_ol, d_st = e.alloc(8 * n), e.alloc(4 * n), e.alloc(8 * n), e.alloc(4 * n), e.alloc(4 * n)
    for d, a in ((d_comp, cbytes), (d_io, in_off), (d_il, in_len), (d_oo, out_off), (d_ol, out_len)):
        e.h2d(d, a)
    e.h2d(d_text, np.full(total + 16, FILL, np.uint8))
    e.inflate_blocks(d_comp, d_io, d_il, d_oo, d_ol, n, d_text, d_st)
    e.sync()
    status = e.d2h(d_st, (n,), np.int32)
    text = e.d2h(d_text, (total + 16,), np.uint8).tobytes()
    e.close()
    assert sorted({c.cls for c in cases if c.kind == dc.MAY}) == sorted(MAY_BE_REFUSED)
    failed, refused = [], []
    for k, c in enumerate(cases):
        a, m, st = int(out_off[k]), c.out_len, int(status[k])
        got = text[a:a + m]
        if text[a - GAP:a] != bytes([FILL]) * GAP:
            failed.append("%s: bytes in front of its text were written (status %d)" % (c.name, st))
        if text[a + m:a + m + GAP] != bytes([FILL]) * GAP:
            failed.append("%s: bytes behind its text were written (status %d)" % (c.name, st))
        if c.kind == dc.MUST:
            if st != 0:
                failed.append("%s: refused with status %d" % (c.name, st))
            elif got != c.text:
                at = next(i for i in range(m) if got[i] != c.text[i])
                failed.append("%s: wrong text from byte %d of %d on" % (c.name, at, m))
        elif c.kind == dc.MAY:
            assert c.cls in MAY_BE_REFUSED
            if st != 0:
                refused.append(c.name)
            elif got != c.text:
                failed.append("%s: taken, with a wrong text" % c.name)
        elif st == 0:                                                   # illegal and taken: only if zlib takes it as this text
            want = dc.zlib_takes(c.comp, m)
            if want is None or want != got:
                failed.append("%s: taken, and zlib %s" % (c.name, "does not take it" if want is None else "reads another text"))
    print("inflate_wave = %d refused of the may-refuse classes: %s" % (wave, refused or "none"))
    assert not failed, "%d of %d streams:\n%s" % (len(failed), n, "\n".join(failed[:60]))
