"""CPU suite: the corpus of hand-assembled DEFLATE streams (tests/deflate_corpus.py) against zlib's inflate, which decides what
every stream is, and the host decoder (hpgv_host_inflate_raw, host/host_inflate.c) against the corpus -- in the stand-alone check
program, built with AddressSanitizer + UBSan and at the shipped optimisation level."""
import struct
import zlib

import pytest

import deflate_builder as db
import deflate_corpus as dc
from test_host_logic_cpu import _run, exe, exe_plain  # noqa: F401  (the two builds of tests/c/host_cpu_check.c)


@pytest.fixture(scope="module")
def cases():
    return dc.corpus()


def test_bit_writer_and_canonical_codes_follow_the_rfc():
    # RFC 1951, 3.2.2: lengths (3, 3, 3, 3, 3, 2, 4, 4) give the codes 010, 011, 100, 101, 110, 00, 1110, 1111
    codes = db.canonical([3, 3, 3, 3, 3, 2, 4, 4])
    want = ["010", "011", "100", "101", "110", "00", "1110", "1111"]
    assert [format(codes[s][0], "0%db" % codes[s][1])[::-1] for s in range(8)] == want
    w = db.BitWriter()
    w.bits(1, 1); w.bits(1, 2); w.bits(0b10110, 5); w.bits(0x1FF, 9)        # LSB first: 1, 10, 01101, then nine ones
    assert w.bitpos == 17 and w.getvalue() == bytes([0b10110011, 0xFF, 0x01])
    assert db.length_symbol(258) == (28, 0) and db.length_symbol(258, True) == (27, 31) and db.length_symbol(257) == (27, 30)
    assert db.distance_symbol(32768) == (29, 8191) and db.distance_symbol(24577) == (29, 0) and db.distance_symbol(1) == (0, 0)
    assert db.expected([97, 98, (5, 2), (3, 7)]) == b"abababaaba"
    assert db.kraft(db.balanced_lengths(range(286), 286)) == db.kraft(db.skewed_lengths(range(40), 40)) == 1 << 15
    lens = [0] * 20 + [5] * 9 + [0] * 150 + [3, 0, 0, 0, 7]
    spelled = db.run_length_code_lengths(lens)
    assert sum({16: 3 + x, 17: 3 + x, 18: 11 + x}.get(s, 1) for s, x in spelled) == len(lens) and len(spelled) < 12


def test_the_corpus_holds_what_it_is_meant_to(cases):
    names = [c.name for c in cases]
    assert 280 <= len(cases) <= 420 and max(c.out_len for c in cases) <= dc.MAX_TEXT
    for d in dc.PERIOD_DISTANCES:
        assert "period/fixed_d%d" % d in names and "period/dynamic_d%d" % d in names
    many = [c for c in cases if c.cls == "many_blocks"]
    assert sorted(c.meta["pad_bits"] for c in many) == list(range(8))         # the stream ends with 0 .. 7 pad bits
    for c in many:
        assert len(c.meta["block_ends"]) == 200 and c.meta["empty"] >= 10
        assert {e % 8 for e in c.meta["block_ends"]} == set(range(8))          # block ends at every bit position
    assert {c.align for c in cases if c.cls == "alignment"} == {0, 1, 2, 3} and cases[-1].cls == "alignment"
    across = [c.name for c in cases if c.cls == "cl_runs" and c.meta["runs_across_the_tables"] == 1]
    assert across == ["cl_runs/" + w for w in ("17_across_the_tables", "18_across_the_tables", "16_across_the_tables")]
    kinds = [c.kind for c in cases]
    assert kinds.count(dc.ILLEGAL) >= 40 and dc.ILLEGAL in kinds[:20]          # interleaved with the legal ones
    buf, in_off, in_len, out_off, out_len, total = dc.layout(cases)
    assert all(buf[o:o + n] == c.comp for o, n, c in zip(in_off, in_len, cases))
    assert all(o % 4 == c.align for o, c in zip(in_off, cases) if c.align is not None)
    assert len(buf) == in_off[-1] + in_len[-1] + 4


def test_zlib_decides_what_every_stream_is(cases):
    # legal: zlib's inflate gives exactly the text the builder's replay gives, ends there, and leaves nothing unused;
    # illegal: zlib raises, does not come to an end, or gives a text of another size
    for c in cases:
        if c.kind == dc.ILLEGAL:
            assert dc.zlib_takes(c.comp, c.out_len) is None, c.name
            continue
        d = zlib.decompressobj(-15)
        assert d.decompress(c.comp) == c.text and d.eof and not d.unused_data and not d.unconsumed_tail, c.name
        assert len(c.text) == c.out_len, c.name


@pytest.mark.parametrize("build", ["asan", "plain"])
def test_host_decoder_on_the_corpus(exe, exe_plain, tmp_path, cases, build):  # noqa: F811
    # every must-take stream decoded, bit for bit; a may-refuse one decoded or refused; nothing zlib does not take taken;
    # no byte written outside the text
    take = {dc.MUST: 1, dc.MAY: 2, dc.ILLEGAL: 0}
    with open(tmp_path / "streams.bin", "wb") as f:
        for c in cases:
            raw = c.text if c.text is not None else bytes(c.out_len)
            f.write(struct.pack("<IIB", len(c.comp), len(raw), take[c.kind]) + c.comp + raw)
    r = _run(exe if build == "asan" else exe_plain, "streams", str(tmp_path / "streams.bin"))
    failed = ["%s: %s" % (cases[int(l.split()[1])].name, " ".join(l.split()[2:])) for l in r.stdout.splitlines() if l.startswith("FAIL")]
    assert not failed, failed
    assert r.returncode == 0 and "streams ok: %d records" % len(cases) in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    refused = [cases[int(l.split()[1])].name for l in r.stdout.splitlines() if l.startswith("refused")]
    assert all(name.split("/")[0] in dc.MAY_REFUSE_CLASSES for name in refused), refused
    print("host decoder (%s) refused: %s" % (build, refused or "none"))
