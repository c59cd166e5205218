"""The corpus of hand-assembled DEFLATE streams that both inflate decoders are held to: legal constructs that zlib's encoder never
emits, by class, and one stream per irregularity.  Built once per process (`corpus()`), from deflate_builder alone; zlib's inflate
is the arbiter of every stream (tests/test_deflate_streams_cpu.py pins the corpus to it).

Classes that must be taken, classes that may be refused and the illegal ones are told apart by `kind`, after the two lists below.
tests/test_gpu_inflate_streams.py states the may-refuse list once more, in the open, and asserts that it is this one."""
import functools
import random
from collections import namedtuple

from deflate_builder import Stream, balanced_lengths, litlen_symbols, plain_code_length_symbols, run_length_code_lengths

MUST, MAY, ILLEGAL = "must-take", "may-refuse", "illegal"
MUST_TAKE_CLASSES = ["full_distance", "ring_seam", "period", "pending", "writers", "cl_runs", "one_distance_code", "long_codes",
                     "spelling_284_31", "many_blocks", "alignment"]
# Legal streams (zlib takes them) that a decoder here may hand to the slower path: a dynamic block without any distance code,
# and one whose literal / length code is the end-of-block code alone, one bit long.  Nothing else may be refused.
MAY_REFUSE_CLASSES = ["no_distance_code", "single_litlen_code_length_1"]
MAX_TEXT = 65280                                      # what a BGZF block holds at most

# name: "<class>/<what>"; text: what the stream stands for (None: illegal); out_len: the text size the decoder is told;
# align: the residue mod 4 of the stream's first byte in the buffer that the case asks for (None: any); meta: class-specific notes
Case = namedtuple("Case", "name cls kind comp text out_len align meta")


def _rand(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


def _case(name, s, kind=MUST, out_len=None, align=None, meta=None, comp=None):
    cls = name.split("/")[0]
    text = None if kind == ILLEGAL else bytes(s.text)
    n = len(s.text) if out_len is None else out_len
    assert n <= MAX_TEXT, name
    meta = dict(meta or {}, runs_across_the_tables=s.runs_across_the_tables)
    return Case(name, cls, kind, s.getvalue() if comp is None else comp, text, n, align, meta)


def _full_distance(rng):
    toks = [(n, d) for d in (32768, 32767, 32507, 24577, 16385) for n in (3, 64, 65, 258)]
    out = []
    for code in ("fixed", "dynamic", "fixed_then_dynamic"):
        s = Stream().stored(_rand(rng, 32768))
        if code == "fixed":
            s.fixed(toks, final=True)
        elif code == "dynamic":
            s.auto_dynamic(toks, final=True)          # its two distance symbols are 28 and 29: 13 extra bits each
        else:
            s.fixed(toks).auto_dynamic(toks[::-1], final=True)
        out.append(_case("full_distance/" + code, s))
    return out


def _ring_seam(rng):
    out = []
    for d in (4094, 4095, 4096, 4097, 4098):
        for cross in (True, False):
            s = Stream().stored(_rand(rng, d + 37))
            for i, n in enumerate((3, 63, 64, 65, 128, 129, 257, 258)):
                # the first source byte's place in a ring of 4 096 bytes: the source's middle on the wrap, or far from it
                want = 4096 - (n + 1) // 2 if cross else 100
                s.stored(_rand(rng, (want + d - len(s.text)) % 4096))
                assert (len(s.text) - d) % 4096 == want
                (s.fixed if i % 2 == 0 else s.auto_dynamic)([(n, d)])
            s.stored(b"", final=True)
            out.append(_case("ring_seam/d%d_%s" % (d, "across_the_wrap" if cross else "inside"), s))
    return out


PERIOD_DISTANCES = list(range(1, 71)) + [127, 128, 129, 255, 256, 257, 258, 259]


def _period(rng):
    out = []
    for d in PERIOD_DISTANCES:
        lens = list(range(3, 259))
        rng.shuffle(lens)
        toks = list(_rand(rng, d)) + [(n, d) for n in lens]
        out.append(_case("period/fixed_d%d" % d, Stream().fixed(toks, final=True)))
        out.append(_case("period/dynamic_d%d" % d, Stream().auto_dynamic(toks, final=True)))
    return out


def _pending(rng):
    # match A, then match B whose source is (part of) what A wrote; "easy" is what the wave decoder's quick path takes: from
    # the ring, 64 bytes at most, not overlapping itself
    a_kinds = [("easy", (40, 200)), ("long", (150, 300)), ("overlapping", (100, 7)), ("far", (90, 5000))]

    def b_kinds(la):
        return [("inside_the_tail", (20, 30)), ("partly_in_the_tail", (50, 90)), ("the_head", (30, la)), ("up_to_the_end", (16, 16)),
                ("up_to_the_end_overlapping", (17, 16)), ("the_last_byte", (64, 1)), ("the_tail_repeated", (200, 64)),
                ("long_from_a", (130, max(la, 130)))]
    out = []
    for sep in ("nothing", "literal", "stored", "block"):
        s = Stream().stored(_rand(rng, 6000))
        k, pairs = 0, []
        for an, a in a_kinds:
            for bn, b in b_kinds(a[0]):
                lead = list(_rand(rng, 5))
                huff = s.fixed if k % 2 == 0 else s.auto_dynamic
                k += 1
                if sep == "nothing":
                    huff(lead + [a, b])
                elif sep == "literal":
                    huff(lead + [a, 0x41 + k % 26, (b[0], b[1] + 1)])
                elif sep == "stored":
                    huff(lead + [a])
                    s.stored(_rand(rng, 3))
                    huff([(b[0], b[1] + 3)] + lead)
                else:
                    huff(lead + [a])
                    s.auto_dynamic([b] + lead)
                pairs.append(an + "+" + bn)
        s.stored(b"", final=True)
        out.append(_case("pending/%s_between" % sep, s, meta={"pairs": pairs}))
    return out


def _writers(rng):
    # 300 bytes by each of the four writers, read back at once by a near match (out of the ring) and, 4 200 bytes later,
    # by a far match (out of global memory)
    out = []
    for merged in (False, True):
        s = Stream().stored(_rand(rng, 5000))
        held = []

        def flush():
            if held:
                (s.fixed if len(s.block_ends) % 2 else s.auto_dynamic)(list(held))
                del held[:]

        def huff(toks):
            held.extend(toks)
            if not merged:
                flush()

        def stored(data):
            flush()
            s.stored(data)
        writers = [("literals", lambda: huff(list(_rand(rng, 300)))), ("stored", lambda: stored(_rand(rng, 300))),
                   ("far_match", lambda: huff([(258, 4500), (42, 4500)])), ("near_match", lambda: huff([(258, 37), (42, 1000)]))]
        for _, write in writers:
            write()
            huff([(100, 100)])                                        # near reader
            write()
            stored(_rand(rng, 4200))
            huff([(100, 4300)])                                       # far reader
        flush()
        s.stored(b"", final=True)
        out.append(_case("writers/" + ("one_block_where_possible" if merged else "a_block_each"), s))
    return out


def _ab_lengths(size=258):
    """'a', 'b', end of block and length 3: two bits each"""
    ll = [0] * size
    for sym in (97, 98, 256, 257):
        ll[sym] = 2
    return ll


def _cl_lengths(cls, more=()):
    used = sorted({s for s, _ in cls} | set(more))
    if len(used) < 2:
        used.append(0 if used[0] else 1)
    return balanced_lengths(used, 19)


def _dyn(s, toks, ll, dd, cls, final=True, hclen=None, more=()):
    assert sum({16: 3 + x, 17: 3 + x, 18: 11 + x}.get(c, 1) for c, x in cls) == len(ll) + len(dd)
    return s.dynamic(toks, ll, dd, cls, _cl_lengths(cls, more), final, hclen=hclen)


def _cl_runs(rng):
    out = []
    # a 17-run over the last two literal / length zeros and the first four distance zeros
    ll = _ab_lengths(260)
    s = Stream().fixed(list(b"17: "))
    _dyn(s, [97, 98, 97, 98, 97, 98, (3, 5), (3, 7)], ll, [0, 0, 0, 0, 1, 1], run_length_code_lengths(ll[:258]) + [(17, 3), (1, 0), (1, 0)])
    out.append(_case("cl_runs/17_across_the_tables", s))
    # an 18-run over eight literal / length zeros and five distance zeros
    ll = _ab_lengths(266)
    s = Stream().fixed(list(b"18: "))
    _dyn(s, [97, 98] * 5 + [(3, 7), (3, 9), (3, 12)], ll, [0] * 5 + [1, 1], run_length_code_lengths(ll[:258]) + [(18, 2), (1, 0), (1, 0)])
    out.append(_case("cl_runs/18_across_the_tables", s))
    # a 16-repeat of the last literal / length length gives the four distance lengths
    ll = _ab_lengths(258)
    s = Stream().fixed(list(b"16: "))
    _dyn(s, [97, 98, 97, 98, (3, 1), (3, 2), (3, 3), (3, 4)], ll, [2, 2, 2, 2], run_length_code_lengths(ll) + [(16, 1)])
    out.append(_case("cl_runs/16_repeats_the_last_litlen_length", s))
    # ... of a length that is not the first table's last but one: 259 has two bits, the four distance lengths repeat it
    ll = [0] * 260
    ll[97] = ll[98] = ll[257] = ll[258] = 3
    ll[256] = ll[259] = 2
    s = Stream().fixed(list(b"16+: "))
    _dyn(s, [97, 98, (3, 1), (4, 2), (5, 3), (5, 4), 98], ll, [2, 2, 2, 2], run_length_code_lengths(ll) + [(16, 1)])
    out.append(_case("cl_runs/16_repeats_the_length_of_symbol_259", s))
    # a 16-repeat that begins in the first table and ends in the second: 258, 259 and the first four distance lengths
    ll = [0] * 260
    ll[97] = ll[98] = 2
    ll[256] = ll[257] = ll[258] = ll[259] = 3
    s = Stream().fixed(list(b"16 across: "))
    _dyn(s, [97, 98, (3, 1), (4, 2), (5, 5), (5, 8), (3, 16)], ll, [3] * 8, run_length_code_lengths(ll[:258]) + [(16, 3), (16, 1)])
    out.append(_case("cl_runs/16_across_the_tables", s))
    # a 16-repeat directly after an 18-run: it repeats the zero
    s = Stream().fixed(list(b"18 16: "))
    cls = [(18, 83), (16, 0), (2, 0), (2, 0), (18, 127), (18, 8), (2, 0), (2, 0), (1, 0), (1, 0)]
    _dyn(s, [97, 98, 98, 97, (3, 1), (3, 2)], _ab_lengths(258), [1, 1], cls)
    out.append(_case("cl_runs/16_after_18", s))
    # HLIT = 257: no length symbol, so no match; HDIST = 1 with the one code unused; HCLEN = 18 (length 1 is the 18th)
    ll = [0] * 257
    ll[97], ll[98], ll[256] = 1, 2, 2
    s = Stream().fixed(list(b"hlit 257: "))
    _dyn(s, [97, 98, 97, 97, 98], ll, [1], run_length_code_lengths(ll) + [(1, 0)])
    out.append(_case("cl_runs/hlit_257_hdist_1", s))
    # HLIT = 286, HDIST = 30: every symbol has a code; lengths 8 / 9 and 4 / 5 make HCLEN = 12, the smallest count with which a
    # block can hold a match under a complete distance code (HCLEN = 4 allows no length but 0: see the illegal list)
    ll, dd = balanced_lengths(range(286), 286), balanced_lengths(range(30), 30)
    toks = list(_rand(rng, 700)) + [(3, 1), (258, 2), (257, 700), (10, 3), (11, 4), (130, 513), (19, 600)] + list(range(256))
    s = Stream().stored(_rand(rng, 25000))
    toks += [(n, d) for n, d in zip((4, 5, 6, 7, 8, 9, 12, 14, 16, 18, 22, 26, 30, 34, 42, 50, 58, 66, 82, 98, 114, 162, 194, 226, 258, 3, 3, 3, 3, 3),
                                    (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 6144,
                                     8192, 12288, 16384, 24576, 25000))]
    cls = plain_code_length_symbols(ll + dd)
    s.dynamic(toks, ll, dd, cls, _cl_lengths(cls), final=True)
    out.append(_case("cl_runs/hlit_286_hdist_30_hclen_12", s))
    s = Stream().stored(_rand(rng, 25000))
    s.dynamic(toks, ll, dd, cls, _cl_lengths(cls), final=True, hclen=19)
    out.append(_case("cl_runs/hlit_286_hdist_30_hclen_19", s))
    return out


def _one_distance_code(rng):
    out = []
    lead = [32 + b % 64 for b in _rand(rng, 60)]
    for name, dd, dists in (("symbol_10_alone", [0] * 10 + [1], range(33, 49)), ("symbol_0_alone", [1], [1]),
                            ("two_of_one_bit_the_second_used", [1, 1], [2])):
        toks = list(lead)
        for i in range(40):
            toks += [((3, 4, 6, 10, 16, 35, 60, 131, 258)[i % 9], list(dists)[i % len(dists)]), lead[i]]
        ll = balanced_lengths(sorted(litlen_symbols(toks)[0] | {256}), 286)
        s = Stream().fixed(list(b"one distance code: "))
        cls = run_length_code_lengths(ll) + plain_code_length_symbols(dd)
        s.dynamic(toks, ll, dd, cls, _cl_lengths(cls), final=True)
        out.append(_case("one_distance_code/" + name, s))
    return out


LONG_LL = [97, 98, 99, 100, 101, 102, 103, 104, 105, 256, 257, 258, 265, 270, 284, 285]
LONG_DD = [0, 1, 2, 3, 4, 5, 8, 10, 14, 16, 20, 22, 24, 26, 28, 29]
_SKEW = list(range(1, 16)) + [15]


def _long_codes(rng):
    from deflate_builder import DIST_BASE
    out = []
    lens_of = {257: 3, 258: 4, 265: 12, 270: 24, 284: 250, 285: 258}
    plans = [("rotation_%d" % k, [(i + k) % 16 for i in range(16)], [(i + 5 * k) % 16 for i in range(16)], LONG_DD) for k in range(16)]
    # every length symbol and the end of block past the 8-bit root, and every distance symbol that is used too
    plans.append(("length_then_distance_past_the_root", list(range(16)), list(range(16)), LONG_DD[8:]))
    for name, lrot, drot, dused in plans:
        ll, dd = [0] * 286, [0] * 30
        for i, sym in enumerate(LONG_LL):
            ll[sym] = _SKEW[lrot[i]]
        for i, sym in enumerate(LONG_DD):
            dd[sym] = _SKEW[drot[i]]
        toks = [97 + b % 9 for b in _rand(rng, 40)]
        for i in range(7 * 16):
            n = lens_of[(257, 258, 265, 270, 284, 285)[i % 6]]
            d = DIST_BASE[dused[i % len(dused)]]
            toks += [(n, d + (i % 2 if d > 4 else 0)), 97 + i % 9]
        s = Stream().stored(_rand(rng, 25000))
        cls = plain_code_length_symbols(ll + dd)
        s.dynamic(toks, ll, dd, cls, _cl_lengths(cls), final=True)
        out.append(_case("long_codes/" + name, s))
    return out


def _spelling(rng):
    toks = list(b"spelled: ") + [(258, 1), (258, 258), 65, (258, 300), (258, 257), (258, 5000), 66, (258, 4096), (258, 4097), (100, 3)]
    return [_case("spelling_284_31/fixed", Stream().stored(_rand(rng, 5000)).fixed(toks, final=True, spell_258_as_284=True)),
            _case("spelling_284_31/dynamic", Stream().stored(_rand(rng, 5000)).auto_dynamic(toks, final=True, spell_258_as_284=True)),
            _case("spelling_284_31/both_spellings", Stream().stored(_rand(rng, 5000)).fixed(toks, spell_258_as_284=True).fixed(toks, final=True))]


def _many_blocks(rng):
    out = []
    for j in range(8):
        s = Stream()
        empty = 0
        for b in range(199):
            kind = b % 3
            if kind == 0:
                s.stored(_rand(rng, rng.choice([0, 0, 1, 7, 300])))
                continue
            toks = []
            if rng.random() >= 0.25:
                if len(s.text) >= 10:                                   # the first match reaches into the blocks before
                    toks.append((rng.randint(3, 40), rng.randint(1, min(len(s.text), 5000))))
                toks += list(_rand(rng, rng.randint(0, 40)))
            empty += not toks
            (s.fixed if kind == 1 else s.auto_dynamic)(toks)
        s.fixed([144 + b % 100 for b in _rand(rng, j)], final=True)   # j nine-bit literals: every count of pad bits in turn
        out.append(_case("many_blocks/%d" % j, s, meta={"block_ends": list(s.block_ends), "pad_bits": s.pad_bits, "empty": empty}))
    return out


def _may_refuse(rng):
    out = []
    ll = [0] * 257
    ll[97], ll[98], ll[256] = 1, 2, 2
    s = Stream().fixed(list(b"no distance code: "))
    _dyn(s, [97, 98, 98, 97, 97], ll, [0], run_length_code_lengths(ll) + [(0, 0)])
    out.append(_case("no_distance_code/hdist_1_length_0", s, MAY))
    # HCLEN = 5: the only lengths are 0 and 8, so 256 literal / length codes of eight bits and no distance code
    ll = [8] * 255 + [0, 8]
    toks = list(_rand(rng, 500).replace(b"\xff", b"\x00"))
    s = Stream().fixed(list(b"hclen 5: "))
    cls = plain_code_length_symbols(ll + [0])
    cl = [0] * 19
    cl[0] = cl[8] = 1
    s.dynamic(toks, ll, [0], cls, cl, final=True)
    out.append(_case("no_distance_code/hclen_5", s, MAY))
    only_eob = [0] * 256 + [1]
    s = Stream().fixed(list(b"an empty block: "))
    _dyn(s, [], only_eob, [1, 1], run_length_code_lengths(only_eob) + [(1, 0), (1, 0)], final=False)
    s.fixed(list(b"and text behind it"), final=True)
    out.append(_case("single_litlen_code_length_1/mid_stream", s, MAY))
    s = Stream().stored(b"abc")
    _dyn(s, [], only_eob, [1, 1], run_length_code_lengths(only_eob) + [(1, 0), (1, 0)])
    out.append(_case("single_litlen_code_length_1/last_block", s, MAY))
    s = Stream()
    _dyn(s, [], only_eob, [1, 1], run_length_code_lengths(only_eob) + [(1, 0), (1, 0)])
    out.append(_case("single_litlen_code_length_1/empty_text", s, MAY))
    return out


def _illegal(rng):
    out = []

    def start():
        return Stream().fixed(list(b"hello"))

    def add(name, s, out_len, comp=None):
        out.append(_case("illegal/" + name, s, ILLEGAL, out_len=out_len, comp=comp))
    ab = _ab_lengths(258)
    ab_cls = run_length_code_lengths(ab)
    good_dd = plain_code_length_symbols([1, 1])
    toks = [97, 98, 98, 97, (3, 2)]

    add("block_type_3", start().bits(1, 1).bits(3, 2), 5)
    add("stored_len_nlen_mismatch", start().stored(b"abcdef", final=True, nlen=0x1234), 11)
    add("stored_length_past_the_input", start().stored(b"x" * 50, final=True, length=100), 105)
    add("stored_length_past_the_text", start().stored(_rand(rng, 100), final=True), 65)
    for hlit in (287, 288):
        s = start().open_dynamic(ab, [1, 1], ab_cls + good_dd, _cl_lengths(ab_cls + good_dd), True, hlit=hlit)
        add("hlit_%d" % hlit, s.tokens(toks).close(), 12)
    for hdist in (31, 32):
        s = start().open_dynamic(ab, [1, 1], ab_cls + good_dd, _cl_lengths(ab_cls + good_dd), True, hdist=hdist)
        add("hdist_%d" % hdist, s.tokens(toks).close(), 12)
    # the code-length code: symbols 0, 1, 2 and 18 are what the header of `ab` needs
    cl = [0] * 19
    cl[0] = cl[1] = cl[2] = cl[18] = 1
    add("code_length_code_over_subscribed", start().open_dynamic(ab, [1, 1], ab_cls + good_dd, cl, True).tokens(toks).close(), 12)
    cl = [0] * 19
    cl[0], cl[1], cl[2], cl[18] = 2, 2, 2, 3
    add("code_length_code_incomplete", start().open_dynamic(ab, [1, 1], ab_cls + good_dd, cl, True).tokens(toks).close(), 12)
    cls = [(16, 0)] + run_length_code_lengths(ab[3:]) + good_dd
    add("16_as_the_first_symbol", start().open_dynamic(ab, [1, 1], cls, _cl_lengths(cls), True).tokens(toks).close(), 12)
    # a run that ends behind the last of the HLIT + HDIST lengths.  A decoder that does not look would find the two distance lengths
    # 1 and 0 -- a lone code of one bit, which is legal -- so the block's match uses that code and the text is the size such a
    # decoder arrives at: only the look at the run's end refuses these two
    over = [97, 98, 98, 97, (3, 1)]
    cls = ab_cls + [(1, 0), (17, 0)]
    add("run_past_the_last_length", start().open_dynamic(ab, [1, 0], cls, _cl_lengths(cls), True).tokens(over).close(), 12)
    cls = ab_cls + [(1, 0), (18, 100)]
    add("long_run_past_the_last_length", start().open_dynamic(ab, [1, 0], cls, _cl_lengths(cls), True).tokens(over).close(), 12)
    ll = [0] * 258
    ll[97], ll[98], ll[99] = 1, 2, 2
    cls = run_length_code_lengths(ll) + good_dd
    add("no_code_for_256", start().open_dynamic(ll, [1, 1], cls, _cl_lengths(cls), True).tokens([97, 98, 99]), 8)
    # HCLEN = 4 gives lengths to 16, 17, 18 and 0 only: every code length is 0, so there is no end-of-block code.  (The smallest
    # HCLEN of a legal block is 5, without a distance code -- no_distance_code/hclen_5 -- and 12 with one: cl_runs.)
    cl = [0] * 19
    cl[0] = cl[18] = 1
    s = start().open_dynamic([0] * 257, [0], [(18, 127), (18, 109)], cl, True, hclen=4)
    add("hclen_4_leaves_no_code_for_256", s, 5)
    ll = [0] * 258
    ll[97] = ll[98] = ll[256] = 1
    cls = run_length_code_lengths(ll) + good_dd
    add("litlen_code_over_subscribed", start().open_dynamic(ll, [1, 1], cls, _cl_lengths(cls), True).tokens([97, 98]).close(), 7)
    ll = [0] * 258
    ll[97] = ll[256] = 2
    cls = run_length_code_lengths(ll) + good_dd
    add("litlen_code_incomplete_two_symbols", start().open_dynamic(ll, [1, 1], cls, _cl_lengths(cls), True).tokens([97, 97]).close(), 7)
    ll = [0] * 256 + [2]
    for n in (2, 3, 9):
        ll[256] = n
        cls = run_length_code_lengths(ll) + good_dd
        add("single_litlen_code_of_length_%d" % n, start().open_dynamic(ll, [1, 1], cls, _cl_lengths(cls), True).close(), 5)
    for name, dd in (("distance_code_over_subscribed", [1, 1, 1]), ("distance_code_incomplete_two_symbols", [2, 2]),
                     ("single_distance_code_of_length_2", [0, 2]), ("single_distance_code_of_length_9", [0, 9])):
        cls = ab_cls + plain_code_length_symbols(dd)
        add(name, start().open_dynamic(ab, dd, cls, _cl_lengths(cls), True).tokens(toks).close(), 12)
    cls = ab_cls + [(1, 0)]
    s = start().open_dynamic(ab, [1], cls, _cl_lengths(cls), True).tokens([97, 98, (3, 1)]).litlen(257).bits(1, 1).close()
    add("unused_code_of_a_one_symbol_distance_code", s, 13)
    for sym in (286, 287):
        add("fixed_litlen_symbol_%d" % sym, start().open_fixed(True).tokens([97, 98]).litlen(sym).close(), 7)
        add("fixed_litlen_symbol_%d_and_a_distance" % sym, start().open_fixed(True).tokens([97, 98]).litlen(sym).dist(0).close(), 10)
    for sym in (30, 31):
        add("fixed_distance_symbol_%d" % sym, start().open_fixed(True).tokens([97, 98]).litlen(257).dist(sym).close(), 10)
    add("distance_past_the_start_of_an_empty_text", Stream().open_fixed(True).tokens([(3, 1)], follow=False).close(), 3)
    add("distance_past_the_start_of_a_short_text", Stream().open_fixed(True).tokens([97, (3, 2)], follow=False).close(), 4)
    s = Stream().stored(_rand(rng, 5000)).open_fixed(True).tokens([(3, 5001)], follow=False).close()
    add("distance_past_the_start_beyond_the_ring", s, 5003)
    s = Stream().stored(_rand(rng, 5000)).open_fixed(True).tokens([(70, 4000), (200, 5071)], follow=False).close()
    add("long_distance_past_the_start_beyond_the_ring", s, 5270)
    for tail, name in (([97, 98, 99], "literal"), ([(40, 3)], "match"), ([(200, 3)], "long_match")):
        s = Stream().fixed(list(b"the text's size: ") + tail, final=True)
        add("text_one_byte_longer_ending_in_a_" + name, s, len(s.text) - 1)
        add("text_one_byte_shorter_ending_in_a_" + name, s, len(s.text) + 1)
    s = Stream().stored(_rand(rng, 300), final=True)
    add("stored_text_one_byte_shorter", s, 301)
    s = Stream().fixed(list(b"cut off inside its last codes!!"), final=True)
    for cut in (1, 2):
        add("last_code_runs_past_the_last_byte_%d" % cut, s, len(s.text), comp=s.getvalue()[:-cut])
    s = Stream().auto_dynamic(list(b"cut off inside a dynamic block's header"), final=True)
    add("header_runs_past_the_last_byte", s, len(s.text), comp=s.getvalue()[:12])
    return out


ALIGNED = ["full_distance/fixed", "full_distance/dynamic", "ring_seam/d4096_across_the_wrap", "period/fixed_d3", "period/dynamic_d64",
           "cl_runs/18_across_the_tables", "long_codes/rotation_3", "many_blocks/3", "one_distance_code/symbol_0_alone"]


@functools.lru_cache(maxsize=None)
def corpus():
    """every case, legal and illegal ones interleaved; the last one is an `alignment` case (the last stream of a buffer)"""
    rng = random.Random(1951)
    legal = []
    for build in (_full_distance, _ring_seam, _period, _pending, _writers, _cl_runs, _one_distance_code, _long_codes, _spelling,
                  _many_blocks, _may_refuse):
        legal += build(rng)
    by_name = {c.name: c for c in legal}
    for name in ALIGNED:
        for a in range(4):
            legal.append(by_name[name]._replace(name="alignment/%d_%s" % (a, name), cls="alignment", align=a))
    bad = _illegal(rng)
    out, step = [], max(1, len(legal) // (len(bad) + 1))
    for i, c in enumerate(legal):
        out.append(c)
        if i % step == step - 1 and bad:
            out.append(bad.pop(0))
    out += bad
    out.append(by_name["many_blocks/5"]._replace(name="alignment/last_many_blocks/5", cls="alignment", align=1))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    assert {c.cls for c in out if c.kind == MUST} == set(MUST_TAKE_CLASSES)
    assert {c.cls for c in out if c.kind == MAY} == set(MAY_REFUSE_CLASSES)
    return tuple(out)


def layout(cases, gap=64, seed=7):
    """the cases' streams in one buffer (every first byte at the residue mod 4 its case asks for, or at its index's; filler bytes
    between the streams; four bytes behind the last, which the wave decoder's contract wants readable) and their texts with `gap`
    bytes in front of the first, between them and behind the last: (buffer, in_off, in_len, out_off, out_len, size of the text buffer)"""
    rng = random.Random(seed)
    buf, in_off, out_off, pos = bytearray(), [], [], gap
    for i, c in enumerate(cases):
        want = i % 4 if c.align is None else c.align
        buf += _rand(rng, (want - len(buf)) % 4)
        in_off.append(len(buf))
        buf += c.comp
        out_off.append(pos)
        pos += c.out_len + gap
    buf += b"\xff" * 4
    return bytes(buf), in_off, [len(c.comp) for c in cases], out_off, [c.out_len for c in cases], pos


def zlib_takes(comp, out_len):
    """what zlib's inflate makes of a raw stream told to be `out_len` bytes of text: the text when the stream is valid, complete,
    has nothing behind it and is of that size; None otherwise.  zlib is the arbiter of what a valid stream is."""
    import zlib
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(comp)
    except zlib.error:
        return None
    if not d.eof or d.unused_data or len(text) != out_len:
        return None
    return text
