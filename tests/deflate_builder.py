"""A DEFLATE stream assembler written from RFC 1951: test infrastructure for the two inflate decoders.

zlib's encoder emits only a corner of the format.  Here a test says, symbol by symbol, what a stream holds -- which block
types, which code lengths, how the code lengths are run-length coded, which (length, distance) pairs -- and gets the bytes
and the text they stand for.  Nothing here decodes: `expected` replays tokens, it never reads a bit.

A token is a literal byte (an int) or a match `(length, distance)`.
"""

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32                                  # 30 and 31 have codes (and no meaning)


class BitWriter:
    """bits go out least significant first, bytes in order (RFC 1951, 3.1.1)"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 256:
            self._flush()

    def _flush(self):
        k = self.n >> 3
        self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
        self.acc >>= 8 * k
        self.n -= 8 * k

    @property
    def bitpos(self):
        return len(self.out) * 8 + self.n

    def align(self):
        self.bits(0, -self.n & 7)

    def raw(self, data):
        assert self.n & 7 == 0
        self._flush()
        self.out += data

    def getvalue(self):
        """the bytes so far, the last one padded with zero bits"""
        self._flush()
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lengths):
    """{symbol: (code as it goes into the bit writer, length)} of the canonical code with these lengths (RFC 1951, 3.2.2).
    Huffman codes are packed starting from their most significant bit, so the code is stored bit-reversed.  Lengths that
    are no prefix code (over-subscribed) still get the numbers the RFC's procedure gives, cut to their length."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            c = nxt[l] & ((1 << l) - 1)
            nxt[l] += 1
            out[s] = (int(format(c, "0%db" % l)[::-1], 2), l)
    return out


def kraft(lengths):
    """sum of 2^-l in units of 2^-15: 32768 for a complete code, more for an over-subscribed one"""
    return sum(1 << (15 - l) for l in lengths if l)


def length_symbol(n, spell_258_as_284=False):
    """(symbol - 257, extra bits' value) of match length n"""
    if n == 258 and spell_258_as_284:
        return 27, 31
    s = max(i for i in range(29) if LEN_BASE[i] <= n)
    return s, n - LEN_BASE[s]


def distance_symbol(d):
    s = max(i for i in range(30) if DIST_BASE[i] <= d)
    return s, d - DIST_BASE[s]


def balanced_lengths(symbols, size):
    """a complete code over `symbols` (two or more) whose lengths differ by one bit at most"""
    symbols = sorted(set(symbols))
    n = len(symbols)
    assert n >= 2
    k = (n - 1).bit_length()
    short = (1 << k) - n
    lens = [0] * size
    for i, s in enumerate(symbols):
        lens[s] = k - 1 if i < short else k
    return lens


def skewed_lengths(symbols, size):
    """a complete code over `symbols` in the order given: 1, 2, .. 7 bits for the first seven, the others balanced under
    the one 7-bit prefix that is left (so 9 bits and more from ten symbols on, 15 at most up to 263)"""
    symbols = list(symbols)
    n = len(symbols)
    assert n >= 2
    lens = [0] * size
    if n <= 8:
        for i, s in enumerate(symbols):
            lens[s] = min(i + 1, n - 1)
        return lens
    for i, s in enumerate(symbols[:7]):
        lens[s] = i + 1
    rest = symbols[7:]
    k = (len(rest) - 1).bit_length()
    short = (1 << k) - len(rest)
    for i, s in enumerate(rest):
        lens[s] = 7 + (k - 1 if i < short else k)
    return lens


def plain_code_length_symbols(lengths):
    return [(l, 0) for l in lengths]


def run_length_code_lengths(lengths):
    """the literal / length and distance lengths as ONE sequence, run-length coded greedily: a run does not care where the
    first table ends (RFC 1951, 3.2.7: "the code length repeat codes can cross from HLIT + 257 to the HDIST + 1 code lengths")"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v = lengths[i]
        j = i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            take = min(run, 138)
            out.append((18, take - 11) if take >= 11 else (17, take - 3))
            i += take
        elif v != 0 and run >= 4:
            out.append((v, 0))
            take = min(run - 1, 6)
            out.append((16, take - 3))
            i += 1 + take
        else:
            out.append((v, 0))
            i += 1
    return out


def replay(tokens, text):
    """append what the tokens stand for to the bytearray `text`"""
    for t in tokens:
        if isinstance(t, int):
            text.append(t)
            continue
        n, d = t[0], t[1]
        assert 1 <= d <= len(text), "a match from before the start of the text"
        if d >= n:
            text += text[len(text) - d:len(text) - d + n]
        else:
            unit = bytes(text[len(text) - d:])
            text += (unit * (n // d + 1))[:n]
    return text


def expected(tokens, before=b""):
    """the text of `tokens` behind the text `before`, in plain Python"""
    return bytes(replay(tokens, bytearray(before)))


class Stream:
    """One raw DEFLATE stream under construction.  `text` follows what the blocks written so far stand for (it stops being
    meaningful once an illegal construct went in through the raw escapes); `block_ends` holds the bit position behind
    every block."""

    def __init__(self):
        self.w = BitWriter()
        self.text = bytearray()
        self.block_ends = []
        self.runs_across_the_tables = 0                  # 16 / 17 / 18 runs that began in the first table and ended in the second
        self.ll = self.dd = None

    # ---- raw escapes
    def bits(self, value, n):
        self.w.bits(value, n)
        return self

    def litlen(self, symbol):
        """the open block's code of a literal / length symbol, nothing else"""
        self.w.bits(*self.ll[symbol])
        return self

    def dist(self, symbol):
        self.w.bits(*self.dd[symbol])
        return self

    # ---- blocks
    def stored(self, data, final=False, length=None, nlen=None):
        """a stored block; `length` / `nlen` override the two header fields"""
        data = bytes(data)
        n = len(data) if length is None else length
        self.w.bits(1 if final else 0, 1)
        self.w.bits(0, 2)
        self.w.align()
        self.w.bits(n, 16)
        self.w.bits((n ^ 0xFFFF) if nlen is None else nlen, 16)
        self.w.raw(data)
        self.text += data
        self.block_ends.append(self.w.bitpos)
        return self

    def open_fixed(self, final=False):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(1, 2)
        self.ll, self.dd = canonical(FIXED_LITLEN), canonical(FIXED_DIST)
        return self

    def open_dynamic(self, litlen_lengths, dist_lengths, code_length_symbols, code_length_lengths, final=False,
                     hlit=None, hdist=None, hclen=None):
        """a dynamic block's header.  `code_length_symbols` is the sequence of (symbol 0 .. 18, extra bits' value) that spells
        the HLIT + HDIST lengths -- given by the caller, so that runs may cross from the first table into the second, or be
        wrong; `hlit`, `hdist`, `hclen` override the counts the header states (the numbers of lengths, not the fields)"""
        self.w.bits(1 if final else 0, 1)
        self.w.bits(2, 2)
        self.w.bits((len(litlen_lengths) if hlit is None else hlit) - 257, 5)
        self.w.bits((len(dist_lengths) if hdist is None else hdist) - 1, 5)
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if code_length_lengths[s]])
        self.w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.w.bits(code_length_lengths[s], 3)
        cc = canonical(code_length_lengths)
        at, first = 0, len(litlen_lengths)
        for item in code_length_symbols:
            s, x = (item, 0) if isinstance(item, int) else item
            self.w.bits(*cc[s])
            if s >= 16:
                self.w.bits(x, CL_EXTRA[s])
            n = {16: 3 + x, 17: 3 + x, 18: 11 + x}.get(s, 1)
            self.runs_across_the_tables += at < first < at + n
            at += n
        self.ll, self.dd = canonical(litlen_lengths), canonical(dist_lengths)
        return self

    def tokens(self, tokens, spell_258_as_284=False, follow=True):
        w, ll, dd = self.w, self.ll, self.dd
        for t in tokens:
            if isinstance(t, int):
                w.bits(*ll[t])
                continue
            s, x = length_symbol(t[0], spell_258_as_284)
            w.bits(*ll[257 + s])
            w.bits(x, LEN_EXTRA[s])
            s, x = distance_symbol(t[1])
            w.bits(*dd[s])
            w.bits(x, DIST_EXTRA[s])
        if follow:
            replay(tokens, self.text)
        return self

    def close(self):
        """the end-of-block code"""
        self.w.bits(*self.ll[256])
        self.block_ends.append(self.w.bitpos)
        return self

    def fixed(self, tokens, final=False, spell_258_as_284=False):
        return self.open_fixed(final).tokens(tokens, spell_258_as_284).close()

    def dynamic(self, tokens, litlen_lengths, dist_lengths, code_length_symbols, code_length_lengths, final=False,
                spell_258_as_284=False, hclen=None):
        self.open_dynamic(litlen_lengths, dist_lengths, code_length_symbols, code_length_lengths, final, hclen=hclen)
        return self.tokens(tokens, spell_258_as_284).close()

    def auto_dynamic(self, tokens, final=False, spell_258_as_284=False, shape=balanced_lengths, runs=False, hlit=None):
        """a dynamic block whose codes are made for its tokens: every symbol used gets a code (`shape` says of which
        lengths), a code that would have one symbol only gets a second, unused one; the header spells every length out, or,
        with `runs`, run-length codes the two tables as one sequence; `hlit` states more literal / length lengths than the
        last symbol used needs (zeros, which then run on into the distance lengths)"""
        lits, dists = litlen_symbols(tokens, spell_258_as_284)
        ll, dd = sorted(lits | {256}), sorted(dists)
        if len(ll) < 2:
            ll = [0] + ll
        for extra in (0, 1):
            if len(dd) < 2 and extra not in dd:
                dd = sorted(dd + [extra])
        if shape is not balanced_lengths:                       # the rarest symbols first: they get the long codes last
            freq = symbol_counts(tokens, spell_258_as_284)
            ll.sort(key=lambda s: -freq[0].get(s, 0))
            dd.sort(key=lambda s: -freq[1].get(s, 0))
        ll_len, dd_len = shape(ll, max(257, max(ll) + 1, hlit or 0)), shape(dd, max(dd) + 1)
        cls = run_length_code_lengths(ll_len + dd_len) if runs else plain_code_length_symbols(ll_len + dd_len)
        used = sorted({s for s, _ in cls})
        if len(used) < 2:
            used.append(0 if used[0] != 0 else 1)
        cl_len = balanced_lengths(used, 19)
        return self.dynamic(tokens, ll_len, dd_len, cls, cl_len, final, spell_258_as_284)

    def getvalue(self):
        return self.w.getvalue()

    @property
    def pad_bits(self):
        return -self.w.bitpos & 7


def litlen_symbols(tokens, spell_258_as_284=False):
    """(literal / length symbols, distance symbols) that the tokens use"""
    lits, dists = set(), set()
    for t in tokens:
        if isinstance(t, int):
            lits.add(t)
        else:
            lits.add(257 + length_symbol(t[0], spell_258_as_284)[0])
            dists.add(distance_symbol(t[1])[0])
    return lits, dists


def symbol_counts(tokens, spell_258_as_284=False):
    a, b = {256: 1}, {}
    for t in tokens:
        if isinstance(t, int):
            a[t] = a.get(t, 0) + 1
        else:
            s = 257 + length_symbol(t[0], spell_258_as_284)[0]
            a[s] = a.get(s, 0) + 1
            d = distance_symbol(t[1])[0]
            b[d] = b.get(d, 0) + 1
    return a, b


def match_tokens(text, start, end, window=32768, min_dist=1):
    """tokens for text[start:end]: at every position the longest of a few match lengths that occurs `min_dist` .. `window`
    bytes back (the occurrence furthest back that bytes.find meets), a literal otherwise.  No encoder worth the name -- it only
    has to turn a text the caller chose into matches of many lengths and distances."""
    out, p = [], start
    while p < end:
        hit = None
        for n in (258, 131, 65, 64, 33, 12, 5, 3):
            if p + n > end:
                continue
            lo = max(0, p - window)
            at = text.find(text[p:p + n], lo, p - min_dist + n) if p - min_dist + n > lo else -1
            if at >= 0 and at <= p - min_dist:
                hit = (n, p - at)
                break
        if hit:
            out.append(hit)
            p += hit[0]
        else:
            out.append(text[p])
            p += 1
    return out
