"""The relatedness estimates without a device (include/hpgv.h "IBS"): the new symbols are exported, hpgv_ibs_terms and
hpgv_ibs_genome are the header's expressions bit for bit with the same NaN pattern, E agrees with exact rational arithmetic, and
the identities a duplicate sample and an empty pair must show."""
from fractions import Fraction

import numpy as np
import pytest

import ibs_golden as ig
from helpers import hpgv, random_codes


@pytest.fixture(scope="module", autouse=True)
def built():
    hpgv.build()


@pytest.fixture(scope="module")
def case():
    """300 rows x 40 columns with one all-missing row, one monomorphic row, and rows with so few calls that T falls below 4"""
    rng = np.random.default_rng(77)
    codes = random_codes(rng, 300, 40, quirks=True, strict=False)
    codes[5] = 0xFF
    codes[6] = 0x00
    codes[7] = 0xFF
    codes[7, 3] = 0x01                                           # one call: T = 2
    codes[8] = 0xFF
    codes[8, 2:4] = (0x00, 0x11)                                 # two calls: T = 4, the first used size
    c4 = ig.class_counts(codes)
    return codes, c4, ig.pair_counts(codes)


def test_symbols_are_exported():
    L = hpgv.load()
    for name in ("hpgv_ibs_pairs_dev", "hpgv_ibs_class_counts_dev", "hpgv_ibs_select_dev", "hpgv_ibs", "hpgv_ibs_text", "hpgv_ibs_terms", "hpgv_ibs_genome"):
        assert name in hpgv.SYMBOLS and hasattr(L, name)
    assert hpgv.IBS_COUNTS.itemsize == 16 and hpgv.IBS_PAIR.itemsize == 32 and hpgv.IBS_PAIR.fields["pi_hat"][1] == 24


def test_terms_are_the_expressions_bit_for_bit(case):
    _, c4, _ = case
    used, terms = hpgv.ibs_terms(c4)
    exp = [ig.terms(*r[:3]) for r in c4.tolist()]
    assert used.tolist() == [u for u, _ in exp]
    ig.same_bits(terms, np.array([t for _, t in exp]), "terms")
    assert not used[5] and used[6] and not used[7] and used[8] and not terms[5].any() and not terms[7].any()


def test_the_edge_of_used_rows_is_t_equal_4():
    L = hpgv.load()
    t = np.full(5, 9.0)
    # T = X + Y = 2 (n0 + n1 + n2) is even for any class counts: T = 3 cannot be given to the function, so the edge is T = 2 against
    # T = 4, the latter in every split of the two samples over the classes
    for n0, n1, n2, T in ((0, 0, 0, 0), (1, 0, 0, 2), (0, 1, 0, 2), (1, 1, 0, 4), (2, 0, 0, 4), (0, 0, 2, 4), (1, 0, 1, 4)):
        t[:] = 9.0
        used = L.hpgv_ibs_terms(n0, n1, n2, hpgv._ptr(t))
        assert used == (1 if T >= 4 else 0), (n0, n1, n2)
        exp_used, exp = ig.terms(n0, n1, n2)
        assert exp_used == bool(used)
        ig.same_bits(t, exp, str((n0, n1, n2)))
        if not used:
            assert not t.any()
    # two samples, one of them heterozygous (X = 3, Y = 1): fall(1, 2) = 0 makes t00 zero, and t01 = 4 (3 2 1 1) / (4 3 2 1) + 0
    t[:] = 9.0
    assert L.hpgv_ibs_terms(1, 1, 0, hpgv._ptr(t)) == 1 and t[0] == 0.0 and t[1] == 4.0 * (6.0 / 24.0)
    # a negative count is no row
    assert L.hpgv_ibs_terms(-1, 5, 5, hpgv._ptr(t)) == 0 and not t.any()


def test_expected_values_against_rational_arithmetic(case):
    """Every term is a few roundings of a positive value: at most 2 products per falling factorial pair, one division, one scaling
    (exact, a power of two) and up to 3 additions of positive terms -- under 8 roundings, relative error < 8 u each, u = 2^-53.  The
    sum of m positive terms added sequentially has relative error <= (m - 1) u on top (Higham, sequential summation of same-signed
    terms), and the final division adds one: (m + 8) 2^-53 bounds the relative error of each E for m used rows."""
    _, c4, _ = case
    E, m = ig.expected(c4)
    got = hpgv.ibs_expected(c4)
    ig.same_bits(got, E, "E")
    exact = [Fraction(0)] * 5
    rows = 0
    for n0, n1, n2 in c4[:, :3].tolist():
        if 2 * (n0 + n1 + n2) >= 4:
            rows += 1
            exact = [a + b for a, b in zip(exact, ig.terms_exact(n0, n1, n2))]
    assert rows == m and m > 250
    bound = Fraction(m + 8, 2 ** 53)
    for k in range(5):
        ex = exact[k] / m
        rel = abs(Fraction(float(got[k])) - ex) / ex
        print("E[%d] = %.17g, relative error %.3g, bound %.3g" % (k, got[k], float(rel), float(bound)))
        assert rel <= bound, (k, float(rel))
    # the five expectations of one row sum to 1 over the IBD states: E00 + E01 + E02 = 1 and E11 + E12 = 1, up to the same bound
    assert abs(got[0] + got[1] + got[2] - 1.0) < 1e-12 and abs(got[3] + got[4] - 1.0) < 1e-12


def test_genome_is_the_expression_bit_for_bit(case):
    _, c4, counts = case
    E, _ = ig.expected(c4)
    iu = np.triu_indices(counts.shape[0], 1)
    recs = counts[iu].astype(np.int32)
    # and records that reach every clamp and renormalisation, n = 0, and a zero E
    extra = np.array([[100, 0, 0, 100], [100, 90, 10, 0], [100, 0, 100, 0], [100, 50, 0, 50], [100, 0, 1, 99], [0, 0, 0, 0], [7, 1, 2, 4],
                      [1000, 400, 500, 100]], np.int32)
    recs = np.concatenate([recs, extra])
    got = hpgv.ibs_genome(recs, E)
    exp = ig.genome_all(recs, E)
    ig.same_bits(got, exp, "genome")
    assert np.isnan(got[len(recs) - 3]).all()                    # n = 0: every value 0 / 0
    # each branch was taken by some record
    raw = []
    for n, i0, i1, i2 in recs.tolist():
        if n:
            S = float(n)
            z0 = i0 / (E[0] * S)
            z1 = (i1 - z0 * (E[1] * S)) / (E[3] * S)
            z2 = (i2 - z0 * (E[2] * S) - z1 * (E[4] * S)) / S
            raw.append((z0, z1, z2))
    raw = np.array(raw)
    assert (raw[:, 0] > 1).any() and (raw[:, 1] > 1).any() and (raw[:, 1] < 0).any() and (raw[:, 2] < 0).any()
    # the structured array form gives the same
    st = np.zeros(len(recs), hpgv.IBS_COUNTS)
    st["n"], st["ibs0"], st["ibs1"], st["ibs2"] = recs.T
    ig.same_bits(hpgv.ibs_genome(st, E), exp, "genome, records")
    # a zero E gives inf or NaN, the same ones
    for zero in range(5):
        Ez = E.copy()
        Ez[zero] = 0.0
        ig.same_bits(hpgv.ibs_genome(recs[:50], Ez), ig.genome_all(recs[:50], Ez), "E[%d] = 0" % zero)
    Enan = np.full(5, np.nan)
    assert np.isnan(hpgv.ibs_genome(recs[:5], Enan)[:, :4]).all()


def test_a_copied_column_is_a_duplicate(case):
    codes, _, _ = case
    codes = codes.copy()
    rng = np.random.default_rng(3)
    codes[:, 11] = codes[:, 4]
    codes[rng.random(len(codes)) < 0.1, 11] = 0xFF               # the copy misses other genotypes than the original
    codes[rng.random(len(codes)) < 0.1, 4] = 0xFF
    c4 = ig.class_counts(codes)
    rec = ig.pair_counts(codes)[4, 11].astype(np.int32)
    assert rec[0] > 200 and rec[1] == 0 and rec[2] == 0 and rec[3] == rec[0]
    out = hpgv.ibs_genome(rec, hpgv.ibs_expected(c4))
    assert out[0] == 0.0 and out[1] == 0.0 and out[2] == 1.0 and out[3] == 1.0 and out[4] == 1.0


def test_no_common_row_gives_nan(case):
    _, c4, _ = case
    out = hpgv.ibs_genome(np.zeros(4, np.int32), hpgv.ibs_expected(c4))
    assert np.isnan(out).all()


def test_the_golden_counts_against_a_direct_count():
    """the indicator products against a loop over the pairs of a small matrix, all 256 byte values among its rows"""
    rng = np.random.default_rng(12)
    codes = random_codes(rng, 40, 9, quirks=True, strict=False)
    codes[:29, 0] = np.arange(0, 256, 9, dtype=np.uint8)[:29]
    skip = np.zeros(40, np.uint8)
    skip[[0, 17]] = 1
    hi, lo = codes >> 4, codes & 15
    g = np.where((hi == 15) | (lo == 15), -1, (hi != 0).astype(int) + (lo != 0))
    for sk in (None, skip):
        got = ig.pair_counts(codes, sk)
        for i in range(9):
            for j in range(9):
                rows = [k for k in range(40) if g[k, i] >= 0 and g[k, j] >= 0 and (sk is None or not sk[k])]
                d = [abs(g[k, i] - g[k, j]) for k in rows]
                exp = [len(rows), d.count(2), d.count(1), d.count(0)] if i < j else [0, 0, 0, 0]
                assert got[i, j].tolist() == exp
