"""The launch dimensions of the permutation kernels that the tests beside them leave unrun (k_assoc_perm in both forms,
csrc/hpgv_assoc_perm_kernels.h; k_tdt_perm and k_tdt_perm_slow, csrc/hpgv_tdt_perm_kernels.h; csrc/hpgv_perm_capi.hip):
passes past the first of the label kernel, the folded (tile, pass) grid of the TDT kernel past its first eight tiles, the signed
i8 operand at +-126, rows of 68 k-steps and more, the layout options that change the pitch and the chunk count the kernels
walk, the refusal at the permutation limit, and (section F) the host plumbing of the synchronous permutation and LD entry
points: a text call without a status array, calls without rows or lines, and a batch whose last row is no whole pitch.  The
case builders, device drivers and references are those of
test_assoc_perm_gpu.py, model_golden.py / test_assoc_trend_perm_gpu.py and test_tdt_perm_gpu.py, with further special label
and flip rows placed where later passes see them.

The label tests add a reference for n_ge that owes nothing to the engine: the exact bracket.  t_p >= t_obs is decided in
Python integers (the factors common to a variant's permutations cancel), G = strictly greater permutations, T = exact ties,
I = the ties whose two sums are the observed ones (identical inputs give identical bits, so these always count), and
G + I <= n_ge <= G + T.  The band T - I is where the engine's rounding decides; two conditions asserted on the reference
alone keep it from hiding a failure: no pair within a relative 1e-12 of the observed statistic that is not an exact tie
(the rounding error of either statistic function is a few 1e-16), and T - I at most 1 % of the compared pairs."""
import ctypes as C
import functools

import numpy as np
import pytest

import ld_golden as lg
import model_golden as mg
import test_assoc_perm_gpu as ap
import test_assoc_trend_perm_gpu as tp
import test_tdt_perm_gpu as td
from helpers import TOL, assert_close, assert_p_close, hpgv, random_codes, set_or_skip
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

PT = 128                                                 # PERM_PT: permutations per pass

# ((affected, unaffected), variants, permutations)
LABEL_CASES = [((37, 45), 70, 129),                      # a second pass of one permutation; two variant tiles, the second ragged
               ((37, 45), 17, 256),                      # two whole passes: label_rows == n_perms, no zero rows behind the matrix
               ((64, 64), 150, 300),                     # three passes, the last ragged inside a 16-column tile; three variant tiles
               ((2, 3), 1, 1100),                        # nine passes over one row: n_ge is the sum of nine workgroups' atomics
               ((2100, 2200), 20, 40)]                   # 68 k-steps and more of the double-buffered label staging, one pass
LABEL_IDS = ["%d+%d-%d-%d" % (w + (nv, P)) for w, nv, P in LABEL_CASES]
NO_BRACKET = ((2, 3), 1, 1100)                           # T - I is a sixth of its pairs: the engine-derived expectation only


def _special(n_perms):
    """the special label rows of a case of several passes: nobody affected at row 128 + 3 (where the matrix has that row and
    the two below leave it free), everybody at n_perms - 2, a copy of the observed labelling in the last row"""
    if n_perms <= PT:
        return ()
    rows = [(n_perms - 2, "everybody"), (n_perms - 1, "observed")]
    if PT + 3 < n_perms - 2:
        rows.insert(0, (PT + 3, "nobody"))
    return tuple(rows)


def _obj(a):
    return np.asarray(a).astype(object)


def _bracket(num, den, num_o, den_o, same, what):
    """The exact bracket of n_ge.  The statistic of variant v under permutation p is num[v, p] / den[v, p] times a positive
    factor common to the row, the observed one num_o[v] / den_o[v] times the same factor; den == 0 marks a NaN; all Python
    integers in object arrays.  same[v, p]: the two sums are the observed ones.  Asserts the two conditions of the module
    docstring and returns (lower bound, upper bound, pairs compared, ties that are not identical) with the bounds per variant."""
    ok = (den != 0) & (den_o != 0)[:, None]
    lhs, rhs = num * den_o[:, None], num_o[:, None] * den
    greater, tie = ok & (lhs > rhs), ok & (lhs == rhs)
    ident = ok & same
    assert not (ident & ~tie).any(), what
    near = ok & ~tie & (abs(lhs - rhs) * 10 ** 12 <= np.maximum(lhs, rhs))
    assert not near.any(), "%s: %d pairs within 1e-12 of the observed statistic that are no exact tie" % (what, near.sum())
    band, pairs = int((tie & ~ident).sum()), int(ok.sum())
    assert pairs > 0 and 100 * band <= pairs, "%s: %d ties that are not identical among %d pairs" % (what, band, pairs)
    G, T, I = greater.sum(axis=1), tie.sum(axis=1), ident.sum(axis=1)
    return G + I, G + T, pairs, band


def _bracket_allelic(obs, perm):
    """of the oracle's observed counts [nv, 4] = {A1, A2, U1, U2} and permuted counts [nv, P, 4]: with a = A1_p, c = A2_p,
    b = R1 - a, d = R2 - c the chi-square is N (ad - bc)^2 / ((a + c)(b + d) R1 R2), and N, R1, R2 are the row's"""
    a, c, b, d = (_obj(perm[:, :, k]) for k in range(4))
    ao, co, bo, do = (_obj(obs[:, k]) for k in range(4))
    R1, R2 = ao + bo, co + do
    same = (perm[:, :, 0] == obs[:, None, 0]) & (perm[:, :, 1] == obs[:, None, 1])
    return _bracket((a * d - b * c) ** 2, (a + c) * (b + d) * (R1 * R2)[:, None], (ao * do - bo * co) ** 2, (ao + co) * (bo + do) * R1 * R2,
                    same, "allelic")


def _bracket_trend(c8, sums):
    """of the observed class counts and the permuted sums [nv, P, 2] = {R_p, D_p}: with a = N D - R W1 the statistic is
    N a^2 / (R (N - R) (N W2 - W1^2)), and N, W1, W2 are the row's"""
    _, _, _, Ro, N, W1, W2, Do = (_obj(x) for x in mg.margins(c8))
    R, D = _obj(sums[:, :, 0]), _obj(sums[:, :, 1])
    spread = N * W2 - W1 * W1
    same = (sums[:, :, 0] == np.asarray(Ro, np.int64)[:, None]) & (sums[:, :, 1] == np.asarray(Do, np.int64)[:, None])
    return _bracket((N[:, None] * D - R * W1[:, None]) ** 2, R * (N[:, None] - R) * spread[:, None], (N * Do - Ro * W1) ** 2, Ro * (N - Ro) * spread,
                    same, "trend")


def _report(form, case, n_ge, lo, hi, pairs, band):
    """printed, not asserted: the one place where the result depends on the engine's rounding"""
    counted = int((n_ge.astype(np.int64) - lo.astype(np.int64)).sum())
    print("%s %s: %d compared pairs, %d exact ties with other sums than the observed ones, %d of them counted by the engine"
          % (form, case, pairs, band, counted))


# ------------------------------------------------------------------------------------------------ A. label kernel, passes

@pytest.mark.parametrize("i,width,nv,n_perms", [(i,) + k for i, k in enumerate(LABEL_CASES)], ids=LABEL_IDS)
def test_allelic_passes(i, width, nv, n_perms):
    strict, special = i % 2 == 0, _special(n_perms)
    c = ap._case(width, nv, n_perms, strict, special)
    obs, perm = c["obs"], c["perm"]
    bracket = _bracket_allelic(obs, perm) if (width, nv, n_perms) != NO_BRACKET else None
    exp_ge, exp_max, t_obs = ap._reference(width, nv, n_perms, strict, special)
    e = ap._engine(c)
    counts, n_ge, bmax, pc = ap._run_dev(e, c)
    e.close()
    assert np.array_equal(counts, obs)
    # counts, bit-exact, under every relabelling; the unaffected side by difference from the observed row totals
    assert np.array_equal(pc[:, :, 0], perm[:, :, 0]) and np.array_equal(pc[:, :, 1], perm[:, :, 1])
    R1, R2 = obs[:, 0] + obs[:, 2], obs[:, 1] + obs[:, 3]
    assert np.array_equal(R1[:, None] - pc[:, :, 0], perm[:, :, 2]) and np.array_equal(R2[:, None] - pc[:, :, 1], perm[:, :, 3])
    assert np.array_equal(pc[:, 0, :], counts[:, :2])                   # row 0 is the observed labelling
    assert not special or special[-1][0] >= PT
    for row, kind in special:                                           # and the rows of the later passes
        if kind == "observed":
            assert np.array_equal(pc[:, row, :], counts[:, :2])
        else:
            assert np.array_equal(pc[:, row, :], 0 * counts[:, :2] if kind == "nobody" else np.stack([R1, R2], axis=1))
            assert bmax[row] == 0.0                                     # an empty margin on every row: the 7.0 is gone all the same
    # statistics, exact against the engine's chi-square kernel on the oracle's tables
    assert np.array_equal(n_ge, exp_ge)
    assert np.array_equal(bmax.view(np.uint64), exp_max.view(np.uint64))
    assert np.all(n_ge[np.isnan(t_obs)] == 0)
    if nv >= 3:
        assert np.isnan(t_obs[1]) and np.isnan(t_obs[2])
    else:
        assert not np.isnan(t_obs).any()
    if special:                                                         # the last row equals the observed statistic on every row that has one
        assert np.all(n_ge[~np.isnan(t_obs)] >= 2)
    if n_perms > 8 * PT:
        assert n_ge[0] > PT                                             # more than one workgroup added to it
    # and against the oracle's own arithmetic
    chi_orc = orc.assoc_stats(orc.TASK_CHISQ, *[perm[:, :, k].reshape(-1) for k in range(4)])[1].reshape(nv, n_perms)
    assert_close(bmax, np.fmax.reduce(chi_orc, axis=0, initial=0.0), "batch_max")
    # the exact bracket: no part of it is the engine's
    if bracket:
        lo, hi, pairs, band = bracket
        assert np.array_equal(hi == 0, np.isnan(t_obs))                 # no pair compared: exactly the rows without a statistic
        assert np.all(lo <= n_ge) and np.all(n_ge <= hi), (n_ge, lo, hi)
        _report("allelic", (width, nv, n_perms), n_ge, lo, hi, pairs, band)


@pytest.mark.parametrize("i,width,nv,n_perms", [(i,) + k for i, k in enumerate(LABEL_CASES)], ids=LABEL_IDS)
def test_trend_passes(i, width, nv, n_perms):
    quirks, special = i % 2 == 1, _special(n_perms)
    c = mg.case(width, nv, n_perms, quirks, special=special)
    sums, exp_ge, exp_max, t_obs, exact = tp._reference(width, nv, n_perms, quirks, special)
    bracket = _bracket_trend(c["c8"], sums) if (width, nv, n_perms) != NO_BRACKET else None
    e = mg.engine(c)
    got = mg.run_dev(e, c, perm=True)
    e.close()
    c8, n_ge, bmax = got["counts8"], got["n_ge"], got["batch_max"]
    assert np.array_equal(c8, c["c8"])
    assert np.array_equal(got["sums"], sums)
    Ro, Do = c8[:, 0:3].sum(axis=1), c8[:, 1] + 2 * c8[:, 2]
    assert np.array_equal(got["sums"][:, 0, 0], Ro) and np.array_equal(got["sums"][:, 0, 1], Do)      # row 0 is the observed labelling: (R, D)
    n = c8[:, 0:3] + c8[:, 3:6]
    assert not special or special[-1][0] >= PT
    for row, kind in special:                                           # and the rows of the later passes
        if kind == "observed":
            assert np.array_equal(got["sums"][:, row, 0], Ro) and np.array_equal(got["sums"][:, row, 1], Do)
        else:
            everybody = np.stack([n.sum(axis=1), n[:, 1] + 2 * n[:, 2]], axis=1)
            assert np.array_equal(got["sums"][:, row, :], 0 * everybody if kind == "nobody" else everybody)
            assert bmax[row] == 0.0                                     # an empty margin on every row: the 7.0 is gone all the same
    assert np.array_equal(n_ge, exp_ge)
    assert np.array_equal(mg.bits(bmax), mg.bits(exp_max))
    assert np.array_equal(mg.bits(got["chisq5"][:, mg.TREND]), mg.bits(t_obs))
    assert np.all(n_ge[np.isnan(t_obs)] == 0)
    if nv >= 3:
        assert np.isnan(t_obs[1]) and np.isnan(t_obs[2])
    else:
        assert not np.isnan(t_obs).any()
    if special:
        assert np.all(n_ge[~np.isnan(t_obs)] >= 2)
    if n_perms > 8 * PT:
        assert n_ge[0] > PT                                             # more than one workgroup added to it
    assert_close(bmax, np.fmax.reduce(exact, axis=0, initial=0.0), "batch_max", TOL)
    assert not np.isinf(bmax).any()
    if bracket:
        lo, hi, pairs, band = bracket
        assert np.array_equal(hi == 0, np.isnan(t_obs))                 # no pair compared: exactly the rows without a statistic
        assert np.all(lo <= n_ge) and np.all(n_ge <= hi), (n_ge, lo, hi)
        _report("trend", (width, nv, n_perms), n_ge, lo, hi, pairs, band)


# ------------------------------------------------------------------------------------------------ B. TDT, the folded grid

# (fast trios, slow families, variants, permutations), further flip rows, further variants that take no part
TDT_CASES = [
    # 9 tiles rounded to 16 and three passes, the last of 4 permutations: tile 8 is the first whose workgroups come after the
    # passes of eight others, and the workgroups of tiles 9 .. 15 leave without writing
    ((16, 3, 520, 260), ((130, "all"), (257, "none")), (515,)),
    # 18 tiles: three groups of eight, the last ragged; two passes
    ((70, 20, 1100, 130), ((64, "all"), (128, "none")), (600, 1090)),
    # nine passes over one row, no tail
    ((5, 0, 1, 1100), ((600, "all"), (1030, "none")), ()),
]


def _check_tdt(c, special, tu, n_ge, bmax, pt):
    assert np.array_equal(tu[:, 0], c["t1"]) and np.array_equal(tu[:, 1], c["t2"])
    assert np.array_equal(pt, c["perm_tu"])
    assert np.array_equal(n_ge, c["n_ge"])
    assert np.array_equal(td._bits(bmax), td._bits(c["bmax"]))
    assert np.array_equal(pt[:, 0, :], tu)                               # no family flipped: the observed transmission
    for row, kind in special:
        assert np.array_equal(pt[:, row, :], tu if kind == "none" else tu[:, ::-1])
    assert np.array_equal(pt[:, c["n_perms"] - 1, :], tu[:, ::-1])      # every family flipped
    # rows 0 and n_perms - 1 and every special row reach the observed statistic (a swap of the two counts keeps it)
    assert np.all(n_ge[c["part"]] >= 2 + len(special)) and not n_ge[~c["part"]].any()


@pytest.mark.parametrize("shape,special,no_part", TDT_CASES, ids=["%d-%d-%d-%d" % k[0] for k in TDT_CASES])
def test_tdt_folded_grid(shape, special, no_part):
    c = td._case(*shape, special=special, no_part=no_part)
    nv, n_perms = shape[2], shape[3]
    passes = -(-n_perms // PT)
    # the reference places the rows where the case says: the last pass, a pass that is neither the first nor (with three and
    # more) the last, and variants past row 512 that take no part
    assert any(kind == "none" and row >= (passes - 1) * PT for row, kind in special)
    assert any(kind == "all" and (passes < 3 or PT <= row < (passes - 1) * PT) for row, kind in special)
    assert all(not c["part"][v] for v in no_part) and (nv < 512 or any(v > 512 for v in no_part))
    assert c["part"].sum() > nv // 4
    if nv == 1:
        assert c["n_ge"][0] > PT                                         # more than one workgroup added to it
    e = td._engine(c)
    tu, n_ge, bmax, pt = td._run_dev(e, c)
    e.close()
    _check_tdt(c, special, tu, n_ge, bmax, pt)


def test_tdt_folded_grid_text_lines_cut_short():
    shape, special, no_part = TDT_CASES[0]
    c = td._case(*shape, special=special, no_part=no_part)
    nv = c["nv"]
    chi = td._chisq(c["perm_tu"][:, :, 0], c["perm_tu"][:, :, 1])
    top = np.argmax(np.where(c["part"][:, None], chi, 0.0), axis=0)      # the row that holds each permutation's maximum
    cut = sorted({3, int(top[top <= 512][0]), int(top[(top > 512) & (top < nv - 1)][0]), nv - 1})
    assert len(cut) == 4 and cut[2] > 512                                # four lines cut short, two of them beyond row 512
    keep = np.ones(nv, bool)
    keep[cut] = False
    exp_max = np.max(np.where((c["part"] & keep)[:, None], chi, 0.0), axis=0, initial=0.0)
    assert not np.array_equal(exp_max, c["bmax"])                        # leaving the rows out changes the maxima
    lines = td._text(c["codes"], c["is_x"]).split(b"\n")[:-1]
    text = b"".join((l if keep[i] else b"7\t5\trs") + b"\n" for i, l in enumerate(lines))
    e = td._engine(c)
    rt = e.tdt_perm_text(text)
    e.close()
    assert rt["n_lines"] == nv and np.array_equal(rt["status"] != 0, ~keep)
    assert np.array_equal(rt["n_ge"][keep], c["n_ge"][keep]) and not rt["n_ge"][~keep].any()
    assert np.array_equal(td._bits(rt["batch_max"]), td._bits(exp_max))
    assert np.array_equal(rt["t1"][keep], c["t1"][keep]) and np.array_equal(rt["t2"][keep], c["t2"][keep])


# ------------------------------------------------------------------------------------------------ C. TDT, the i8 operand at +-126

@functools.lru_cache(maxsize=None)
def _case_i8():
    """20 slow families of 63 counted children (the most hpgv_set_tdt_flips takes; 20 give a tail of two chunks per row), 10 fast
    trios and the spare columns of _pedigree; 40 rows, 40 flip rows"""
    rng = np.random.default_rng(6363)
    n_fast, n_slow, nv, n_perms = 10, 20, 40, 40
    ns, fam = td._pedigree(rng, n_fast, n_slow, slow_children=63)
    fcol, mcol, coff, ccol, _ = fam
    slow = [f for f in range(len(fcol)) if fcol[f] >= 0 and coff[f + 1] - coff[f] == 63]
    assert len(slow) == n_slow
    codes = random_codes(rng, nv, ns, quirks=True)
    codes[nv // 2:] = random_codes(rng, nv - nv // 2, ns, quirks=False)

    def fill(v, families, child):
        """both parents heterozygous, every child the same homozygote"""
        for f in families:
            codes[v, fcol[f]] = codes[v, mcol[f]] = 0x01
            codes[v, ccol[coff[f]:coff[f + 1]]] = child

    for v in range(0, 6):
        fill(v, slow, 0x11)
    for v in range(6, 12):
        fill(v, slow, 0x00)
    for v in range(12, 20):                              # half the families one way, half the other
        fill(v, slow[v % 2::2], 0x11)
        fill(v, slow[1 - v % 2::2], 0x00)
    is_x = (np.arange(nv) % 3 == 2).astype(np.uint8)
    flips = (rng.random((n_perms, len(fcol))) < rng.uniform(0.2, 0.8, size=(n_perms, 1))).astype(np.uint8)
    flips[0], flips[1], flips[n_perms - 1] = 0, 1, 1
    flips[2] = np.arange(len(fcol)) % 2
    flips[3, slow] = np.arange(n_slow) % 2               # alternating slow families
    return td._finish(ns, fam, codes, is_x, flips, n_fast, n_slow)


def test_tdt_i8_operand_at_its_limit():
    c = _case_i8()
    d_f = c["d_f"]
    D_p = c["perm_tu"][:, :, 0].astype(np.int64) - c["perm_tu"][:, :, 1]
    # the case says something: both ends of the i8 range that the setter admits, and sums far outside it
    assert d_f.max() == 126 and d_f.min() == -126
    assert np.abs(D_p).max() >= 2000
    assert (np.abs(d_f) > 100).sum() >= 200 and c["part"].sum() >= 30
    e = td._engine(c)
    tu, n_ge, bmax, pt = td._run_dev(e, c)
    res = e.tdt(c["codes"], c["is_x"])
    e.close()
    _check_tdt(c, ((1, "all"),), tu, n_ge, bmax, pt)
    odds, chisq, p = orc.tdt_stats(c["t1"], c["t2"])
    assert np.array_equal(res["t1"], c["t1"]) and np.array_equal(res["t2"], c["t2"])
    assert np.array_equal(td._bits(res["chisq"]), td._bits(chisq)) and np.array_equal(td._bits(res["odds"]), td._bits(odds))
    assert_p_close(res["p"], p, "tdt p")


# ------------------------------------------------------------------------------------------------ D. layout options

OPT_CASE = ((37, 45), 150, 130, True)


def _run_both_forms(options):
    """the model scan and statistics, the trend form and the allelic form of the permutation kernel on OPT_CASE, on an engine
    with `options` set before the cohort"""
    c = mg.case(*OPT_CASE, special=_special(OPT_CASE[2]))
    e = hpgv.Engine(0)
    for key, value in options:
        set_or_skip(e, key, value)
    e.set_cohort(c["cond"])
    e.set_perm_labels(c["labels"])
    got = mg.run_dev(e, c, perm=True)
    counts, n_ge, bmax, pc = ap._run_dev(e, dict(c, is_x=np.zeros(c["nv"], np.uint8)))
    pitch = e.assoc_layout()[2]
    e.close()
    got.update(a_counts=counts, a_n_ge=n_ge, a_batch_max=bmax, a_perm_counts=pc, pitch=pitch)
    return c, got


@functools.lru_cache(maxsize=None)
def _default_forms():
    return _run_both_forms(())[1]


@pytest.mark.parametrize("key,value", [("row_align", 128), ("row_align", 256), ("variants_per_wave", 1), ("variants_per_wave", 7), ("nontemporal", 0)])
def test_options_do_not_change_label_permutation(key, value):
    c, got = _run_both_forms(((key, value),))
    ref = _default_forms()
    if key == "row_align":
        assert got["pitch"] % value == 0 and got["pitch"] != ref["pitch"]
    for k in ("counts8", "sums", "n_ge", "a_counts", "a_n_ge", "a_perm_counts"):
        assert np.array_equal(got[k], ref[k]), k
    for k in ("chisq5", "p5", "batch_max", "a_batch_max"):
        assert np.array_equal(mg.bits(got[k]), mg.bits(ref[k])), k
    assert np.array_equal(got["counts8"], c["c8"])                       # and the counts are numpy's, not only one another's
    assert got["n_ge"].any() and got["a_n_ge"].any() and got["batch_max"].any() and got["a_batch_max"].any()


def test_row_align_does_not_change_tdt_permutation():
    c = td._case(*td.MID)
    e = hpgv.Engine(0)
    set_or_skip(e, "row_align", 128)
    assert e.set_families(c["ns"], *c["fam"])[:2] == (c["n_fast"], c["n_slow"])
    pitch = e.tdt_layout()[2]
    assert pitch % 128 == 0
    e.set_tdt_flips(c["flips"])
    tu, n_ge, bmax, pt = td._run_dev(e, c)
    e.close()
    d = td._engine(c)
    assert d.tdt_layout()[2] != pitch                                    # the default engine's rows are another length
    ref = td._run_dev(d, c)
    d.close()
    for a, b in zip((tu, n_ge, td._bits(bmax), pt), (ref[0], ref[1], td._bits(ref[2]), ref[3])):
        assert np.array_equal(a, b)
    _check_tdt(c, (), tu, n_ge, bmax, pt)


# ------------------------------------------------------------------------------------------------ E. limits and state

TOO_MANY = (1 << 20) + 1


def test_too_many_label_rows_are_refused_and_the_earlier_stay():
    shape = ((1, 1), 5, 33, True)                                        # a cohort of two columns, 33 label rows
    c = ap._case(*shape)
    exp_ge, exp_max, _ = ap._reference(*shape)
    assert exp_ge.any() and exp_max.any()
    e = ap._engine(c)
    lab = np.ascontiguousarray(c["labels"])
    for _ in range(2):
        _, n_ge, bmax, _ = ap._run_dev(e, c)
        assert np.array_equal(n_ge, exp_ge) and np.array_equal(bmax.view(np.uint64), exp_max.view(np.uint64))
        assert e.L.hpgv_set_perm_labels(e.h, C.c_void_p(lab.ctypes.data), TOO_MANY) == hpgv.ERR_UNSUPPORTED
    e.close()


def test_too_many_flip_rows_are_refused_and_the_earlier_stay():
    rng = np.random.default_rng(33)
    fam = (np.array([0], np.int32), np.array([1], np.int32), np.array([0, 1], np.int32), np.array([2], np.int32), np.array([1], np.uint8))
    codes = random_codes(rng, 12, 3, quirks=False)
    codes[0] = [0x01, 0x01, 0x11]                                        # a row that surely takes part
    is_x = (np.arange(12) % 4 == 3).astype(np.uint8)
    flips = rng.integers(0, 2, size=(33, 1)).astype(np.uint8)
    flips[0], flips[32] = 0, 1
    c = td._finish(3, fam, codes, is_x, flips, 1, 0)
    assert c["n_ge"].any() and c["bmax"].any()
    e = td._engine(c)
    fl = np.ascontiguousarray(flips)
    for _ in range(2):
        tu, n_ge, bmax, pt = td._run_dev(e, c)
        _check_tdt(c, (), tu, n_ge, bmax, pt)
        assert e.L.hpgv_set_tdt_flips(e.h, C.c_void_p(fl.ctypes.data), TOO_MANY) == hpgv.ERR_UNSUPPORTED
    e.close()


# ------------------------------------------------------------------------------------------------ F. host plumbing of the entry points

# Shapes that cross every boundary of the plumbing once: 37 columns (no multiple of 16), 70 rows or lines (a second, ragged
# 64-variant tile), 130 permutations (a second pass); the pedigree has two two-child families, so that the slow tail exists
PLUMB = ((16, 17), 70, 130, True)
PLUMB_WINDOW = 12
LINE_FILTERED = 0x100                                                    # HPGV_LINE_FILTERED of include/hpgv.h
CUT, RARE = 40, 66                                                       # the line cut short; the record below the frequency filter
I32, F64 = np.int32, np.float64

# the per-line outputs of the text forms in the order of their C signatures: (name, dtype, shape of one line's part)
TEXT_FORMS = {
    "assoc_perm": ("hpgv_assoc_perm_text", [(k, I32, ()) for k in ("A1", "A2", "U1", "U2")] + [(k, F64, ()) for k in ("odds", "chisq", "p")] + [("n_ge", I32, ())]),
    "model": ("hpgv_assoc_model_text", [("counts8", I32, (8,)), ("chisq5", F64, (5,)), ("p5", F64, (5,)), ("n_ge", I32, ())]),
    "tdt_perm": ("hpgv_tdt_perm_text", [("t1", I32, ()), ("t2", I32, ())] + [(k, F64, ()) for k in ("odds", "chisq", "p")] + [("n_ge", I32, ())]),
    "ld": ("hpgv_ld_text", [("r2", F64, (PLUMB_WINDOW,)), ("counts6", I32, (PLUMB_WINDOW, 6))]),
}


@functools.lru_cache(maxsize=None)
def _plumb_labels():
    """mg.case(PLUMB) with chromosome flags; row RARE is all reference but for one heterozygous call in a cohort column"""
    c = dict(mg.case(*PLUMB))
    assert c["ns"] == 37
    codes = c["codes"].copy()
    codes[RARE] = 0x00
    codes[RARE, np.flatnonzero(c["cond"] == 1)[2]] = 0x01
    c.update(codes=codes, is_x=(np.arange(c["nv"]) % 5 == 3).astype(np.uint8))
    return c


@functools.lru_cache(maxsize=None)
def _plumb_families():
    """three trios and two two-child families over 37 columns; row RARE is all reference but for one heterozygous father of a trio"""
    rng = np.random.default_rng(3737)
    ns, fam = td._pedigree(rng, 3, 2, slow_children=2)
    assert ns == 37
    nv, n_perms = PLUMB[1], PLUMB[2]
    codes = random_codes(rng, nv, ns, quirks=True)
    codes[nv // 2:] = random_codes(rng, nv - nv // 2, ns, quirks=False)
    fcol, _, coff, _, _ = fam
    trio = [f for f in range(len(fcol)) if fcol[f] >= 0 and coff[f + 1] - coff[f] == 1][0]
    codes[RARE] = 0x00
    codes[RARE, fcol[trio]] = 0x01
    is_x = (np.arange(nv) % 5 == 3).astype(np.uint8)
    assert not is_x[RARE]
    flips = (rng.random((n_perms, len(fcol))) < rng.uniform(0.2, 0.8, size=(n_perms, 1))).astype(np.uint8)
    flips[0], flips[n_perms - 1] = 0, 1
    c = td._finish(ns, fam, codes, is_x, flips, 3, 2)
    assert c["part"][RARE] and c["part"][CUT]
    return c


def _plumb_engine(form, filters=False):
    c = _plumb_families() if form == "tdt_perm" else _plumb_labels()
    e = td._engine(c) if form == "tdt_perm" else mg.engine(c)
    if filters:                                                          # a frequency filter that rejects row RARE (1 / 74 alleles)
        assert e.L.hpgv_set_stats_cohort(e.h, c["ns"]) == hpgv.OK
        assert e.L.hpgv_set_text_filters(e.h, C.c_double(0.02), C.c_double(-1.0), C.c_long(-1)) == hpgv.OK
    return c, e


def _call_text(e, form, text, max_lines, n_perms, with_status):
    """the form's C entry point on buffers pre-filled with sentinels: (n_lines, dict of every output)"""
    fn, outs = TEXT_FORMS[form]
    m = max(max_lines, 1)
    res = {k: np.full((m,) + shape, 0x5A5A5A5A if dt is I32 else -7.0, dt) for k, dt, shape in outs}
    status = np.full(m, -1, I32) if with_status else None
    nl = C.c_int(-1)
    args = [e.h, text, len(text), max_lines, C.byref(nl), None, None, hpgv._ptr(status)] + ([PLUMB_WINDOW] if form == "ld" else [])
    args += [hpgv._ptr(res[k]) for k, _, _ in outs]
    if form != "ld":
        res["batch_max"] = np.full(n_perms, -7.0)
        args.append(hpgv._ptr(res["batch_max"]))
    assert getattr(e.L, fn)(*args) == hpgv.OK
    return nl.value, res, status


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("form", sorted(TEXT_FORMS))
def test_text_without_a_status_array(form):
    """status == NULL: the call brings the status array that the record filters and the skip bytes need; every output is that of
    the call with one, and the lines that are no records or were filtered take no part"""
    c, e = _plumb_engine(form, filters=True)
    nv, n_perms = c["nv"], c["n_perms"]
    lines = ap._text(c["codes"], c["is_x"]).split(b"\n")[:-1]
    text = b"".join((b"7\t5\trs" if i == CUT else l) + b"\n" for i, l in enumerate(lines))
    nl, res, status = _call_text(e, form, text, nv, n_perms, True)
    nl0, res0, _ = _call_text(e, form, text, nv, n_perms, False)
    assert nl == nl0 == nv
    for k in res:
        assert np.array_equal(_raw(res[k]), _raw(res0[k])), k
    assert (status[CUT] & 0xFF) == 1 and (status[RARE] & LINE_FILTERED) and (status[RARE] & 0xFF) == 0
    skip = ((status & 0xFF) == 1) | ((status & LINE_FILTERED) != 0)
    assert 2 <= skip.sum() < nv // 2
    keep = ~skip
    sub = dict(c, codes=c["codes"][keep], is_x=c["is_x"][keep])
    if form == "ld":
        cohort = c["cond"] != 2
        exp = lg.band(c["codes"][:, cohort], PLUMB_WINDOW, skip=skip.astype(np.uint8))
        lg.assert_same((res0["r2"], res0["counts6"]), exp)
        assert np.isnan(res0["r2"][skip]).all() and np.isfinite(res0["r2"]).sum() > nv
        # and no later row pairs with a skipped one: slot d - 1 of row b is the pair (b - d, b)
        for b in np.flatnonzero(skip):
            for d in range(1, min(PLUMB_WINDOW, nv - 1 - b) + 1):
                assert np.isnan(res0["r2"][b + d, d - 1])
    else:
        if form == "assoc_perm":
            _, n_ge, bmax, _ = ap._run_dev(e, sub)
        elif form == "model":
            got = mg.run_dev(e, sub, perm=True)
            n_ge, bmax = got["n_ge"], got["batch_max"]
        else:
            _, n_ge, bmax, _ = td._run_dev(e, sub)
        assert not res0["n_ge"][skip].any() and np.array_equal(res0["n_ge"][keep], n_ge) and n_ge.any()
        assert np.array_equal(mg.bits(res0["batch_max"]), mg.bits(bmax)) and bmax.any()
        # row RARE would have counted: with every line a record and no filter it reaches its own statistic at least once
        full = {"assoc_perm": lambda: ap._run_dev(e, c)[1], "model": lambda: mg.run_dev(e, c, perm=True)["n_ge"], "tdt_perm": lambda: td._run_dev(e, c)[1]}[form]()
        assert full[RARE] >= 1
    e.close()


@pytest.mark.parametrize("form", ["assoc_perm", "model", "tdt_perm"])
def test_empty_permutation_calls_zero_batch_max(form):
    """no variants, no lines: HPGV_OK, nothing per row, and batch_max -- the identity of the merge by maximum -- written all the same"""
    c, e = _plumb_engine(form)
    n_perms = c["n_perms"]
    fn, outs = TEXT_FORMS[form]
    bmax = np.full(n_perms + 1, -7.0)
    dummy = np.zeros(64, np.uint8)                                       # (the model call wants n_ge with batch_max)
    rows = [None, c["ns"], 0] + ([] if form == "model" else [None])      # gt, pitch, n_variants[, is_x]
    assert getattr(e.L, fn[:-len("_text")])(e.h, *rows, *[hpgv._ptr(dummy)] * len(outs), hpgv._ptr(bmax)) == hpgv.OK
    assert not bmax[:n_perms].any() and bmax[n_perms] == -7.0
    nl, res, _ = _call_text(e, form, b"", 0, n_perms, True)
    assert nl == 0 and not res["batch_max"].any()
    assert all(np.all(res[k] == (0x5A5A5A5A if dt is I32 else -7.0)) for k, dt, _ in outs)
    e.close()


def test_empty_ld_calls():
    """hpgv_ld_edges without rows (hpgv_ld without rows: test_ld_gpu.py::test_host_and_text_entry_points), hpgv_ld_text without lines"""
    c, e = _plumb_engine("ld")
    n = C.c_uint64(99)
    assert e.L.hpgv_ld_edges(e.h, None, c["ns"], 0, PLUMB_WINDOW, None, None, -1, 0.5, None, 0, C.byref(n)) == hpgv.OK and n.value == 0
    nl, res, _ = _call_text(e, "ld", b"", 0, 0, True)
    assert nl == 0 and np.all(res["r2"] == -7.0)
    e.close()


def _tight(codes, pad=11):
    """the rows at a pitch of n_samples + pad in a buffer that ends with the last row's last sample: (buffer, pitch)"""
    nv, ns = codes.shape
    pitch = ns + pad
    buf = np.full((nv - 1) * pitch + ns, 0xEE, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, shape=(nv, ns), strides=(pitch, 1))
    view[:] = codes
    return buf, pitch


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("form", ["labels", "families"])
def test_last_row_need_not_be_a_whole_pitch(form, fused):
    """(n_variants - 1) * pitch + n_samples bytes are all a batch entry point may read of the caller's matrix: on a buffer of exactly
    that size, through the one-pass kernel and through the kernel chain, the results are those of the packed matrix.  (This pins
    the contract; an over-read of the last row's pad would need a guard page to show)"""
    c, e = _plumb_engine("tdt_perm" if form == "families" else "assoc_perm")
    e.set_option("batch_fused", fused)
    nv, n_perms, codes = c["nv"], c["n_perms"], np.ascontiguousarray(c["codes"])
    buf, pitch = _tight(codes)
    assert buf.size == (nv - 1) * pitch + c["ns"] and pitch == c["ns"] + 11
    view = np.lib.stride_tricks.as_strided(buf, shape=codes.shape, strides=(pitch, 1))
    names = TEXT_FORMS["tdt_perm" if form == "families" else "assoc_perm"][1]

    def perm_call(fn):
        res = {k: np.zeros(nv, dt) for k, dt, _ in names}
        res["batch_max"] = np.full(n_perms, -7.0)
        assert fn(e.h, hpgv._ptr(buf), pitch, nv, hpgv._ptr(c["is_x"]), *[hpgv._ptr(res[k]) for k, _, _ in names], hpgv._ptr(res["batch_max"])) == hpgv.OK
        return res

    if form == "families":
        plain, plain_exp = e.tdt_view(view, c["ns"], c["is_x"]), e.tdt(codes, c["is_x"])
        perm, perm_exp = perm_call(e.L.hpgv_tdt_perm), e.tdt_perm(codes, c["is_x"])
        assert np.array_equal(plain_exp["t1"], c["t1"]) and np.array_equal(perm_exp["n_ge"], c["n_ge"])
    else:
        plain, plain_exp = e.assoc_view(hpgv.TASK_CHISQ, view, c["ns"], c["is_x"]), e.assoc(hpgv.TASK_CHISQ, codes, c["is_x"])
        perm, perm_exp = perm_call(e.L.hpgv_assoc_perm), e.assoc_perm(codes, c["is_x"])
        assert perm_exp["n_ge"].any()
        r2, c6 = np.zeros((nv, PLUMB_WINDOW)), np.zeros((nv, PLUMB_WINDOW, 6), I32)
        assert e.L.hpgv_ld(e.h, hpgv._ptr(buf), pitch, nv, PLUMB_WINDOW, None, None, -1, hpgv._ptr(r2), hpgv._ptr(c6)) == hpgv.OK
        ld_exp = e.ld(codes, PLUMB_WINDOW)
        assert np.array_equal(mg.bits(r2), mg.bits(ld_exp["r2"])) and np.array_equal(c6, ld_exp["counts6"]) and c6.any()
    for got, exp in ((plain, plain_exp), (perm, perm_exp)):
        for k in exp:
            assert np.array_equal(_raw(got[k]), _raw(exp[k])), k
    e.close()


def test_text_wrappers_cut_their_outputs_to_the_capacity():
    """n_lines counts every line of the text while the per-line arrays end at the capacity.  With room for five lines the arrays
    have five rows whatever the slice asks for, so that half pins the shapes and values only; the wrappers' min(n_lines, max_lines)
    is pinned by the call with room for none, where their own arrays still hold one row"""
    c, e = _plumb_engine("ld")
    nv, ns = c["nv"], c["ns"]
    text = ap._text(c["codes"], c["is_x"])
    full, five = e.ld_text(text, PLUMB_WINDOW), e.ld_text(text, PLUMB_WINDOW, max_lines=5)
    assert five["n_lines"] == nv and five["r2"].shape == (5, PLUMB_WINDOW) and five["counts6"].shape == (5, PLUMB_WINDOW, 6) and five["status"].shape == (5,)
    assert np.array_equal(mg.bits(five["r2"]), mg.bits(full["r2"][:5])) and np.array_equal(five["counts6"], full["counts6"][:5])
    none = e.tokenize(text, ns, max_lines=0)
    e.close()
    assert none["n_lines"] == nv
    assert none["gt"].shape == (0, ns) and none["is_x"].shape == (0,) and none["status"].shape == (0,) and none["field_off"].shape == (0, 10)
    assert none["line_off"].shape == (1,)
