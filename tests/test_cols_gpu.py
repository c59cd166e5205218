"""The grid that the kernels over sample columns share (cols_item and the triangular decode of cols_pair_walk,
csrc/hpgv_cols_kernels.h) past the shapes of the tools' own suites, which stop at 130 columns for the pair kernels: 321 columns
are 6 column tiles, the last of one column, and 21 tile pairs up to (5, 5).  With the 65 rows in one range the grid is 8 x 3
workgroups for 21 items -- the items are no multiple of 8 and three workgroups find none.  Exact integers against numpy."""
import numpy as np
import pytest

import grm_golden as gg
import ibs_golden as ig
import score_golden as sg
from helpers import hpgv

pytestmark = pytest.mark.gpu

COLS, ROWS, SCORE_ROWS = 321, 65, 300


@pytest.fixture(scope="module")
def eng():
    e = ig.engine()
    yield e
    e.close()


def test_the_shape_is_what_it_is_for():
    tiles = -(-COLS // 64)
    pairs = tiles * (tiles + 1) // 2
    assert (tiles, pairs, COLS - 64 * (tiles - 1)) == (6, 21, 1)
    assert hpgv.ibs_plan_rows(ROWS, COLS, 256) >= ROWS and hpgv.grm_plan_rows(ROWS, COLS, 256) >= ROWS     # one range: 21 items on 24 workgroups
    ranges = -(-SCORE_ROWS // hpgv.score_plan_rows(SCORE_ROWS, COLS, 5, 256))
    assert (tiles * ranges) % 8 != 0                                                                        # score: 12 items on 16


def test_ibs_pairs(eng):
    codes = ig.matrix(ROWS, COLS)
    exp = ig.pair_counts(codes)
    upper = np.triu(np.ones((COLS, COLS), bool), 1)
    assert (exp[upper][:, 0] > 0).all() and exp[320 - 64:320, 320].any()                                    # every pair has rows, the last tile's too
    for fill, what in ((0xFF, "pads 0xFF"), (None, "garbage past n_cols")):
        got = ig.run_dev(eng, ig.lay(codes, fill=fill), COLS)
        ig.check_counts(got, exp, what)
        assert np.array_equal(got[upper], exp[upper]), what


@pytest.mark.parametrize("which", [0, 1], ids=["s11", "s14"])
def test_grm_pairs(eng, which):
    codes = ig.matrix(ROWS, COLS) if which == 0 else gg.balanced(ROWS, COLS)
    s, maf = (gg.DEFAULT, gg.EXTREME)[which]
    G = gg.golden(codes, s, maf)
    upper = np.triu(np.ones((COLS, COLS), bool))
    assert G["used"].sum() >= ROWS // 4 and G["acc"][320, 320, 1] > 0
    for fill, what in ((0xFF, "pads 0xFF"), (None, "garbage past n_cols")):
        got = gg.run_dev(eng, ig.lay(codes, fill=fill), COLS, s, maf)
        gg.check_acc(got, G["acc"], what)
        assert np.array_equal(got[upper], G["acc"][upper]), what


def test_score_cols(eng):
    codes = ig.matrix(SCORE_ROWS, COLS)
    w, s, flags = sg.random_inputs(SCORE_ROWS, 5, 321)
    for impute in (1, 0):
        G = sg.golden(codes, w, s, flags, impute)
        assert G["used"].sum() >= SCORE_ROWS // 2 and G["acc"][:5, 320].all()
        for fill, what in ((0xFF, "pads 0xFF"), (None, "garbage past n_cols")):
            acc, const = sg.run_dev(eng, ig.lay(codes, fill=fill), COLS, w, s, flags, impute)
            sg.check_acc((acc, const), G, "%s, impute %d" % (what, impute))
            assert np.array_equal(acc[:, :COLS], G["acc"]), what
