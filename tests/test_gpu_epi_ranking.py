"""The epistasis rankings (hpgv_epi_rank_pairs / _triples, the matrix-core scans k_epi_pairs_mfma / k_epi_triples_mfma and the
host loop around them: bands from the last row up, per-fold thresholds, growing bands, overflow and retry) against the CPU
oracle's dense scans, never against another GPU kernel.  Every call's kernel is the one hpgv_epi_last_rank_info reports; i, j,
k, accuracy, risky cells and the list lengths are compared exactly (the accuracy is a handful of IEEE double operations on
integer counts)."""
from importlib import import_module

import numpy as np
import pytest

from helpers import all_combs, epi_random_dataset, epi_random_folds, hpgv, oracle_top
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

sharding = import_module("hpg-variant_amd.sharding")
SUBSETS = (hpgv.EPI_TESTING, hpgv.EPI_TRAINING)


@pytest.fixture(scope="module")
def eng():
    e = hpgv.Engine(0)
    yield e
    e.close()


def _load(eng, data, nA, nU, fold, k):
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    return orc.fold_masks_from_assignment(fold, k)


def _same_ranking(res, exp, order, what):
    k = len(exp["n"])
    for f in range(k):
        n = int(exp["n"][f])
        assert int(res["n"][f]) == n, (what, f, int(res["n"][f]), n)
        for key in tuple("ijk"[:order]) + ("accuracy", "risky"):
            assert np.array_equal(res[key][f][:n], exp[key][f][:n]), (what, f, key)


def _rank_pairs(eng, subset, N, kernel, rows=None):
    res = eng.epi_rank_pairs(subset, N, rows=rows)
    info = eng.epi_last_rank_info()
    assert info["kernel"] == kernel, (info, kernel)
    return res, info


def _rank_triples(eng, subset, N, kernel):
    res = eng.epi_rank_triples(subset, N)
    info = eng.epi_last_rank_info()
    assert info["kernel"] == kernel, (info, kernel)
    return res, info


def _chunks(nA, nU, fold, k):
    """staging chunks of the (fold, class) runs as epi_build_folds lays them out: every run padded to 128-sample steps, an even
    number of steps (one of pad bits when none), 8 steps (1024 samples) per chunk"""
    fold = np.asarray(fold)
    steps = 0
    for f in range(k):
        steps += -(-int((fold[:nA] == f).sum()) // 128) + -(-int((fold[nA:] == f).sum()) // 128)
    steps = max(steps, 1)
    steps += steps % 2
    return -(-steps // 8)


# ---- 1. pair ranking, thresholds active ----------------------------------------------------------------------------------
# V = 768 and N <= 25: the first band is rows [640, 767) (8 128 pairs: under the starting 8 192, the next 64-row block would
# pass it), its lists stay below cap / 64 so the band grows x32 to 262 144 pairs, rows [64, 640) (286 400 would pass it), and
# rows [0, 64) are a third launch -- the last two with thresholds from the bands before.  N = 65 536 starts at 2 N pairs:
# rows [256, 767), then the rest.
V_PAIRS = 768


@pytest.mark.parametrize("k,nA,nU,p_missing,what", [
    (1, 128, 128, 0.0, "1 fold, complete data, groups of exactly 128"),
    (2, 254, 258, 0.03, "groups of 127 and 129, missing calls, unequal classes"),
    (2, 700, 650, 0.02, "groups that straddle a 1024-sample chunk"),
    (2, 100, 300, "rare", "ratio 1:3 with rare genotypes: cells exactly on the MDR boundary"),
    (10, 100, 100, 0.0, "10 folds, complete data, equal classes"),
    (11, 132, 110, 0.04, "11 folds, missing calls, unequal classes"),
    (16, 112, 128, 0.0, "16 folds, complete data, unequal classes"),
    (16, 96, 96, 0.05, "16 folds, missing calls, equal classes"),
])
def test_pair_ranking_against_the_oracle(eng, k, nA, nU, p_missing, what):
    rng = np.random.default_rng(nA * 13 + nU + k)
    v = V_PAIRS
    if p_missing == "rare":
        codes = np.array([0, 1, 2, 255], np.uint8)
        data = codes[rng.choice(4, size=(v, nA + nU), p=[0.93, 0.05, 0.015, 0.005])]
    else:
        data = epi_random_dataset(rng, v, nA, nU, p_missing=p_missing)
        assert (data.max() <= 2) == (p_missing == 0.0)
    data[5, :nA] = rng.choice([1, 2], size=nA); data[600, :nA] = rng.choice([1, 2], size=nA)   # an interaction across the bands
    data[11] = 1                                                     # a monomorphic SNP: empty cells
    fold = epi_random_folds(rng, nA, nU, k)
    masks = _load(eng, data, nA, nU, fold, k)
    sizes = [int((fold[:nA] == f).sum()) for f in range(k)] + [int((fold[nA:] == f).sum()) for f in range(k)]
    if "128" in what:
        assert set(sizes) == {128}
    if "127" in what:
        assert set(sizes) == {127, 129}
    if "straddle" in what:                                           # runs of 3 steps: fold 1's cases are samples 768 .. 1152
        assert all(-(-s // 128) == 3 for s in sizes)
    if p_missing == "rare":                                          # some cell of some pair has cases * nU == controls * nA
        ties = sum(int(((a * nU == u * nA) & (a + u > 0)).sum()) for i in range(0, 40, 2)
                   for a, u in [orc.epi_counts_all_folds([data[i], data[i + 1]], nA, nU, masks)])
        assert ties > 0
    pairs = all_combs(v, 2)
    for subset in SUBSETS:
        acc, rm = orc.epi_scan_pairs(data, nA, nU, masks, subset)
        for N in (1, 25, 65536):
            res, info = _rank_pairs(eng, subset, N, hpgv.EPI_KERNEL_PAIRS_MFMA)
            assert info["launches"] >= (3 if N <= 25 else 2), info
            _same_ranking(res, oracle_top(acc, rm, pairs, N), 2, (what, subset, N))


# ---- 2. triple ranking ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v,k,nA,nU,p_missing", [(72, 2, 130, 127, 0.0), (64, 10, 110, 90, 0.04), (66, 11, 121, 121, 0.0),
                                                 (60, 16, 96, 112, 0.03)])
def test_triple_ranking_against_the_oracle(eng, v, k, nA, nU, p_missing):
    # first SNPs from the last one down, thresholds from the first launches on; N small enough that they filter
    rng = np.random.default_rng(v * 3 + k)
    data = epi_random_dataset(rng, v, nA, nU, p_missing=p_missing)
    data[3, :nA] = rng.choice([1, 2], size=nA); data[v - 5, :nA] = rng.choice([1, 2], size=nA)
    data[7] = 0
    fold = epi_random_folds(rng, nA, nU, k)
    masks = _load(eng, data, nA, nU, fold, k)
    triples = all_combs(v, 3)
    for subset in SUBSETS:
        acc, rm = orc.epi_scan_triples(data, nA, nU, masks, subset)
        for N in (1, 30, 400):
            res, info = _rank_triples(eng, subset, N, hpgv.EPI_KERNEL_TRIPLES_MFMA)
            assert info["launches"] >= 3 and info["relaunches"] == 0, info
            _same_ranking(res, oracle_top(acc, rm, triples, N), 3, (v, k, subset, N))


# ---- 3. ties at the threshold, overflow and retry ------------------------------------------------------------------------

@pytest.mark.parametrize("nA,nU", [(50, 46), (123, 141)])
def test_ties_at_the_threshold_and_the_overflow_retry(eng, nA, nU):
    # SNPs 0 .. 999 are copies of one SNP that separates cases (genotype 2) from controls (0): every pair of two copies, and every
    # pair of a copy with a noise SNP that has no missing call in the evaluated part, has accuracy exactly 1 in every fold
    # (0.7 to 1.4 million models per fold).  SNPs 1000 .. 2999 are noise with missing calls.  The ranking is the lexicographically
    # smallest of the tied models.
    # The host loop (cap = max(2^20, 64 V) = 1 048 576 models per fold): bands from row 2999 up.  The first, rows [2880, 2999),
    # lists its 7 140 pairs; lists below cap / 64 grow the band x32 (262 144 pairs: rows [2304, 2880)), lists below cap / 8 x4
    # (1 048 576: rows [1408, 2304)), noise only so far and near-empty lists against the thresholds: x32 again, which takes every
    # row left, [0, 1408) -- and 2.5 million of its models per fold reach thresholds below 1.  That list overflows: the band
    # again with half its pairs (1 616 032), [640, 1408) and on, where the lists fill with models of accuracy 1 and the thresholds
    # become 1; the later bands [64, 640) and [0, 64) hold SMALLER tied models that must still be listed (accuracy >= threshold,
    # and the single-precision pre-filter must not drop them).
    # Class sizes: testing parts of 17 / 17 / 16 cases and 16 / 15 / 15 controls; then of 41 cases and 47 controls, where the
    # pair scan's single-precision estimate of an accuracy of 1 is 1 - 2^-24, below the threshold 1: only the pre-filter's slack
    # lets those ties through to the double-precision comparison.
    rng = np.random.default_rng(5)
    v, copies, k, N = 3000, 1000, 3, 2000
    f32 = np.float32
    if nA == 123:
        assert f32(0.5) * (f32(41) * f32(1 / 41) + f32(47) * f32(1 / 47)) < f32(1)
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.05)
    data[:copies, :nA] = 2
    data[:copies, nA:] = 0
    fold = epi_random_folds(rng, nA, nU, k)
    masks = _load(eng, data, nA, nU, fold, k)
    pairs = all_combs(v, 2)
    for subset in SUBSETS:
        acc, rm = orc.epi_scan_pairs(data, nA, nU, masks, subset)
        assert all(int((acc[f] == 1.0).sum()) >= copies * (copies - 1) // 2 for f in range(k))
        exp = oracle_top(acc, rm, pairs, N)
        del acc, rm
        assert np.all(exp["accuracy"][:, :N] == 1.0)
        res, info = _rank_pairs(eng, subset, N, hpgv.EPI_KERNEL_PAIRS_MFMA)
        assert info["relaunches"] >= 1 and info["launches"] >= 5, info
        _same_ranking(res, exp, 2, ("ties", subset))
        # row bands (one GPU's share each, sharding.pair_row_range): the merged lists are the same ranking
        for world in (2, 3):
            parts = [_rank_pairs(eng, subset, N, hpgv.EPI_KERNEL_PAIRS_MFMA, rows=sharding.pair_row_range(g, world, v))[0]
                     for g in range(world)]
            for f in range(k):
                merged = sorted((-float(p["accuracy"][f][e]), int(p["i"][f][e]), int(p["j"][f][e]), int(p["risky"][f][e]))
                                for p in parts for e in range(int(p["n"][f])))[:N]
                assert [(i, j, r) for _, i, j, r in merged] == [(int(x), int(y), int(r)) for x, y, r in
                                                               zip(exp["i"][f], exp["j"][f], exp["risky"][f])], (world, f)


@pytest.mark.parametrize("nA,nU,k", [(50, 46, 3), (37, 41, 5)])
def test_triple_ties_at_the_threshold(eng, nA, nU, k):
    # copies of a separating SNP at the low indices: many triples of accuracy exactly 1, found by launches after the thresholds
    # became 1 (first SNPs from the last one down): every one of the smallest must be listed
    rng = np.random.default_rng(nA + k)
    v, copies = 64, 12
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.05)
    data[:copies, :nA] = 2
    data[:copies, nA:] = 0
    data[40:44, :nA] = 1                                             # a second block: ties at 1 at high first SNPs too
    data[40:44, nA:] = 0
    fold = epi_random_folds(rng, nA, nU, k)
    masks = _load(eng, data, nA, nU, fold, k)
    triples = all_combs(v, 3)
    for subset in SUBSETS:
        acc, rm = orc.epi_scan_triples(data, nA, nU, masks, subset)
        for N in (3, 150, 1000):
            exp = oracle_top(acc, rm, triples, N)
            assert np.all(exp["accuracy"][:, :N] == 1.0)
            res, info = _rank_triples(eng, subset, N, hpgv.EPI_KERNEL_TRIPLES_MFMA)
            assert info["launches"] >= 3, info
            _same_ranking(res, exp, 3, ("triple ties", subset, N))


# ---- 4. folds that lack a class, ranking mode ----------------------------------------------------------------------------

@pytest.mark.parametrize("v,nA,nU,k", [(12, 20, 2, 4), (12, 2, 21, 4), (12, 3, 3, 3), (12, 1, 40, 2), (80, 300, 4, 7),
                                       (80, 5, 260, 9), (70, 14, 600, 16)])
def test_ranking_on_folds_that_lack_a_class(eng, v, nA, nU, k):
    # fewer cases (or controls) than folds: the matrix-core scans evaluate a fold without controls at the end of its cases
    # (test_u <= 0) and a fold without cases from its controls alone; testing accuracies of 0/0 are NaN and never ranked
    rng = np.random.default_rng(nA * 31 + nU + v)
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.05)
    fold = epi_random_folds(rng, nA, nU, k)
    masks = _load(eng, data, nA, nU, fold, k)
    pairs, triples = all_combs(v, 2), all_combs(v, 3)
    for subset in SUBSETS:
        acc, rm = orc.epi_scan_pairs(data, nA, nU, masks, subset)
        acc3, rm3 = orc.epi_scan_triples(data, nA, nU, masks, subset)
        for N in (10, len(triples)):
            res, _ = _rank_pairs(eng, subset, min(N, 65536), hpgv.EPI_KERNEL_PAIRS_MFMA)
            _same_ranking(res, oracle_top(acc, rm, pairs, min(N, 65536)), 2, ("pairs", subset, N))
            res3, _ = _rank_triples(eng, subset, min(N, 65536), hpgv.EPI_KERNEL_TRIPLES_MFMA)
            _same_ranking(res3, oracle_top(acc3, rm3, triples, min(N, 65536)), 3, ("triples", subset, N))
        if subset == hpgv.EPI_TESTING and min(nA, nU) < k:
            assert np.isnan(acc).any()


# ---- 5. both sides of every fallback condition ---------------------------------------------------------------------------

@pytest.mark.parametrize("nA,nU,k,chunks,pairs_kernel,triples_kernel", [
    # the largest classes of 16-bit counts at 2 folds: exactly 128 chunks (4 groups of 32 767 / 32 768 samples, 256 steps each)
    (65535, 65535, 2, 128, hpgv.EPI_KERNEL_PAIRS_MFMA, hpgv.EPI_KERNEL_TRIPLES_MFMA),
    # a class of 65 536: the 16-bit packing cannot hold it -- vector ALU pairs, no triple ranking at all
    (65536, 1000, 2, 65, hpgv.EPI_KERNEL_PAIRS_VALU, None),
    # both classes below 65 536 but more than 128 chunks: 30 groups of 4 369 / 4 370 samples, 35 steps each, 1 050 steps
    (65535, 65535, 15, 132, hpgv.EPI_KERNEL_PAIRS_VALU, hpgv.EPI_KERNEL_TRIPLES),
])
def test_both_sides_of_the_matrix_core_limits(eng, nA, nU, k, chunks, pairs_kernel, triples_kernel):
    rng = np.random.default_rng(nA + k)
    v = 8
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.02)
    data[2, :nA] = rng.choice([1, 2], size=nA)
    fold = epi_random_folds(rng, nA, nU, k)
    assert _chunks(nA, nU, fold, k) == chunks
    eng.epi_set_dataset(data, nA, nU)
    if max(nA, nU) >= 65536:                                         # no one-fold layout for a class that large: folds first
        with pytest.raises(hpgv.HpgvError, match="no folds"):
            eng.epi_rank_pairs(hpgv.EPI_TESTING, 3)
    eng.epi_set_folds(fold, k)
    masks = orc.fold_masks_from_assignment(fold, k)
    pairs, triples = all_combs(v, 2), all_combs(v, 3)
    for subset in SUBSETS:
        acc, rm = orc.epi_scan_pairs(data, nA, nU, masks, subset)
        for N in (3, len(pairs)):
            res, _ = _rank_pairs(eng, subset, N, pairs_kernel)
            _same_ranking(res, oracle_top(acc, rm, pairs, N), 2, ("pairs", nA, k, subset, N))
        if triples_kernel is None:
            with pytest.raises(hpgv.HpgvError):
                eng.epi_rank_triples(subset, 5)
            continue
        acc3, rm3 = orc.epi_scan_triples(data, nA, nU, masks, subset)
        for N in (3, len(triples)):
            res3, _ = _rank_triples(eng, subset, N, triples_kernel)
            _same_ranking(res3, oracle_top(acc3, rm3, triples, N), 3, ("triples", nA, k, subset, N))


# ---- 6. state that outlives a call ---------------------------------------------------------------------------------------

def _order_oracle(data, nA, nU, masks, subset, order, N):
    combs = all_combs(data.shape[0], order)
    k = masks.shape[0]
    acc = np.zeros((k, len(combs)))
    rm = np.zeros((k, len(combs), 8), np.uint32)
    for c, comb in enumerate(combs):
        a, m, _ = orc.epi_model_wide([data[s] for s in comb], nA, nU, masks, subset)
        acc[:, c], rm[:, c] = a, m
    out = []
    for f in range(k):
        ok = np.flatnonzero(~np.isnan(acc[f]))
        best = ok[np.argsort(-acc[f][ok], kind="stable")[:N]]
        out.append((combs[best], acc[f][best], rm[f][best]))
    return out


def test_consecutive_calls_with_the_state_changing(eng):
    # one engine: candidate lists, thresholds, counters and tile lists outlive a call and are shared by the pair, triple and
    # any-order rankings; folds 16 -> 3 -> 10, a dataset that shrinks and then grows past its first size, the largest N first
    rng = np.random.default_rng(2024)

    def pairs_call(data, nA, nU, masks, subset, N):
        acc, rm = orc.epi_scan_pairs(data, nA, nU, masks, subset)
        res, _ = _rank_pairs(eng, subset, N, hpgv.EPI_KERNEL_PAIRS_MFMA)
        _same_ranking(res, oracle_top(acc, rm, all_combs(data.shape[0], 2), N), 2, ("state pairs", data.shape[0], N))

    def triples_call(data, nA, nU, masks, subset, N):
        acc, rm = orc.epi_scan_triples(data, nA, nU, masks, subset)
        res, _ = _rank_triples(eng, subset, N, hpgv.EPI_KERNEL_TRIPLES_MFMA)
        _same_ranking(res, oracle_top(acc, rm, all_combs(data.shape[0], 3), N), 3, ("state triples", data.shape[0], N))

    def order_call(data, nA, nU, masks, subset, N, order=4):
        res = eng.epi_rank_order(order, subset, N)
        assert eng.epi_last_rank_info()["kernel"] == hpgv.EPI_KERNEL_COMBS
        for f, (combs, acc, rm) in enumerate(_order_oracle(data, nA, nU, masks, subset, order, N)):
            n = len(acc)
            assert int(res["n"][f]) == n
            assert np.array_equal(res["combs"][f][:n], combs) and np.array_equal(res["accuracy"][f][:n], acc)
            assert np.array_equal(res["risky"][f][:n], rm)

    nA, nU = 120, 100
    big = epi_random_dataset(rng, 60, nA, nU, p_missing=0.03)
    big[4, :nA] = rng.choice([1, 2], size=nA)
    eng.epi_set_dataset(big, nA, nU)
    fold = epi_random_folds(rng, nA, nU, 16)
    eng.epi_set_folds(fold, 16)
    m = orc.fold_masks_from_assignment(fold, 16)
    pairs_call(big, nA, nU, m, hpgv.EPI_TESTING, 1770)
    triples_call(big, nA, nU, m, hpgv.EPI_TRAINING, 3000)
    pairs_call(big, nA, nU, m, hpgv.EPI_TRAINING, 40)
    fold = epi_random_folds(rng, nA, nU, 3)                          # fewer folds, same dataset
    eng.epi_set_folds(fold, 3)
    m = orc.fold_masks_from_assignment(fold, 3)
    triples_call(big, nA, nU, m, hpgv.EPI_TESTING, 20)
    pairs_call(big, nA, nU, m, hpgv.EPI_TESTING, 7)
    nA2, nU2 = 90, 130                                               # a smaller dataset
    small = epi_random_dataset(rng, 14, nA2, nU2, p_missing=0.0)
    eng.epi_set_dataset(small, nA2, nU2)
    fold = epi_random_folds(rng, nA2, nU2, 10)
    eng.epi_set_folds(fold, 10)
    m = orc.fold_masks_from_assignment(fold, 10)
    order_call(small, nA2, nU2, m, hpgv.EPI_TESTING, 30)
    pairs_call(small, nA2, nU2, m, hpgv.EPI_TRAINING, 5)
    triples_call(small, nA2, nU2, m, hpgv.EPI_TESTING, 100)
    order_call(small, nA2, nU2, m, hpgv.EPI_TRAINING, 2)
    nA3, nU3 = 70, 90                                                # larger than the first one again
    grown = epi_random_dataset(rng, 72, nA3, nU3, p_missing=0.05)
    eng.epi_set_dataset(grown, nA3, nU3)
    fold = epi_random_folds(rng, nA3, nU3, 10)
    eng.epi_set_folds(fold, 10)
    m = orc.fold_masks_from_assignment(fold, 10)
    triples_call(grown, nA3, nU3, m, hpgv.EPI_TRAINING, 25)
    pairs_call(grown, nA3, nU3, m, hpgv.EPI_TESTING, 300)
    triples_call(grown, nA3, nU3, m, hpgv.EPI_TESTING, 5)


# ---- 7. shares of first SNPs, and the any-order ranking across launches --------------------------------------------------

@pytest.fixture(scope="module")
def cohort40():
    """V = 40, 60 cases, 52 controls, 3 folds, missing calls: the dataset, the fold of every sample, and per subset the oracle's
    dense triple scan (computed once, read by both tests)"""
    rng = np.random.default_rng(40)
    v, nA, nU, k = 40, 60, 52, 3
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.04)
    fold = epi_random_folds(rng, nA, nU, k)
    masks = orc.fold_masks_from_assignment(fold, k)
    scans = {subset: orc.epi_scan_triples(data, nA, nU, masks, subset) for subset in SUBSETS}
    return data, nA, nU, fold, k, scans


def test_triple_ranking_by_shares_of_first_snps(eng, cohort40):
    # hpgv_epi_rank_triples_rows as one GPU of a group calls it: the lists of the shares [0, 7), [7, 19), [19, 40) merge into the
    # whole ranking; first SNPs 38 and 39 begin no triple
    data, nA, nU, fold, k, scans = cohort40
    _load(eng, data, nA, nU, fold, k)
    v, N = data.shape[0], 25
    triples = all_combs(v, 3)
    for subset in SUBSETS:
        exp = oracle_top(*scans[subset], triples, N)
        _same_ranking(eng.epi_rank_triples(subset, N), exp, 3, ("whole", subset))
        parts = [eng.epi_rank_triples(subset, N, rows=rows) for rows in ((0, 7), (7, 19), (19, 40))]
        for f in range(k):
            merged = sorted((-float(p["accuracy"][f][e]), int(p["i"][f][e]), int(p["j"][f][e]), int(p["k"][f][e]), int(p["risky"][f][e]))
                            for p in parts for e in range(int(p["n"][f])))[:N]
            n = int(exp["n"][f])
            assert [(-a, i, j, kk, r) for a, i, j, kk, r in merged] == [
                (float(exp["accuracy"][f][e]), int(exp["i"][f][e]), int(exp["j"][f][e]), int(exp["k"][f][e]), int(exp["risky"][f][e]))
                for e in range(n)], (subset, f)
        empty = eng.epi_rank_triples(subset, N, rows=(38, 40))
        assert not empty["n"].any(), empty["n"]


def test_order_ranking_across_launches_with_thresholds(eng, cohort40):
    # order 3 through the listed-combination kernel: the first launch takes 4 096 of the 9 880 combinations, the second the rest
    # and lists only what reaches the thresholds of the first; ties go by the combination, wherever a launch listed it
    data, nA, nU, fold, k, scans = cohort40
    _load(eng, data, nA, nU, fold, k)
    N = 9
    triples = all_combs(data.shape[0], 3)
    assert len(triples) == 9880
    for subset in SUBSETS:
        exp = oracle_top(*scans[subset], triples, N)
        res = eng.epi_rank_order(3, subset, N)
        info = eng.epi_last_rank_info()
        assert info["kernel"] == hpgv.EPI_KERNEL_COMBS and info["launches"] >= 2, info
        for f in range(k):
            n = int(exp["n"][f])
            assert int(res["n"][f]) == n, (subset, f)
            want = np.stack([exp[key][f][:n] for key in "ijk"], axis=1)
            assert np.array_equal(res["combs"][f][:n], want), (subset, f)
            assert np.array_equal(res["accuracy"][f][:n], exp["accuracy"][f][:n]), (subset, f)
            assert np.array_equal(res["risky"][f][:n, 0], exp["risky"][f][:n]), (subset, f)
