"""Epistasis / MDR counting on the GPU (hpgv_epi_*) against the oracle and the reference's unit-test vectors
(tests/golden/reference_kats.json "epistasis_model").  Integer counts and risky-cell masks bit-exact; the
balanced accuracy is a handful of IEEE double operations on those integers, so it is compared exactly too."""
import numpy as np
import pytest

from helpers import epi_counts_from_reference_masks, epi_random_dataset, epi_random_folds, epi_unpad, hpgv
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = hpgv.Engine(0)
    yield e
    e.close()


def _same(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def test_counts_reference_kat(eng, goldens):
    k = goldens["kats"]["epistasis_model"]["counts"]
    nA, nU = k["num_affected"], k["num_unaffected"]
    rows = np.stack([epi_unpad(r, nA, nU) for r in k["padded_rows"]])
    eng.epi_set_dataset(rows, nA, nU)
    aff, unaff = eng.epi_counts([k["order2"]["rows"]])
    assert aff[0].tolist() == k["order2"]["aff"] and unaff[0].tolist() == k["order2"]["unaff"]
    aff, unaff = eng.epi_counts([k["order3"]["rows"]])
    assert aff[0].tolist() == k["order3"]["aff"] and unaff[0].tolist() == k["order3"]["unaff"]


def test_counts_all_folds_reference_kat(eng, goldens):
    k = goldens["kats"]["epistasis_model"]["counts_all_folds"]
    nA, nU, nf = k["num_affected"], k["num_unaffected"], k["num_folds"]
    rows = np.stack([epi_unpad(r, nA, nU) for r in k["padded_rows"]])
    eng.epi_set_dataset(rows, nA, nU)
    eng.epi_set_fold_masks(np.array(k["padded_fold_masks"], np.uint8), nf)     # the reference's own padded mask array
    aff, unaff = eng.epi_counts([k["order2"]["rows"]], all_folds=True)
    assert aff[:, 0, :].tolist() == k["order2"]["aff"] and unaff[:, 0, :].tolist() == k["order2"]["unaff"]
    aff, unaff = eng.epi_counts([k["order3"]["rows"]], all_folds=True)
    for f, cells in k["order3"]["some_cells"].items():
        for c, (ea, eu) in cells.items():
            assert (aff[int(f)][0][int(c)], unaff[int(f)][0][int(c)]) == (ea, eu), (f, c)
    bad = np.array(k["padded_fold_masks"], np.uint8)
    bad[1][0] = 0                                                     # sample 0 now left out of two folds
    with pytest.raises(hpgv.HpgvError):
        eng.epi_set_fold_masks(bad, nf)


def test_confusion_reference_kats_through_the_pair_scan(eng, goldens):
    # the order-2 confusion-matrix vectors: with the KAT's fold mask as one fold of a 2-fold partition the scan must
    # give the accuracy of the KAT's matrix whenever the MDR rule picks the KAT's risky cells; the matrices
    # themselves are pinned on the oracle (tests/test_epi_oracle.py), here the scan is compared with the oracle
    for case in goldens["kats"]["epistasis_model"]["confusion"]:
        if len(case["padded_rows"]) != 2:
            continue
        nA, nU = case["num_affected"], case["num_unaffected"]
        rows = np.stack([epi_unpad(r, nA, nU) for r in case["padded_rows"]])
        mask = epi_unpad(case["padded_fold_mask"], nA, nU)
        fold = np.where(mask == 1, 1, 0).astype(np.int32)            # training part of fold 0 = fold 1's testing samples
        if len(set(fold.tolist())) < 2:
            continue
        eng.epi_set_dataset(rows, nA, nU)
        eng.epi_set_folds(fold, 2)
        masks = orc.fold_masks_from_assignment(fold, 2)
        for subset in (hpgv.EPI_TESTING, hpgv.EPI_TRAINING):
            acc, rm = eng.epi_scan_pairs(subset)
            eacc, erm = orc.epi_scan_pairs(rows, nA, nU, masks, subset)
            assert np.array_equal(rm, erm.astype(np.uint16)) and _same(acc, eacc), case["line"]


@pytest.mark.parametrize("v,nA,nU,k", [(70, 37, 52, 5), (9, 16, 16, 2), (130, 300, 420, 10), (65, 5, 4, 3), (40, 1100, 1300, 4),
                                       (33, 64, 64, 1), (20, 700, 650, 16), (12, 2500, 2300, 8), (6, 36000, 34000, 2)])   # (the last: rows too long for the LDS form of the plane builder)
def test_pair_scan_matches_the_oracle(eng, v, nA, nU, k):
    rng = np.random.default_rng(v * 7 + k)
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.03)
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    masks = orc.fold_masks_from_assignment(fold, k)
    for subset in (hpgv.EPI_TESTING, hpgv.EPI_TRAINING):
        acc, rm = eng.epi_scan_pairs(subset)
        eacc, erm = orc.epi_scan_pairs(data, nA, nU, masks, subset)
        assert acc.shape == eacc.shape == (k, v * (v - 1) // 2)
        assert np.array_equal(rm, erm.astype(np.uint16)), "risky cells differ"
        assert _same(acc, eacc), "accuracy differs"
    # a band of rows gives the same numbers as the whole scan
    if v > 8:
        a2, m2 = eng.epi_scan_pairs(hpgv.EPI_TRAINING, 3, 8)
        lo = 3 * (2 * v - 3 - 1) // 2
        assert _same(a2, acc[:, lo: lo + a2.shape[1]]) and np.array_equal(m2, rm[:, lo: lo + a2.shape[1]])


@pytest.mark.parametrize("v,nA,nU,k", [(70, 37, 52, 5), (130, 300, 420, 10), (65, 5, 4, 3), (40, 1100, 1300, 4), (33, 64, 64, 1),
                                       (50, 256, 256, 8), (90, 100, 100, 10), (12, 2500, 2300, 8), (21, 3, 40, 2), (24, 300, 280, 12), (18, 160, 160, 16)])
def test_pair_scan_on_a_dataset_without_missing_calls(eng, v, nA, nU, k):
    # complete data takes its own counting path (four cells counted, five derived from per-SNP genotype counts): every pair
    # against the oracle, both subsets; the ranking with every model kept; and the same numbers with the path switched off
    rng = np.random.default_rng(v * 11 + k)
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.0)
    assert data.max() <= 2
    if v > 40:
        data[3] = 0; data[17] = 2; data[29, :nA] = 1                # monomorphic SNPs: whole rows / columns of empty cells
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    masks = orc.fold_masks_from_assignment(fold, k)
    pairs = [(i, j) for i in range(v) for j in range(i + 1, v)]
    for subset in (hpgv.EPI_TESTING, hpgv.EPI_TRAINING):
        acc, rm = eng.epi_scan_pairs(subset)
        eacc, erm = orc.epi_scan_pairs(data, nA, nU, masks, subset)
        assert np.array_equal(rm, erm.astype(np.uint16)), "risky cells differ"
        assert _same(acc, eacc), "accuracy differs"
        res = eng.epi_rank_pairs(subset, len(pairs))
        for f in range(k):
            a = np.where(np.isnan(acc[f]), -np.inf, acc[f])
            order = [p for p in sorted(range(len(pairs)), key=lambda p: (-a[p], pairs[p])) if a[p] > -np.inf]
            n = len(order)
            assert res["n"][f] == n
            assert [(int(x), int(y)) for x, y in zip(res["i"][f][:n], res["j"][f][:n])] == [pairs[p] for p in order]
            assert np.array_equal(res["accuracy"][f][:n], acc[f][order]) and np.array_equal(res["risky"][f][:n], rm[f][order])
    eng.set_option("epi_complete", 0)
    try:
        acc0, rm0 = eng.epi_scan_pairs(hpgv.EPI_TRAINING)
    finally:
        eng.set_option("epi_complete", 1)
    assert _same(acc0, acc) and np.array_equal(rm0, rm)
    # one missing call anywhere switches the path off by itself
    data[v // 2, (nA + nU) // 2] = 255
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    acc1, rm1 = eng.epi_scan_pairs(hpgv.EPI_TESTING)
    eacc1, erm1 = orc.epi_scan_pairs(data, nA, nU, masks, hpgv.EPI_TESTING)
    assert np.array_equal(rm1, erm1.astype(np.uint16)) and _same(acc1, eacc1)


@pytest.mark.parametrize("nA,nU", [(1000, 3000), (333, 999), (1200, 800), (77, 770)])
def test_mdr_rule_on_cells_at_the_boundary(eng, nA, nU):
    # rare genotypes give many small cells whose counts sit exactly on (or one sample off) the cohort's case/control
    # ratio: the division-free form of the rule must decide them as the reference's float sequence does
    rng = np.random.default_rng(nA + nU)
    v, k = 60, 4
    codes = np.array([0, 1, 2, 255], np.uint8)
    data = codes[rng.choice(4, size=(v, nA + nU), p=[0.93, 0.05, 0.015, 0.005])]
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    masks = orc.fold_masks_from_assignment(fold, k)
    acc, rm = eng.epi_scan_pairs(hpgv.EPI_TESTING)
    eacc, erm = orc.epi_scan_pairs(data, nA, nU, masks, 0)
    assert np.array_equal(rm, erm.astype(np.uint16)) and _same(acc, eacc)
    # the data does hold exact ties: some cell of some pair has count_aff * nU == count_unaff * nA (non-empty)
    ties = 0
    for i, j in [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11)]:
        fa, fu = orc.epi_counts_all_folds([data[i], data[j]], nA, nU, masks)
        ties += int(((fa * nU == fu * nA) & (fa + fu > 0)).sum())
    assert ties > 0


def test_counts_order_4_reference_masks_kat(eng, goldens):
    # the four SNPs of test_get_masks (test/test_epistasis_model.c:34-100): the engine's order-4 counts are what
    # combination_counts' arithmetic gives on the reference's own expected masks
    k = goldens["kats"]["epistasis_model"]["masks_order4"]
    nA, nU = k["num_affected"], k["num_unaffected"]
    rows = np.stack([epi_unpad(r, nA, nU) for r in k["padded_rows"]])
    eng.epi_set_dataset(rows, nA, nU)
    aff, unaff = eng.epi_counts([[0, 1, 2, 3]])
    ea, eu = epi_counts_from_reference_masks(k["masks"], nA, nU, 4)
    assert aff[0].tolist() == ea and unaff[0].tolist() == eu
    for sub in ([0, 1, 2], [1, 2, 3], [0, 3]):
        a, u = eng.epi_counts([sub])
        ea, eu = epi_counts_from_reference_masks([k["masks"][s] for s in sub], nA, nU, len(sub))
        assert a[0].tolist() == ea and u[0].tolist() == eu, sub


def test_counts_against_the_oracle_order_2_to_5(eng):
    rng = np.random.default_rng(99)
    v, nA, nU, k = 25, 333, 401, 7
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.05)
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    masks = orc.fold_masks_from_assignment(fold, k)
    for order in (2, 3, 4, 5):
        combs = np.array([sorted(rng.choice(v, size=order, replace=False)) for _ in range(40 if order < 4 else 11)], np.int32)
        aff, unaff = eng.epi_counts(combs)
        faff, funaff = eng.epi_counts(combs, all_folds=True)
        for n, comb in enumerate(combs):
            rows = [data[c] for c in comb]
            ea, eu = orc.epi_counts(rows, nA, nU)
            assert np.array_equal(aff[n], ea) and np.array_equal(unaff[n], eu)
            fa, fu = orc.epi_counts_all_folds(rows, nA, nU, masks)
            assert np.array_equal(faff[:, n, :], fa) and np.array_equal(funaff[:, n, :], fu)


def test_ranking_is_the_top_of_the_dense_scan(eng):
    rng = np.random.default_rng(17)
    v, nA, nU, k, n = 150, 180, 220, 5, 12
    data = epi_random_dataset(rng, v, nA, nU)
    # plant an interaction so the best models are not all ties
    data[7, :nA] = rng.choice([1, 2], size=nA); data[91, :nA] = rng.choice([1, 2], size=nA)
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    acc, rm = eng.epi_scan_pairs(hpgv.EPI_TESTING)
    res = eng.epi_rank_pairs(hpgv.EPI_TESTING, n)
    pairs = [(i, j) for i in range(v) for j in range(i + 1, v)]
    for f in range(k):
        a = np.where(np.isnan(acc[f]), -np.inf, acc[f])
        order = sorted(range(len(pairs)), key=lambda p: (-a[p], pairs[p]))[:n]
        assert res["n"][f] == n
        assert [(int(x), int(y)) for x, y in zip(res["i"][f], res["j"][f])] == [pairs[p] for p in order]
        assert np.array_equal(res["accuracy"][f], acc[f][order]) and np.array_equal(res["risky"][f], rm[f][order])
    assert (7, 91) == (int(res["i"][0][0]), int(res["j"][0][0]))
    # row bands (the multi-GPU unit of work, hpg-variant_amd/sharding.py pair_row_range): the merged band lists are the ranking
    from importlib import import_module
    sh = import_module("hpg-variant_amd.sharding")
    for world in (2, 3):
        parts = [eng.epi_rank_pairs(hpgv.EPI_TESTING, n, rows=sh.pair_row_range(g, world, v)) for g in range(world)]
        for f in range(k):
            merged = sorted(((-float(p["accuracy"][f][e]), int(p["i"][f][e]), int(p["j"][f][e])) for p in parts for e in range(p["n"][f])))[:n]
            assert [(i_, j_) for _, i_, j_ in merged] == [(int(x), int(y)) for x, y in zip(res["i"][f], res["j"][f])]


@pytest.mark.parametrize("nA,nU,k", [(180, 220, 5), (200, 200, 10), (64, 64, 2), (130, 127, 7)])
def test_ranking_with_every_model_kept_is_the_dense_scan(eng, nA, nU, k):
    # the ranking mode evaluates on packed 16-bit pairs and forms the high-risk mask only for kept models: with every
    # model kept, accuracies and masks of all pairs (and of all triples) must be those of the dense scan, both subsets
    rng = np.random.default_rng(nA + 7 * k)
    v = 36
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.03)
    data[5, :nA] = rng.choice([1, 2], size=nA); data[20, :nA] = rng.choice([1, 2], size=nA)
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    pairs = [(i, j) for i in range(v) for j in range(i + 1, v)]
    triples = [(a, b, c) for a in range(v) for b in range(a + 1, v) for c in range(b + 1, v)]
    for subset in (hpgv.EPI_TESTING, hpgv.EPI_TRAINING):
        acc, rm = eng.epi_scan_pairs(subset)
        res = eng.epi_rank_pairs(subset, len(pairs))
        for f in range(k):
            a = np.where(np.isnan(acc[f]), -np.inf, acc[f])
            order = [p for p in sorted(range(len(pairs)), key=lambda p: (-a[p], pairs[p])) if a[p] > -np.inf]
            n = len(order)                                            # (a fold without cases or without controls ranks nothing)
            assert res["n"][f] == n
            assert [(int(x), int(y)) for x, y in zip(res["i"][f][:n], res["j"][f][:n])] == [pairs[p] for p in order]
            assert np.array_equal(res["accuracy"][f][:n], acc[f][order]) and np.array_equal(res["risky"][f][:n], rm[f][order])
        acc3, rm3 = eng.epi_scan_triples(subset)
        res3 = eng.epi_rank_triples(subset, len(triples))
        for f in range(k):
            vals = np.array([acc3[f][t] for t in triples])
            vals = np.where(np.isnan(vals), -np.inf, vals)
            order = [p for p in sorted(range(len(triples)), key=lambda p: (-vals[p], triples[p])) if vals[p] > -np.inf]
            n = len(order)
            assert res3["n"][f] == n
            assert [(int(a_), int(b_), int(c_)) for a_, b_, c_ in zip(res3["i"][f][:n], res3["j"][f][:n], res3["k"][f][:n])] == [triples[p] for p in order]
            assert np.array_equal(res3["accuracy"][f][:n], np.array([acc3[f][triples[p]] for p in order]))
            assert np.array_equal(res3["risky"][f][:n], np.array([rm3[f][triples[p]] for p in order], np.uint32))


@pytest.mark.parametrize("v,nA,nU,k,p_missing", [(300, 2500, 1700, 3, 0.05), (200, 900, 900, 16, 0.02), (131, 1030, 1030, 10, 0.0),
                                                  (97, 40, 3000, 2, 0.1), (260, 5000, 5000, 10, 0.01), (70, 129, 127, 12, 0.12)])
def test_matrix_core_ranking_is_the_vector_alu_ranking(eng, v, nA, nU, k, p_missing):
    # k_epi_pairs_mfma (cell counts as FP4 MFMAs, two passes) against k_epi_pairs (popcounts, one pass): several column
    # tiles and row blocks, blocks on the diagonal, groups longer and shorter than a staging chunk, up to 16 folds, classes of
    # equal and of unequal size, data with many, few and no missing calls; both subsets; a short list and every model
    rng = np.random.default_rng(v + nA + 3 * k)
    data = epi_random_dataset(rng, v, nA, nU, p_missing=p_missing)
    data[7, :nA] = rng.choice([1, 2], size=nA); data[v - 3, :nA] = rng.choice([1, 2], size=nA)
    data[11] = 1                                                     # a monomorphic SNP: empty cells everywhere
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    try:
        for subset in (hpgv.EPI_TESTING, hpgv.EPI_TRAINING):
            for n in (25, v * (v - 1) // 2):
                res = {}
                for mfma in (1, 0):
                    eng.set_option("epi_pairs_mfma", mfma)
                    res[mfma] = eng.epi_rank_pairs(subset, n)
                    # the scan that ran, as the library reports it: the two sides are two different kernels
                    assert eng.epi_last_rank_info()["kernel"] == (hpgv.EPI_KERNEL_PAIRS_MFMA if mfma else hpgv.EPI_KERNEL_PAIRS_VALU)
                for f in range(k):
                    m = int(res[0]["n"][f])
                    assert int(res[1]["n"][f]) == m and m > 0
                    for key in ("i", "j", "accuracy", "risky"):
                        assert np.array_equal(res[1][key][f][:m], res[0][key][f][:m]), (key, f, subset, n)
    finally:
        eng.set_option("epi_pairs_mfma", 1)


@pytest.mark.parametrize("v,nA,nU,k,p_missing", [(70, 700, 500, 3, 0.05), (40, 900, 900, 10, 0.02), (66, 260, 260, 5, 0.0), (33, 40, 1500, 2, 0.1), (38, 640, 700, 13, 0.03), (30, 800, 800, 16, 0.02)])
def test_matrix_core_triple_ranking_is_the_vector_alu_ranking(eng, v, nA, nU, k, p_missing):
    # k_epi_triples_mfma against k_epi_triples3 / k_epi_triples: blocks of 16 second SNPs on and off the diagonals, third SNPs
    # in one and in two tiles of 64, groups longer and shorter than a staging chunk, equal and unequal classes; both subsets; a
    # short list and every model
    rng = np.random.default_rng(v + nA + 3 * k)
    data = epi_random_dataset(rng, v, nA, nU, p_missing=p_missing)
    data[2, :nA] = rng.choice([1, 2], size=nA); data[v // 2, :nA] = rng.choice([1, 2], size=nA); data[v - 2, :nA] = rng.choice([1, 2], size=nA)
    data[5] = 1                                                      # a monomorphic SNP: empty cells everywhere
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    try:
        for subset in (hpgv.EPI_TESTING, hpgv.EPI_TRAINING):
            for n in (25, v * (v - 1) * (v - 2) // 6):
                res = {}
                for mfma in (1, 0):
                    eng.set_option("epi_triples_mfma", mfma)
                    res[mfma] = eng.epi_rank_triples(subset, n)
                    assert eng.epi_last_rank_info()["kernel"] == (hpgv.EPI_KERNEL_TRIPLES_MFMA if mfma else
                                                                  hpgv.EPI_KERNEL_TRIPLES3 if k <= 10 else hpgv.EPI_KERNEL_TRIPLES)
                for f in range(k):
                    m = int(res[0]["n"][f])
                    assert int(res[1]["n"][f]) == m and m > 0
                    for key in ("i", "j", "k", "accuracy", "risky"):
                        assert np.array_equal(res[1][key][f][:m], res[0][key][f][:m]), (key, f, subset, n)
    finally:
        eng.set_option("epi_triples_mfma", 1)


def test_epistasis_error_paths(eng):
    e = hpgv.Engine(0)
    with pytest.raises(hpgv.HpgvError):
        e.L.hpgv_epi_set_folds.argtypes  # noqa: B018  (keeps the symbol referenced)
        e._chk(e.L.hpgv_epi_set_folds(e.h, None, 2))                  # no dataset yet
    data = np.zeros((4, 10), np.uint8)
    e.epi_set_dataset(data, 5, 5)
    with pytest.raises(hpgv.HpgvError):
        e.epi_set_folds(np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 9], np.int32), 5)   # fold id out of range
    with pytest.raises(hpgv.HpgvError):
        e.epi_set_folds(np.zeros(10, np.int32), 17)                  # more folds than supported
    with pytest.raises(hpgv.HpgvError):
        e.epi_counts(np.array([[0, 4]], np.int32))                   # SNP index outside the dataset
    e.close()


def test_run_epistasis_from_a_dataset_file(tmp_path):
    """hpgv_run_epistasis (run_epistasis, singlenode/epistasis_runner.c): dataset file in, report out; the expected
    report is rebuilt from the oracle's scan with the same folds (same rand() stream)."""
    import ctypes as C
    import struct
    from importlib import import_module
    b = import_module("hpg-variant_amd._build")
    L = C.CDLL(b.HOSTLIB)
    L.get_k_folds.restype = C.POINTER(C.POINTER(C.c_int))
    L.get_k_folds.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.POINTER(C.c_uint))]
    L.hpgv_run_epistasis.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
    L.hpgv_host_last_error.restype = C.c_char_p
    libc = C.CDLL(None)
    assert L.hpgv_host_init(0) == 0          # the engine bound BEFORE the seeds below: the runtime's start-up may draw from rand()
    rng = np.random.default_rng(23)
    v, nA, nU, k, n, reps = 45, 90, 110, 5, 8, 2
    data = epi_random_dataset(rng, v, nA, nU)
    data[3, :nA] = rng.choice([1, 2], size=nA); data[30, :nA] = rng.choice([1, 2], size=nA)
    path = tmp_path / "epi.bin"
    with open(path, "wb") as f:                                      # dataset.c:63-76
        f.write(struct.pack("<III", v, nA, nU)); f.write(data.tobytes())
    # the folds the run will deal: same seed, same calls
    libc.srand(777)
    folds_per_rep = []
    for _ in range(reps):
        sizes = C.POINTER(C.c_uint)()
        folds = L.get_k_folds(nA, nU, k, C.byref(sizes))
        fold_of = np.empty(nA + nU, np.int32)
        for f in range(k):
            for j in range(sizes[3 * f]):
                fold_of[folds[f][j]] = f
        folds_per_rep.append(fold_of)
    pairs = [(i, j) for i in range(v) for j in range(i + 1, v)]
    for mode in (1, 0):
        libc.srand(777)
        prefix = str(tmp_path / ("out%d" % mode))
        rc = L.hpgv_run_epistasis(str(path).encode(), k, reps, n, hpgv.EPI_TESTING, mode, prefix.encode())
        assert rc == 0, L.hpgv_host_last_error()
        for r in range(reps):
            masks = orc.fold_masks_from_assignment(folds_per_rep[r], k)
            acc, rm = orc.epi_scan_pairs(data, nA, nU, masks, 0)
            merged = {}
            for f in range(k):
                a = np.where(np.isnan(acc[f]), -np.inf, acc[f])
                for p in sorted(range(len(pairs)), key=lambda q: (-a[q], pairs[q]))[:n]:
                    e = merged.setdefault(pairs[p], [0.0, 0, int(rm[f][p])])
                    e[0] += acc[f][p]; e[1] += 1
            rows = [(pr, s / k, c, m) for pr, (s, c, m) in merged.items()]
            rows.sort(key=(lambda t: (-t[1], t[0])) if mode == 1 else (lambda t: (-t[2], -t[1], t[0])))
            lines = open("%s.cv%d.epi" % (prefix, r + 1)).read().splitlines()
            assert lines[0] == "#CROSS VALIDATION %d" % (r + 1) and lines[1] == "#COMBINATIONS OF: 2 SNPs"
            assert lines[2] == ("#EVALUATION MODE: Cross-validation accuracy" if mode == 1 else "#EVALUATION MODE: Cross-validation consistency")
            assert lines[3] == "#EVALUATION PARTITION: Testing" and lines[4] == "#POSITION\tSNPs\tGENOTYPES\tCV-C\tCV-A"
            body = lines[5:]
            assert len(body) == min(n, len(rows))
            for pos, (line, (pr, a, c, m)) in enumerate(zip(body, rows)):
                gts = "".join("(%d-%d), " % (cell // 3, cell % 3) for cell in range(9) if m >> cell & 1)
                assert line == "%d\t( %d, %d )\t%s%d\t%.3f" % (pos + 1, pr[0], pr[1], gts, c, a), (mode, r, pos)
            assert rows[0][0] == (3, 30)                             # the planted interaction wins


@pytest.mark.parametrize("v,nA,nU,k", [(14, 60, 75, 4), (9, 32, 32, 2), (20, 210, 180, 10), (70, 40, 50, 3)])
def test_triple_scan_matches_the_oracle(eng, v, nA, nU, k):
    # order 3 (27 cells): every triple of a small set against the oracle's model, both evaluation subsets
    rng = np.random.default_rng(v + k)
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.04)
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    masks = orc.fold_masks_from_assignment(fold, k)
    triples = [(a, b, c) for a in range(v) for b in range(a + 1, v) for c in range(b + 1, v)]
    if len(triples) > 600:
        triples = [triples[t] for t in rng.choice(len(triples), 600, replace=False)]
    for subset in (hpgv.EPI_TESTING, hpgv.EPI_TRAINING):
        acc, rm = eng.epi_scan_triples(subset)
        assert np.isnan(acc[:, 3, 2, 5]).all() and np.isnan(acc[:, 1, 1, 2]).all()       # not a triple i < j < k
        for (a, b, c) in triples:
            ea, em, _ = orc.epi_model([data[a], data[b], data[c]], nA, nU, masks, subset)
            assert np.array_equal(rm[:, a, b, c], em), (a, b, c)
            got = acc[:, a, b, c]
            assert np.all((got == ea) | (np.isnan(got) & np.isnan(ea))), (a, b, c, got, ea)


def test_triple_ranking_is_the_top_of_the_dense_scan(eng):
    rng = np.random.default_rng(303)
    v, nA, nU, k, n = 40, 150, 170, 5, 9
    data = epi_random_dataset(rng, v, nA, nU)
    for s in (4, 17, 33):                                            # a planted three-way signal
        data[s, :nA] = rng.choice([1, 2], size=nA)
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    acc, rm = eng.epi_scan_triples(hpgv.EPI_TESTING)
    res = eng.epi_rank_triples(hpgv.EPI_TESTING, n)
    triples = [(a, b, c) for a in range(v) for b in range(a + 1, v) for c in range(b + 1, v)]
    for f in range(k):
        vals = np.array([acc[f][t] for t in triples])
        vals = np.where(np.isnan(vals), -np.inf, vals)
        order = sorted(range(len(triples)), key=lambda p: (-vals[p], triples[p]))[:n]
        assert res["n"][f] == n
        assert [(int(a), int(b), int(c)) for a, b, c in zip(res["i"][f], res["j"][f], res["k"][f])] == [triples[p] for p in order]
        assert np.array_equal(res["accuracy"][f], np.array([acc[f][triples[p]] for p in order]))
        assert np.array_equal(res["risky"][f], np.array([rm[f][triples[p]] for p in order], np.uint32))
    assert (4, 17, 33) == (int(res["i"][0][0]), int(res["j"][0][0]), int(res["k"][0][0]))


def test_run_epistasis_order_3_report(tmp_path):
    import ctypes as C
    import struct
    from importlib import import_module
    b = import_module("hpg-variant_amd._build")
    L = C.CDLL(b.HOSTLIB)
    L.hpgv_run_epistasis_order.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
    L.hpgv_host_last_error.restype = C.c_char_p
    rng = np.random.default_rng(41)
    v, nA, nU = 24, 120, 130
    data = epi_random_dataset(rng, v, nA, nU)
    for s_ in (2, 9, 20):
        data[s_, :nA] = rng.choice([1, 2], size=nA)
    path = tmp_path / "epi3.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<III", v, nA, nU)); f.write(data.tobytes())
    prefix = str(tmp_path / "o3")
    rc = L.hpgv_run_epistasis_order(str(path).encode(), 3, 4, 1, 6, hpgv.EPI_TRAINING, 1, prefix.encode())
    assert rc == 0, L.hpgv_host_last_error()
    lines = open(prefix + ".cv1.epi").read().splitlines()
    assert lines[1] == "#COMBINATIONS OF: 3 SNPs" and lines[3] == "#EVALUATION PARTITION: Training"
    first = lines[5].split("\t")
    # epistasis_report.c:62-77: position, "( i, j, k )", then the risky cells "(a-b, c), " run straight into the CV-c count
    assert first[0] == "1" and first[1] == "( 2, 9, 20 )" and first[2].startswith("(")
    genos, count = first[2].rsplit("), ", 1)
    cells = genos.split("), ")
    assert count == "4" and all(len(c.strip("()").replace("-", ",").replace(" ", "").split(",")) == 3 for c in cells)
    assert "(1-1, 1)" in first[2] and "(2-2, 2)" in first[2] and "(0-" not in first[2]      # the planted carriers
    assert L.hpgv_run_epistasis_order(str(path).encode(), 6, 4, 1, 6, 0, 1, prefix.encode()) != 0      # order 6: refused (2 to 5)


@pytest.mark.parametrize("nA,nU,k", [(20, 2, 4), (2, 21, 4), (3, 3, 3), (1, 40, 2)])
def test_folds_that_lack_a_class(eng, nA, nU, k):
    # fewer cases (or controls) than folds: some folds hold one class only; sizes of zero give 0/0 = NaN accuracies exactly
    # where the reference's division does
    rng = np.random.default_rng(nA * 31 + nU)
    v = 12
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.05)
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    masks = orc.fold_masks_from_assignment(fold, k)
    for subset in (hpgv.EPI_TESTING, hpgv.EPI_TRAINING):
        acc, rm = eng.epi_scan_pairs(subset)
        eacc, erm = orc.epi_scan_pairs(data, nA, nU, masks, subset)
        assert np.array_equal(rm, erm.astype(np.uint16)) and _same(acc, eacc)
        acc3, rm3 = eng.epi_scan_triples(subset)
        for (a, b, c) in [(0, 1, 2), (0, 5, 11), (3, 4, 9), (9, 10, 11), (2, 7, 8)]:
            ea, em, _ = orc.epi_model([data[a], data[b], data[c]], nA, nU, masks, subset)
            assert np.array_equal(rm3[:, a, b, c], em), (a, b, c)
            got = acc3[:, a, b, c]
            assert np.all((got == ea) | (np.isnan(got) & np.isnan(ea))), (a, b, c, got, ea)


def test_random_cohorts_through_every_scan(eng):
    # cohorts drawn at random (HPGV_SOAK_SHAPES of them: 3 in the suite): SNP counts, class sizes equal and unequal, 1 to 16 folds --
    # the scans are instantiated per fold count and per "classes are equal", and the dispatch picks by both
    import os
    rng = np.random.default_rng(int(os.environ.get("HPGV_FUZZ_SEED", "82")))
    for _ in range(int(os.environ.get("HPGV_SOAK_SHAPES", "3"))):
        k = int(rng.integers(1, 17))
        nA = int(rng.choice([int(rng.integers(k, 60)), int(rng.integers(60, 700)), int(rng.integers(700, 1500))]))
        nU = nA if rng.random() < 0.4 else int(max(k, nA * rng.uniform(0.3, 2.5)))
        test_pair_scan_matches_the_oracle(eng, int(rng.integers(3, 90)), nA, nU, k)
        test_pair_scan_on_a_dataset_without_missing_calls(eng, int(rng.integers(34, 80)), nA, nU, k)
        test_triple_scan_matches_the_oracle(eng, int(rng.integers(6, 24)), nA, nU, k)
        test_ranking_with_every_model_kept_is_the_dense_scan(eng, min(nA, 400), min(nU, 400), min(k, 10))


# ---- any order the reference's --order takes (2 to 5): the listed-combination kernel, one lane per cell ---------------------

@pytest.mark.parametrize("order,v,nA,nU,k", [(2, 14, 120, 150, 5), (3, 11, 97, 64, 4), (4, 9, 210, 190, 10), (5, 8, 130, 310, 3),
                                             (4, 7, 33, 1200, 16), (5, 7, 500, 500, 1)])
def test_listed_combinations_of_any_order_match_the_oracle(eng, order, v, nA, nU, k):
    import itertools
    rng = np.random.default_rng(1000 * order + v)
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.03)
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    masks = orc.fold_masks_from_assignment(fold, k)
    combs = np.array(list(itertools.combinations(range(v), order)), np.int32)
    if len(combs) > 60:
        combs = combs[np.sort(rng.choice(len(combs), 60, replace=False))]
    for subset in (hpgv.EPI_TESTING, hpgv.EPI_TRAINING):
        acc, mask = eng.epi_eval_combs(combs, subset)
        for n, comb in enumerate(combs):
            ea, em, _ = orc.epi_model_wide([data[c] for c in comb], nA, nU, masks, subset)
            assert _same(acc[n], ea), (comb, subset, acc[n], ea)
            assert np.array_equal(mask[n], em), (comb, subset)


def test_listed_combinations_agree_with_the_pair_and_triple_scans(eng):
    # two implementations of orders 2 and 3: the tile scans and the one-lane-per-cell kernel
    import itertools
    rng = np.random.default_rng(5)
    v, nA, nU, k = 40, 700, 650, 6
    data = epi_random_dataset(rng, v, nA, nU)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(epi_random_folds(rng, nA, nU, k), k)
    for subset in (hpgv.EPI_TESTING, hpgv.EPI_TRAINING):
        pa, pm = eng.epi_scan_pairs(subset)
        pairs = np.array(list(itertools.combinations(range(v), 2)), np.int32)
        acc, mask = eng.epi_eval_combs(pairs, subset)
        assert _same(acc.T, pa) and np.array_equal(mask[:, :, 0].T, pm.astype(np.uint32)) and not mask[:, :, 1:].any()
        ta, tm = eng.epi_scan_triples(subset)
        triples = np.array(list(itertools.combinations(range(v), 3)), np.int32)
        acc, mask = eng.epi_eval_combs(triples, subset)
        assert _same(acc.T, ta[:, triples[:, 0], triples[:, 1], triples[:, 2]])
        assert np.array_equal(mask[:, :, 0].T, tm[:, triples[:, 0], triples[:, 1], triples[:, 2]])


def _rank_from_dense(acc, combs, n):
    """per fold the best n of a dense evaluation (folds x combos), ties to the smaller combination (= the listing order)"""
    out = []
    for f in range(acc.shape[0]):
        ok = np.flatnonzero(~np.isnan(acc[f]))
        order = ok[np.lexsort((ok, -acc[f][ok]))][:n]
        out.append(order)
    return out


@pytest.mark.parametrize("order,v", [(4, 13), (5, 11), (2, 30)])
def test_ranking_of_any_order_is_the_top_of_the_dense_evaluation(eng, order, v):
    import itertools
    rng = np.random.default_rng(order * 31 + v)
    nA, nU, k, n = 150, 170, 5, 9
    data = epi_random_dataset(rng, v, nA, nU)
    carriers = rng.choice(v, size=order, replace=False)
    data[np.ix_(carriers, np.arange(nA))] = rng.choice([1, 2], size=(order, nA))         # a planted model: the cases carry the variants
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(epi_random_folds(rng, nA, nU, k), k)
    combs = np.array(list(itertools.combinations(range(v), order)), np.int32)
    for subset in (hpgv.EPI_TESTING, hpgv.EPI_TRAINING):
        acc, mask = eng.epi_eval_combs(combs, subset)
        res = eng.epi_rank_order(order, subset, n)
        best = _rank_from_dense(acc.T, combs, n)
        for f in range(k):
            assert res["n"][f] == len(best[f])
            assert np.array_equal(res["combs"][f][: len(best[f])], combs[best[f]])
            assert _same(res["accuracy"][f][: len(best[f])], acc[best[f], f])
            assert np.array_equal(res["risky"][f][: len(best[f])], mask[best[f], f])
        # the first SNPs dealt to three "devices": the shares' lists merge into the same ranking
        parts = [eng.epi_rank_order(order, subset, n, rows=r) for r in ((0, 2), (2, 5), (5, v))]
        for f in range(k):
            cand = [(-p["accuracy"][f][e], tuple(p["combs"][f][e])) for p in parts for e in range(p["n"][f])]
            cand.sort()
            assert [c[1] for c in cand[:n]] == [tuple(c) for c in res["combs"][f][: res["n"][f]]]
    if order == 2:                                                   # ... and the pair scan's own ranking
        rp = eng.epi_rank_pairs(hpgv.EPI_TRAINING, n)
        for f in range(k):
            assert np.array_equal(rp["i"][f], res["combs"][f][:, 0]) and np.array_equal(rp["j"][f], res["combs"][f][:, 1])
            assert _same(rp["accuracy"][f], res["accuracy"][f]) and np.array_equal(rp["risky"][f], res["risky"][f][:, 0])


def test_any_order_error_paths(eng):
    data = np.zeros((6, 10), np.uint8)
    eng.epi_set_dataset(data, 5, 5)
    with pytest.raises(hpgv.HpgvError):
        eng.epi_eval_combs(np.zeros((1, 6), np.int32), hpgv.EPI_TESTING)          # order 6
    with pytest.raises(hpgv.HpgvError):
        eng.epi_eval_combs(np.array([[0, 1, 2, 9]], np.int32), hpgv.EPI_TESTING)   # SNP outside the dataset
    with pytest.raises(hpgv.HpgvError):
        eng.epi_rank_order(4, 7, 3)                                                # no such subset
    res = eng.epi_rank_order(5, hpgv.EPI_TESTING, 4, rows=(3, 6))                  # no combination of 5 starts at SNP 3 of 6
    assert res["n"].tolist() == [0]


def test_run_epistasis_order_4_report(tmp_path):
    import ctypes as C
    import struct
    from importlib import import_module
    b = import_module("hpg-variant_amd._build")
    L = C.CDLL(b.HOSTLIB)
    L.hpgv_run_epistasis_order.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
    L.hpgv_host_last_error.restype = C.c_char_p
    rng = np.random.default_rng(44)
    v, nA, nU = 12, 140, 150
    data = epi_random_dataset(rng, v, nA, nU)
    for s_ in (1, 4, 6, 10):
        data[s_, :nA] = rng.choice([1, 2], size=nA)
    path = tmp_path / "epi4.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<III", v, nA, nU)); f.write(data.tobytes())
    prefix = str(tmp_path / "o4")
    rc = L.hpgv_run_epistasis_order(str(path).encode(), 4, 4, 1, 5, hpgv.EPI_TRAINING, 1, prefix.encode())
    assert rc == 0, L.hpgv_host_last_error()
    lines = open(prefix + ".cv1.epi").read().splitlines()
    assert lines[1] == "#COMBINATIONS OF: 4 SNPs"
    first = lines[5].split("\t")
    # epistasis_report.c:62-77 for order 4: "( i, j, k, l )" and cells "(a-b, c, d), "
    assert first[0] == "1" and first[1] == "( 1, 4, 6, 10 )"
    genos, count = first[2].rsplit("), ", 1)
    assert count == "4" and "(1-1, 1, 1)" in first[2] and "(2-2, 2, 2)" in first[2] and "(0-" not in first[2]
    assert all(len(c.strip("()").replace("-", ",").replace(" ", "").split(",")) == 4 for c in genos.split("), "))
