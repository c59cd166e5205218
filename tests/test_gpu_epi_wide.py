"""The wide form of the epistasis scans (option "epi_wide", k_epi_combs_wide): more than 16 folds, (fold, class) groups and
classes of 65 536 samples or more.  Every expectation comes from the CPU oracle (its counts are plain ints and it takes up to 64
folds), never from another GPU kernel.  Combinations, accuracies (exact doubles), risky masks and list lengths are compared with
==; every ranking call's kernel is the one hpgv_epi_last_rank_info reports."""
import numpy as np
import pytest

from helpers import all_combs, epi_random_dataset, epi_random_folds, hpgv, oracle_top
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

SUBSETS = (hpgv.EPI_TESTING, hpgv.EPI_TRAINING)
ORDERS = (2, 3, 4, 5)
WIDE = hpgv.EPI_KERNEL_COMBS_WIDE


@pytest.fixture(scope="module")
def eng():
    e = hpgv.Engine(0)
    e.set_option("epi_wide", 1)
    yield e
    e.close()


def _same(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _models(data, nA, nU, masks, subset, order):
    """the oracle's model of every combination of `order` SNPs: combs, accuracy (folds x combs), masks (folds x combs x 8)"""
    combs = all_combs(data.shape[0], order)
    k = masks.shape[0]
    acc, rm = np.zeros((k, len(combs))), np.zeros((k, len(combs), 8), np.uint32)
    for c, comb in enumerate(combs):
        a, m, _ = orc.epi_model_wide([data[s] for s in comb], nA, nU, masks, subset)
        acc[:, c], rm[:, c] = a, m
    return combs, acc, rm


def _check_rank_order(eng, order, subset, N, combs, acc, rm, kernel, what):
    """hpgv_epi_rank_order against the top of the oracle's models: NaN accuracies rank nowhere, ties go by the combination (the
    models are listed in lexicographic order: a stable sort by accuracy)"""
    res = eng.epi_rank_order(order, subset, N)
    info = eng.epi_last_rank_info()
    assert info["kernel"] == kernel, (what, info)
    for f in range(acc.shape[0]):
        ok = np.flatnonzero(~np.isnan(acc[f]))
        best = ok[np.argsort(-acc[f][ok], kind="stable")[:N]]
        n = len(best)
        assert int(res["n"][f]) == n, (what, f, int(res["n"][f]), n)
        assert np.array_equal(res["combs"][f][:n], combs[best]), (what, f)
        assert np.array_equal(res["accuracy"][f][:n], acc[f][best]), (what, f)
        assert np.array_equal(res["risky"][f][:n], rm[f][best]), (what, f)
    return info


def _check_tile_ranking(eng, order, subset, N, exp_scan, kernel, what):
    """hpgv_epi_rank_pairs / _triples against the top of the oracle's dense scan"""
    res = eng.epi_rank_pairs(subset, N) if order == 2 else eng.epi_rank_triples(subset, N)
    info = eng.epi_last_rank_info()
    assert info["kernel"] == kernel, (what, info)
    exp = oracle_top(*exp_scan, N)
    for f in range(len(exp["n"])):
        n = int(exp["n"][f])
        assert int(res["n"][f]) == n, (what, f, int(res["n"][f]), n)
        for key in tuple("ijk"[:order]) + ("accuracy", "risky"):
            assert np.array_equal(res[key][f][:n], exp[key][f][:n]), (what, f, key)
    return info


def _check_everything(eng, data, nA, nU, masks, pairs_kernel, triples_kernel, order_kernel, what):
    """rank_order at orders 2 to 5, rank_pairs and rank_triples, both subsets, N = 3 and N = every model"""
    v = data.shape[0]
    for subset in SUBSETS:
        for order in ORDERS:
            combs, acc, rm = _models(data, nA, nU, masks, subset, order)
            for N in (3, len(combs)):
                _check_rank_order(eng, order, subset, N, combs, acc, rm, order_kernel, (what, "order", order, subset, N))
        scan2 = orc.epi_scan_pairs(data, nA, nU, masks, subset) + (all_combs(v, 2),)
        scan3 = orc.epi_scan_triples(data, nA, nU, masks, subset) + (all_combs(v, 3),)
        for N in (3, len(scan3[2])):
            _check_tile_ranking(eng, 2, subset, min(N, len(scan2[2])), scan2, pairs_kernel, (what, "pairs", subset, N))
            _check_tile_ranking(eng, 3, subset, N, scan3, triples_kernel, (what, "triples", subset, N))


# ---- 1. many folds -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nA,nU,k", [(200, 170, 17), (200, 170, 33), (90, 70, 64), (40, 20, 33)])
def test_many_folds(eng, nA, nU, k):
    # (40, 20, 33): 13 folds hold no control (and 26 a single case): testing accuracies of 0/0 are NaN and never ranked, the
    # contract of test_ranking_on_folds_that_lack_a_class
    rng = np.random.default_rng(nA * 7 + nU + k)
    data = epi_random_dataset(rng, 8, nA, nU, p_missing=0.02)
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    masks = orc.fold_masks_from_assignment(fold, k)
    if nU < k:
        assert np.isnan(orc.epi_scan_pairs(data, nA, nU, masks, hpgv.EPI_TESTING)[0]).any()
    _check_everything(eng, data, nA, nU, masks, WIDE, WIDE, WIDE, (nA, nU, k))


# ---- 2. large classes --------------------------------------------------------------------------------------------------------

def _large_cohort(nA, nU, k):
    """V = 6 with the carry cases planted: the first 65 536 cases have genotype 0 at SNPs 0 and 1, every other case genotype 1 at
    SNP 0 -- cell (0, 0) of pair (0, 1) holds exactly 65 536 cases (the low 16 bits of that count are zero).  The same cases have
    genotype 0 at SNP 2: cell (0, 0) of pair (1, 2) holds them and some of the others, a count past 65 535 with low bits set"""
    rng = np.random.default_rng(nA + nU + k)
    data = epi_random_dataset(rng, 6, nA, nU, p_missing=0.02)
    data[0, :65536] = 0
    data[1, :65536] = 0
    data[0, 65536:nA] = 1
    data[2, :65536] = 0
    fold = epi_random_folds(rng, nA, nU, k)
    return data, fold, orc.fold_masks_from_assignment(fold, k)


@pytest.mark.parametrize("nA,nU,k,pairs_kernel", [
    (65600, 300, 1, WIDE),                                           # one group of 65 600: the implicit single fold of set_dataset
    (140000, 300, 2, WIDE),                                          # groups of 70 000
    (70000, 66000, 2, hpgv.EPI_KERNEL_PAIRS_VALU),                   # classes above 65 535 in groups below: the pair scan stays
])
def test_large_classes(eng, nA, nU, k, pairs_kernel):
    data, fold, masks = _large_cohort(nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    if k > 1:
        eng.epi_set_folds(fold, k)
    aff, unaff = eng.epi_counts([[0, 1], [1, 2]])
    ea, eu = orc.epi_counts([data[0], data[1]], nA, nU)
    assert int(ea[0]) == 65536 and int(aff[0][0]) == 65536
    assert np.array_equal(aff[0], ea) and np.array_equal(unaff[0], eu)
    ea, eu = orc.epi_counts([data[1], data[2]], nA, nU)
    assert int(ea[0]) > 65536 and np.array_equal(aff[1], ea) and np.array_equal(unaff[1], eu)
    _check_everything(eng, data, nA, nU, masks, pairs_kernel, WIDE, WIDE, (nA, nU, k))


# ---- 3. the same answers where both kernels work -----------------------------------------------------------------------------

def test_wide_and_packed_kernels_both_match_the_oracle(eng):
    rng = np.random.default_rng(3)
    v, nA, nU, k = 10, 300, 260, 10
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.02)
    fold = epi_random_folds(rng, nA, nU, k)
    masks = orc.fold_masks_from_assignment(fold, k)
    try:
        eng.set_option("epi_wide", 2)
        eng.epi_set_dataset(data, nA, nU)
        eng.epi_set_folds(fold, k)
        got = {}
        for wide in (2, 0):
            eng.set_option("epi_wide", wide)
            for subset in SUBSETS:
                for order in ORDERS:
                    got[wide, subset, order] = eng.epi_eval_combs(all_combs(v, order), subset)
            eng.epi_rank_order(4, hpgv.EPI_TESTING, 3)
            assert eng.epi_last_rank_info()["kernel"] == (WIDE if wide else hpgv.EPI_KERNEL_COMBS)
    finally:
        eng.set_option("epi_wide", 1)
    for subset in SUBSETS:
        for order in ORDERS:
            _, acc, rm = _models(data, nA, nU, masks, subset, order)
            for wide in (2, 0):
                g_acc, g_rm = got[wide, subset, order]
                assert _same(g_acc.T, acc), (wide, subset, order)
                assert np.array_equal(g_rm.transpose(1, 0, 2), rm), (wide, subset, order)


# ---- 4. counts ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nA,nU,k", [(200, 170, 17), (140000, 300, 2)])
def test_counts_of_wide_layouts(eng, nA, nU, k):
    if nA > 65535:
        data, fold, masks = _large_cohort(nA, nU, k)
    else:
        rng = np.random.default_rng(44)
        data = epi_random_dataset(rng, 6, nA, nU, p_missing=0.02)
        fold = epi_random_folds(rng, nA, nU, k)
        masks = orc.fold_masks_from_assignment(fold, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    for order in ORDERS:
        combs = all_combs(6, order)[::3]
        aff, unaff = eng.epi_counts(combs)
        aff_f, unaff_f = eng.epi_counts(combs, all_folds=True)
        for c, comb in enumerate(combs):
            rows = [data[s] for s in comb]
            ea, eu = orc.epi_counts(rows, nA, nU)
            assert np.array_equal(aff[c], ea) and np.array_equal(unaff[c], eu), (order, comb)
            ea, eu = orc.epi_counts_all_folds(rows, nA, nU, masks)
            assert np.array_equal(aff_f[:, c], ea) and np.array_equal(unaff_f[:, c], eu), (order, comb)


# ---- 5. several launches with thresholds -------------------------------------------------------------------------------------

def test_several_launches_with_thresholds(eng):
    """V = 40, order 3, 17 folds: 9 880 triples.  The any-order ranking lists max(4 096, 4 N) combinations in its first launch and
    up to 131 072 in each one after, so these calls take TWO launches (4 096 + 5 784), the second against the thresholds the
    first left (two, not three or more: the list limits are EpiListOrder's, the same for the packed and the wide kernel)."""
    rng = np.random.default_rng(17)
    v, nA, nU, k = 40, 120, 100, 17
    data = epi_random_dataset(rng, v, nA, nU, p_missing=0.02)
    for s in (6, 22, 35):                                            # a planted interaction, found in the second launch
        data[s, :nA] = rng.choice([1, 2], size=nA)
    data[38] = data[22]; data[39] = data[35]                         # deliberate ties: (6, 22, 35) = (6, 22, 39) = (6, 35, 38) = (6, 38, 39)
    fold = epi_random_folds(rng, nA, nU, k)
    eng.epi_set_dataset(data, nA, nU)
    eng.epi_set_folds(fold, k)
    masks = orc.fold_masks_from_assignment(fold, k)
    triples = all_combs(v, 3)
    assert len(triples) == 9880
    for subset in SUBSETS:
        acc, rm = orc.epi_scan_triples(data, nA, nU, masks, subset)
        t = {tuple(c): n for n, c in enumerate(triples)}
        assert np.array_equal(acc[:, t[6, 22, 35]], acc[:, t[6, 38, 39]])
        rm8 = np.zeros(rm.shape + (8,), np.uint32)
        rm8[..., 0] = rm
        for N in (5, 200):
            info = _check_tile_ranking(eng, 3, subset, N, (acc, rm, triples), WIDE, ("launches", subset, N))
            assert info["launches"] >= 2 and info["relaunches"] == 0, info
            info = _check_rank_order(eng, 3, subset, N, triples, acc, rm8, WIDE, ("launches, order", subset, N))
            assert info["launches"] >= 2, info


# ---- 6. state that outlives a call -------------------------------------------------------------------------------------------

def test_state_across_wide_and_packed_layouts(eng):
    # one engine: the fold tables, thresholds and counters follow the layout's fold count -- 33 folds, 10, 17; then a large-class
    # dataset, a small one, and the large one again.  After every change: pairs, triples, order 4, and the kernel that ran
    rng = np.random.default_rng(66)

    expected = {}                                                    # the oracle's answers per (cohort, folds, subset): computed once

    def calls(data, nA, nU, fold, k, pairs_kernel, triples_kernel, order_kernel):
        masks = orc.fold_masks_from_assignment(fold, k)
        v = data.shape[0]
        for subset, N in ((hpgv.EPI_TESTING, 4), (hpgv.EPI_TRAINING, 30)):
            if (nA, k, subset) not in expected:
                expected[nA, k, subset] = (orc.epi_scan_pairs(data, nA, nU, masks, subset) + (all_combs(v, 2),),
                                           orc.epi_scan_triples(data, nA, nU, masks, subset) + (all_combs(v, 3),),
                                           _models(data, nA, nU, masks, subset, 4))
            scan2, scan3, models4 = expected[nA, k, subset]
            _check_tile_ranking(eng, 2, subset, N, scan2, pairs_kernel, ("state pairs", k, nA))
            _check_tile_ranking(eng, 3, subset, N, scan3, triples_kernel, ("state triples", k, nA))
            _check_rank_order(eng, 4, subset, N, *models4, order_kernel, ("state order 4", k, nA))

    nA, nU = 200, 170
    small = epi_random_dataset(rng, 8, nA, nU, p_missing=0.02)
    eng.epi_set_dataset(small, nA, nU)
    for k in (33, 10, 17):
        fold = epi_random_folds(rng, nA, nU, k)
        eng.epi_set_folds(fold, k)
        if k > 16:
            calls(small, nA, nU, fold, k, WIDE, WIDE, WIDE)
        else:
            calls(small, nA, nU, fold, k, hpgv.EPI_KERNEL_PAIRS_MFMA, hpgv.EPI_KERNEL_TRIPLES_MFMA, hpgv.EPI_KERNEL_COMBS)
    big, big_fold, _ = _large_cohort(140000, 300, 2)
    for turn in range(3):
        if turn == 1:
            fold = epi_random_folds(rng, nA, nU, 5)
            eng.epi_set_dataset(small, nA, nU)
            eng.epi_set_folds(fold, 5)
            calls(small, nA, nU, fold, 5, hpgv.EPI_KERNEL_PAIRS_MFMA, hpgv.EPI_KERNEL_TRIPLES_MFMA, hpgv.EPI_KERNEL_COMBS)
        else:
            eng.epi_set_dataset(big, 140000, 300)
            eng.epi_set_folds(big_fold, 2)
            calls(big, 140000, 300, big_fold, 2, WIDE, WIDE, WIDE)


# ---- 7. a group context ------------------------------------------------------------------------------------------------------

def test_group_ranking_of_a_wide_layout():
    rng = np.random.default_rng(77)
    nA, nU, k, N = 120, 100, 17, 12
    g = hpgv.Engine([0, 0])
    one = hpgv.Engine(0)
    try:
        g.set_option("epi_wide", 1)                                  # goes to both members
        one.set_option("epi_wide", 1)
        for order, v in ((2, 130), (4, 12)):                         # (order 2: shares of whole blocks of 64 first SNPs)
            data = epi_random_dataset(rng, v, nA, nU, p_missing=0.02)
            fold = epi_random_folds(rng, nA, nU, k)
            masks = orc.fold_masks_from_assignment(fold, k)
            for e in (g, one):
                e.epi_set_dataset(data, nA, nU)
                e.epi_set_folds(fold, k)
            shares = [g.group_epi_share(order, m) for m in range(2)]
            assert shares[0][0] == 0 and shares[0][1] == shares[1][0] and shares[1][1] == v and shares[0][1] > 0
            for subset in SUBSETS:
                if order == 2:
                    acc, rm = orc.epi_scan_pairs(data, nA, nU, masks, subset)
                    combs, rm8 = all_combs(v, 2), np.zeros(rm.shape + (8,), np.uint32)
                    rm8[..., 0] = rm
                else:
                    combs, acc, rm8 = _models(data, nA, nU, masks, subset, order)
                res = g.group_epi_rank(order, subset, N)
                single = one.epi_rank_order(order, subset, N)
                assert one.epi_last_rank_info()["kernel"] == WIDE
                for f in range(k):
                    ok = np.flatnonzero(~np.isnan(acc[f]))
                    best = ok[np.argsort(-acc[f][ok], kind="stable")[:N]]
                    n = len(best)
                    for r in (res, single):
                        assert int(r["n"][f]) == n, (order, subset, f)
                        assert np.array_equal(r["combs"][f][:n], combs[best]), (order, subset, f)
                        assert np.array_equal(r["accuracy"][f][:n], acc[f][best]) and np.array_equal(r["risky"][f][:n], rm8[f][best]), (order, subset, f)
    finally:
        g.close()
        one.close()


# ---- 8. the runner -----------------------------------------------------------------------------------------------------------

def test_run_epistasis_with_20_folds(tmp_path):
    """hpgv_run_epistasis as in test_run_epistasis_from_a_dataset_file, with --num-folds 20: the runner sets "epi_wide" for its
    run; the expected report is rebuilt from the oracle's scan with the same folds (same rand() stream)."""
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
    v, nA, nU, k, n, reps = 45, 90, 110, 20, 8, 2
    data = epi_random_dataset(rng, v, nA, nU)
    data[3, :nA] = rng.choice([1, 2], size=nA); data[30, :nA] = rng.choice([1, 2], size=nA)
    path = tmp_path / "epi.bin"
    with open(path, "wb") as f:                                      # dataset.c:63-76
        f.write(struct.pack("<III", v, nA, nU)); f.write(data.tobytes())
    libc.srand(777)                                                  # the folds the run will deal: same seed, same calls
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


# ---- 9. what stays refused ---------------------------------------------------------------------------------------------------

def test_what_stays_refused(eng):
    rng = np.random.default_rng(9)
    nA, nU = 60, 50
    data = epi_random_dataset(rng, 7, nA, nU)
    eng.epi_set_dataset(data, nA, nU)
    with pytest.raises(hpgv.HpgvError, match="64"):
        eng.epi_set_folds(epi_random_folds(rng, nA, nU, 65), 65)     # the wide kernel's fold tables end at 64
    eng.epi_set_folds(epi_random_folds(rng, nA, nU, 17), 17)
    for scan in (lambda: eng.epi_scan_pairs(hpgv.EPI_TESTING), lambda: eng.epi_scan_triples(hpgv.EPI_TESTING)):
        with pytest.raises(hpgv.HpgvError, match="hpgv_epi_eval_combs"):      # the dense scans read tables a wide-only layout lacks
            scan()
    with pytest.raises(hpgv.HpgvError):
        eng.epi_rank_order(6, hpgv.EPI_TESTING, 3)                   # the model record holds 243 cells
    plain = hpgv.Engine(0)                                           # without the option every limit is where it was
    try:
        plain.epi_set_dataset(data, nA, nU)
        with pytest.raises(hpgv.HpgvError, match="16"):
            plain.epi_set_folds(epi_random_folds(rng, nA, nU, 17), 17)
    finally:
        plain.close()
