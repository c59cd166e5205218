"""The recorded numbers of the permutation within strata (profiles/assoc_cmh_perm.json, written by tools/bench_assoc_cmh_perm.py)
against what DESIGN.md states about them.  The expectation was: at every K measured the new call beats route (b) -- the masked
label rows through hpgv_assoc_perm_dev with d_perm_counts on the commit before -- by more than the run-to-run spread of both
(its slowest run is faster than (b)'s fastest).  Recorded: with stratum-contiguous columns it does, at every K on both shapes; with
interleaved columns it does on the 200-sample shape and at K = 64 on the 10 000-sample shape, and MISSES at K = 2 and K = 8 there
(0.659 against 0.383 ms, 2.49 against 1.69 ms), which DESIGN.md says in bold with the cause.  This test holds the file to exactly
that: the flags the tool wrote follow from the times, the contiguous form beats (b) everywhere, and the interleaved misses are the
two DESIGN.md names and no others."""
import json
import os

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "assoc_cmh_perm.json")
STATED_MISSES = {(10000, 4096, 2, "interleaved"), (10000, 4096, 8, "interleaved")}


def test_the_recorded_times_against_route_b_are_what_the_design_document_states():
    with open(PROFILE) as f:
        doc = json.load(f)
    runs = doc["runs"]
    assert doc["bench"] == "assoc_cmh_perm" and doc["route_b_measured_on"] == "parent checkout"
    assert {(r["samples"], r["rows"]) for r in runs} == {(10000, 4096), (200, 65536)} and {r["strata"] for r in runs} == {2, 8, 64}
    assert all(r["perms"] == 1000 for r in runs) and len(runs) == 6
    misses = set()
    for r in runs:
        fl, b = r["floor_hpgv_assoc_perm_dev"], r["route_b"]
        assert isinstance(b, dict), "every route (b) of the recorded shapes fitted the device"
        assert abs(r["contiguous_over_floor"] - r["contiguous"]["ms_med"] / fl["ms_med"]) < 1e-3
        for order in ("contiguous", "interleaved"):
            beats = r[order]["ms_max"] < b["ms_min"]
            assert r[order + "_beats_route_b"] == beats
            if not beats:
                misses.add((r["samples"], r["rows"], r["strata"], order))
    assert misses == STATED_MISSES
