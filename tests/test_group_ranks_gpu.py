"""The group hand-over at TWO TO EIGHT RANKS on one GPU (hpgv_group_capi.hip: hand_over, counters_reduce, gather_lists).

RCCL refuses one device twice, so on a one-GPU box every context is rank 0 and tests/test_group_scan_gpu.py never runs
`comms[M.rank]` with a rank above 0, a peer number other than 0, several senders in one group or a reduce over more than
one rank.  Here libhpgv.so loads a stand-in communicator (tests/c/fake_rccl.hip through HPGV_RCCL_LIB) that accepts
repeated devices, and the test switch group_fake_ranks = n puts the members that share device 0 on ranks of their own:
the first n share rank 0, every later member is a rank.  n = 1 is the topology of G distinct GPUs, n = 2 with four
members is [0, 0, 1, 2]: a local copy beside two communicator routes.

Every case asserts (1) the rank count, (2) results bit-identical to one ordinary context (the C drivers) or equal to the
oracle (in process), and (3) the stand-in's own totals ($FAKE_RCCL_LOG): the bytes that went THROUGH the communicator
are the bytes the topology says must -- a member routed around it would leave the results right and the count short.
The stand-in is tested by itself at the end: one that accepted anything would prove nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import build_fake_rccl, hpgv
from test_group_scan_gpu import _AssocCohort, driver, epi_driver, ranking_between_unsynced_scans_scenario, refused_group_call_scenario  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, INVALID_USAGE = 0, 4, 5          # ncclResult_t
INT8, INT32, FLOAT32, SUM = 0, 2, 7, 0                   # ncclDataType_t, ncclRedOp_t
MODEL_BYTES = 64                                          # one record of a ranking's top lists (hpgv.h: hpgv_group_epi_rank)


@pytest.fixture(scope="module")
def fake_rccl(tmp_path_factory):
    hpgv.build()
    return build_fake_rccl(tmp_path_factory.mktemp("fake_rccl"))[0]


def totals(log):
    """the lines of $FAKE_RCCL_LOG, one per world, as dicts of ints"""
    with open(log) as f:
        return [{k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line)} for line in f if line.strip()]


def comm_members(members, shared, self_exchange):
    """the members whose results reach member 0 through the communicator under group_fake_ranks = shared"""
    return [k for k in range(members) if (k == 0 and self_exchange) or (k > 0 and k >= shared)]


def n_ranks(members, shared):
    return members - min(shared, members) + 1


def shard(v, members, k):
    return v * (k + 1) // members - v * k // members


# bytes per variant of the pieces that have a destination, and how many pieces that is, per call of the scan driver:
#   chi-square 16 + 8 + 8 + 8, Fisher 16 + 8 + 8 (no chi-square array), TDT 8 + 8 + 8 + 8, stats 32 + 8 + 8
SCAN_CALL_BYTES, SCAN_CALL_PIECES, SCAN_CALLS_EACH = (40, 32, 32, 48), (4, 3, 4, 3), 3


@pytest.mark.parametrize("members,variants,samples,shared,self_exchange", [
    (2, 1009, 301, 1, 0),
    (3, 7, 30, 1, 0),                # ragged
    (4, 3, 30, 1, 0),                # a rank whose shard is empty
    (8, 1009, 301, 1, 0),
    (8, 1009, 301, 1, 1),            # member 0 over the communicator too: every result byte is carried
    (4, 1009, 301, 2, 0),            # [0, 0, 1, 2]: a local add (k_add_i32) beside the reduce, a local copy beside two sends
    (3, 150001, 1201, 1, 0),         # transfers long enough for the next call's scans to run under them
    (2, 0, 30, 1, 0),                # no variants: no send may be queued
])
def test_c_host_drives_the_group_scan_over_ranks(driver, fake_rccl, tmp_path, members, variants, samples, shared, self_exchange):
    log = str(tmp_path / "rccl.log")
    env = dict(os.environ, HPGV_RCCL_LIB=fake_rccl, FAKE_RCCL_LOG=log)
    args = [driver, str(members), str(variants), str(samples)] + (["self"] if self_exchange else []) + ["ranks=%d" % shared]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    ranks = n_ranks(members, shared)
    assert "members=%d rccl_ranks=%d self_exchange=%d\n" % (members, ranks, self_exchange) in r.stdout and "group scan ok" in r.stdout
    assert r.stdout.count("bit-identical") == 4          # chi-square, Fisher, TDT, stats (with the per-sample counters)
    carried = [shard(variants, members, k) for k in comm_members(members, shared, self_exchange)]
    assert totals(log) == [dict(ranks=ranks,
                                sends=SCAN_CALLS_EACH * sum(SCAN_CALL_PIECES) * sum(1 for n in carried if n),
                                send_bytes=SCAN_CALLS_EACH * sum(SCAN_CALL_BYTES) * sum(carried),
                                reduces=SCAN_CALLS_EACH * ranks, reduce_elems=SCAN_CALLS_EACH * ranks * samples)], r.stdout


@pytest.mark.parametrize("members,v,nA,nU,k,order,shared,self_exchange", [
    (2, 300, 400, 380, 5, 2, 1, 0),
    (3, 100, 150, 170, 4, 2, 1, 0),          # an empty share: its (unused) list is carried all the same
    (3, 60, 120, 140, 4, 3, 1, 1),
    (4, 16, 90, 110, 3, 4, 2, 0),            # [0, 0, 1, 2]
])
def test_c_host_deals_the_epistasis_scan_over_ranks(epi_driver, fake_rccl, tmp_path, members, v, nA, nU, k, order, shared, self_exchange):
    log = str(tmp_path / "rccl.log")
    env = dict(os.environ, HPGV_RCCL_LIB=fake_rccl, FAKE_RCCL_LOG=log)
    args = [epi_driver] + [str(x) for x in (members, v, nA, nU, k, order)] + (["self"] if self_exchange else []) + ["ranks=%d" % shared]
    r = subprocess.run(args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    ranks = n_ranks(members, shared)
    assert "rccl_ranks=%d\n" % ranks in r.stdout and "group epistasis ok" in r.stdout and r.stdout.count("bit-identical") == 2
    # the driver ranks both evaluation subsets, 24 models per fold: every communicator-route member sends its k x 24 records
    sends = 2 * len(comm_members(members, shared, self_exchange))
    assert totals(log) == [dict(ranks=ranks, sends=sends, send_bytes=sends * k * 24 * MODEL_BYTES, reduces=0, reduce_elems=0)], r.stdout


# ---- in process: against the oracle.  HPGV_RCCL_LIB by monkeypatch, so that later tests of the session load RCCL again. ----

@pytest.fixture
def stand_in(fake_rccl, tmp_path, monkeypatch):
    log = str(tmp_path / "rccl.log")
    monkeypatch.setenv("HPGV_RCCL_LIB", fake_rccl)
    monkeypatch.setenv("FAKE_RCCL_LOG", log)
    return log


ASSOC_BYTES, ASSOC_PIECES = 40, 4            # a chi-square call: counts 16, odds 8, chi-square 8, p 8


def assoc_totals(members, v, shared, self_exchange, calls):
    """what `calls` chi-square calls of an _AssocCohort of v variants leave in the stand-in's log"""
    carried = [shard(v, members, k) for k in comm_members(members, shared, self_exchange)]
    return dict(ranks=n_ranks(members, shared), sends=calls * ASSOC_PIECES * sum(1 for n in carried if n),
                send_bytes=calls * ASSOC_BYTES * sum(carried), reduces=0, reduce_elems=0)


@pytest.mark.parametrize("self_exchange", [0, 1])
def test_three_ranks_against_the_oracle(stand_in, self_exchange):
    """61 x 301 on [0, 0, 0] as three ranks: counts exactly the oracle's, statistics within TOL, two calls into two result sets"""
    c = _AssocCohort([0, 0, 0], self_exchange, fake_ranks=1)
    a, b = c.result_set(), c.result_set()
    c.assoc(a)
    c.assoc(b)
    c.g.group_sync()
    c.check(a)
    c.check(b)
    c.close()
    assert totals(stand_in) == [assoc_totals(3, _AssocCohort.V, 1, self_exchange, 2)]


@pytest.mark.parametrize("self_exchange", [0, 1])
def test_a_refused_group_call_leaves_the_ranks_usable(stand_in, fake_rccl, self_exchange):
    """test_a_refused_group_call_leaves_the_group_usable at three and four ranks.  After the refused calls (one of them drained)
    the stand-in has no group open and nothing recorded: ending a group is an error, and the correct calls that follow carry
    exactly their own sends."""
    F = C.CDLL(fake_rccl)                                                   # the copy libhpgv.so holds: same path, same thread

    def no_group_is_open():
        assert F.ncclGroupEnd() == INVALID_USAGE
        assert F.ncclGroupStart() == OK and F.ncclGroupEnd() == OK         # an empty group: nothing was left recorded

    refused_group_call_scenario(self_exchange, fake_ranks=1, after_refusals=no_group_is_open)
    assert totals(stand_in) == [assoc_totals(3, _AssocCohort.V, 1, self_exchange, 2), assoc_totals(4, 3, 1, self_exchange, 1)]


@pytest.mark.parametrize("self_exchange", [0, 1])
def test_a_group_ranking_between_unsynced_scans_over_ranks(stand_in, self_exchange):
    """test_a_group_ranking_between_unsynced_scans with member 1 on a rank of its own: three scans and, between them, the gather
    of a ranking (3 folds x 5 models per member) share the second rank's stream, scratch generations and communicator"""
    ranking_between_unsynced_scans_scenario(self_exchange, fake_ranks=1)
    want = assoc_totals(2, _AssocCohort.V, 1, self_exchange, 3)
    lists = len(comm_members(2, 1, self_exchange))
    want["sends"] += lists
    want["send_bytes"] += lists * 3 * 5 * MODEL_BYTES
    assert totals(stand_in) == [want]


def test_fake_ranks_must_be_set_before_the_communicator(stand_in):
    g = hpgv.Engine([0, 0])
    g.set_option("group_fake_ranks", 1)
    g.set_option("group_fake_ranks", 0)
    g.set_option("group_fake_ranks", 1)
    assert g.group_comm_init() == 2
    assert g.L.hpgv_set_option(g.h, b"group_fake_ranks", 2) == hpgv.ERR_STATE
    assert g.group_comm_init() == 2
    g.close()
    assert totals(stand_in) == [dict(ranks=2, sends=0, send_bytes=0, reduces=0, reduce_elems=0)]
    e = hpgv.Engine(0)
    with pytest.raises(hpgv.HpgvError):                                      # an ordinary context has no such option
        e.set_option("group_fake_ranks", 1)
    e.close()


# ---- the stand-in itself, through ctypes, on device buffers and streams of an Engine ----

class _World:
    """a world of the stand-in over device 0, one stream per rank, and device memory with known contents"""

    def __init__(self, lib, n):
        F = self.F = C.CDLL(lib)
        vp = C.c_void_p
        F.ncclCommInitAll.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int)]
        F.ncclCommDestroy.argtypes = [vp]
        F.ncclCommCount.argtypes = [vp, C.POINTER(C.c_int)]
        F.ncclGetErrorString.argtypes, F.ncclGetErrorString.restype = [C.c_int], C.c_char_p
        F.ncclSend.argtypes = F.ncclRecv.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, vp, vp]
        F.ncclReduce.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, vp]
        self.e = hpgv.Engine(0)
        self.n = n
        self.comms = (vp * n)()
        assert F.ncclCommInitAll(self.comms, n, (C.c_int * n)(*([0] * n))) == OK
        self.streams = []
        for _ in range(n):
            s = vp()
            assert self.e.L.hpgv_stream_create(self.e.h, C.byref(s)) == hpgv.OK
            self.streams.append(s)

    def buf(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.e.alloc(arr.nbytes)
        self.e.h2d(p, arr)
        return p

    def send(self, r, p, count, to, dtype=INT8):
        return self.F.ncclSend(p, count, dtype, to, self.comms[r], self.streams[r])

    def recv(self, r, p, count, frm, dtype=INT8):
        return self.F.ncclRecv(p, count, dtype, frm, self.comms[r], self.streams[r])

    def reduce(self, r, src, dst, count, root=0, dtype=INT32, op=SUM):
        return self.F.ncclReduce(src, dst, count, dtype, op, root, self.comms[r], self.streams[r])

    def sync(self):
        for s in self.streams:
            assert self.e.L.hpgv_stream_sync(self.e.h, s) == hpgv.OK

    def close(self):
        self.sync()
        for c in self.comms:
            assert self.F.ncclCommDestroy(c) == OK
        for s in self.streams:
            assert self.e.L.hpgv_stream_destroy(self.e.h, s) == hpgv.OK
        self.e.close()


def at(p, off):
    return C.c_void_p(p.value + off)


CANARY = 0xA5


def _exchange(w, rng):
    """Ranks 1 and 2 send to rank 0 in one group: rank 1 two messages of different sizes, rank 2 one, the receives issued in
    another order than the sends.  Returns (sends, bytes).  The right bytes land and every byte around them keeps its canary."""
    m1a, m1b, m2 = (rng.integers(0, 256, n, dtype=np.uint8) for n in (1000, 24, 37))
    d_m1a, d_m1b, d_m2 = w.buf(m1a), w.buf(m1b), w.buf(m2)
    dst = np.full(4096, CANARY, np.uint8)
    d_dst = w.buf(dst)
    F = w.F
    assert F.ncclGroupStart() == OK
    assert w.send(1, d_m1a, 1000, 0) == OK and w.send(2, d_m2, 37, 0) == OK and w.send(1, d_m1b, 24, 0) == OK
    assert w.recv(0, at(d_dst, 3000), 37, 2) == OK
    assert w.recv(0, at(d_dst, 256), 1000, 1) == OK and w.recv(0, at(d_dst, 2000), 24, 1) == OK
    assert F.ncclGroupEnd() == OK
    w.sync()
    dst[3000:3037], dst[256:1256], dst[2000:2024] = m2, m1a, m1b
    assert np.array_equal(w.e.d2h(d_dst, (4096,), np.uint8), dst)
    for p in (d_m1a, d_m1b, d_m2, d_dst):
        w.e.free(p)
    return 3, 1061


def test_stand_in_carries_a_three_rank_exchange(fake_rccl, tmp_path, monkeypatch):
    log = str(tmp_path / "rccl.log")
    monkeypatch.setenv("FAKE_RCCL_LOG", log)
    w = _World(fake_rccl, 3)
    n = C.c_int(0)
    assert w.F.ncclCommCount(w.comms[2], C.byref(n)) == OK and n.value == 3
    assert len({w.F.ncclGetErrorString(r) for r in range(8)}) == 8      # a fixed text per code
    sends, nbytes = _exchange(w, np.random.default_rng(1))
    assert not os.path.exists(log)                                           # the totals are the LAST destroy's
    w.close()
    assert totals(log) == [dict(ranks=3, sends=sends, send_bytes=nbytes, reduces=0, reduce_elems=0)]


def test_stand_in_reduces_over_three_ranks(fake_rccl, tmp_path, monkeypatch):
    """int32 sums onto the root, exactly: in place at the root (as the library calls it) and into a receive buffer of its own;
    the other ranks' receive buffers stay as they were.  300 elements: more than one block of the add kernel."""
    log = str(tmp_path / "rccl.log")
    monkeypatch.setenv("FAKE_RCCL_LOG", log)
    w = _World(fake_rccl, 3)
    rng = np.random.default_rng(2)
    n = 300
    x = [rng.integers(-2 ** 29, 2 ** 29, n, dtype=np.int32) for _ in range(3)]
    for root, in_place in ((0, True), (2, False)):
        d_x = [w.buf(a) for a in x]
        d_out = [w.buf(np.full(n + 2, 7 + r, np.int32)) for r in range(3)]
        assert w.F.ncclGroupStart() == OK
        for r in range(3):
            dst = d_x[r] if in_place else at(d_out[r], 4)
            assert w.reduce(r, d_x[r], dst, n, root) == OK
        assert w.F.ncclGroupEnd() == OK
        w.sync()
        total = x[0] + x[1] + x[2]
        for r in range(3):
            got_x, got_out = w.e.d2h(d_x[r], (n,), np.int32), w.e.d2h(d_out[r], (n + 2,), np.int32)
            want_out = np.full(n + 2, 7 + r, np.int32)
            if r == root and not in_place:
                want_out[1:n + 1] = total
            assert np.array_equal(got_x, total if (r == root and in_place) else x[r])
            assert np.array_equal(got_out, want_out)
        for p in d_x + d_out:
            w.e.free(p)
    w.close()
    assert totals(log) == [dict(ranks=3, sends=0, send_bytes=0, reduces=6, reduce_elems=6 * n)]


def test_stand_in_refuses_what_rccl_would_hang_on(fake_rccl, tmp_path, monkeypatch):
    """Every refusal queues nothing -- the destinations keep their canaries -- and leaves the world able to complete a correct
    exchange right after it."""
    log = str(tmp_path / "rccl.log")
    monkeypatch.setenv("FAKE_RCCL_LOG", log)
    w = _World(fake_rccl, 3)
    F, rng = w.F, np.random.default_rng(3)
    src = rng.integers(0, 256, 512, dtype=np.uint8)
    ints = rng.integers(-1000, 1000, 128, dtype=np.int32)
    d_src = w.buf(src)
    d_int = [w.buf(ints) for _ in range(3)]
    d_dst = w.buf(np.full(1024, CANARY, np.uint8))

    def grouped(calls, ended):
        """the calls all return ncclSuccess (they are only recorded); the group's end is `ended`"""
        assert F.ncclGroupStart() == OK
        assert [c() for c in calls] == [OK] * len(calls)
        assert F.ncclGroupEnd() == ended

    cases = {
        "a send without its receive": lambda: grouped([lambda: w.send(1, d_src, 512, 0)], INVALID_USAGE),
        "a receive without its send": lambda: grouped([lambda: w.recv(0, d_dst, 512, 1)], INVALID_USAGE),
        "a matched pair beside a send without its receive: neither is carried": lambda: grouped(
            [lambda: w.send(1, d_src, 512, 0), lambda: w.recv(0, d_dst, 512, 1), lambda: w.send(2, d_src, 100, 0)], INVALID_USAGE),
        "a count mismatch": lambda: grouped([lambda: w.send(1, d_src, 512, 0), lambda: w.recv(0, d_dst, 511, 1)], INVALID_USAGE),
        "a datatype mismatch": lambda: grouped([lambda: w.send(1, d_src, 128, 0, INT32), lambda: w.recv(0, d_dst, 128, 1, INT8)], INVALID_USAGE),
        "a receive naming the wrong peer": lambda: grouped([lambda: w.send(1, d_src, 512, 0), lambda: w.recv(0, d_dst, 512, 2)], INVALID_USAGE),
        "a send on the wrong rank's communicator": lambda: grouped([lambda: w.send(0, d_src, 512, 0), lambda: w.recv(0, d_dst, 512, 1)], INVALID_USAGE),
        "a reduce that one rank omits": lambda: grouped([lambda r=r: w.reduce(r, d_int[r], d_int[r], 128) for r in (0, 2)], INVALID_USAGE),
        "a reduce one rank calls twice": lambda: grouped([lambda r=r: w.reduce(r, d_int[r], d_int[r], 128) for r in (0, 1, 1)], INVALID_USAGE),
        "a reduce with a different count on one rank": lambda: grouped(
            [lambda r=r: w.reduce(r, d_int[r], d_int[r], 127 if r == 1 else 128) for r in range(3)], INVALID_USAGE),
        "a reduce with a different root on one rank": lambda: grouped(
            [lambda r=r: w.reduce(r, d_int[r], d_int[r], 128, root=1 if r == 2 else 0) for r in range(3)], INVALID_USAGE),
    }

    def send_outside_a_group():
        assert w.send(1, d_src, 512, 0) == INVALID_USAGE and w.recv(0, d_dst, 512, 1) == INVALID_USAGE

    def a_float_reduce():                               # the refused call is the group's error, and what was recorded beside it is dropped
        assert F.ncclGroupStart() == OK
        assert w.send(1, d_src, 512, 0) == OK and w.recv(0, d_dst, 512, 1) == OK
        assert w.reduce(0, d_int[0], d_int[0], 128, dtype=FLOAT32) == INVALID_ARGUMENT
        assert F.ncclGroupEnd() == INVALID_ARGUMENT

    def a_peer_out_of_range():
        assert F.ncclGroupStart() == OK
        assert w.send(1, d_src, 512, 3) == INVALID_ARGUMENT
        assert F.ncclGroupEnd() == INVALID_ARGUMENT

    def an_end_without_a_start():
        assert F.ncclGroupEnd() == INVALID_USAGE

    def a_reduce_outside_a_group():                     # a group of one call: two ranks are missing
        assert w.reduce(0, d_int[0], d_int[0], 128) == INVALID_USAGE

    cases.update({f.__name__: f for f in (send_outside_a_group, a_float_reduce, a_peer_out_of_range, an_end_without_a_start, a_reduce_outside_a_group)})
    sends = nbytes = 0
    for name, refused in cases.items():
        refused()
        w.sync()
        assert np.all(w.e.d2h(d_dst, (1024,), np.uint8) == CANARY), name
        for d in d_int:
            assert np.array_equal(w.e.d2h(d, (128,), np.int32), ints), name
        s, b = _exchange(w, rng)                        # ... and the same world completes a correct exchange
        sends, nbytes = sends + s, nbytes + b
    w.close()
    assert totals(log) == [dict(ranks=3, sends=sends, send_bytes=nbytes, reduces=0, reduce_elems=0)]
