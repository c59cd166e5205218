// hpgv_group_capi.hip -- the variant-sharded resident scan of a group context (include/hpgv.h "hpgv_group_*").
//
// The reference's runner fans batches of variants out to its workers and collects one record per variant
// (assoc_runner.c:106-207, tdt_runner.c:150-200, stats_runner.c:176-215); variants carry no state from one to the next
// (assoc.c:38-82, tdt.c:41-271).  With the cohort resident in the HBM of G devices this becomes: member g scans the
// contiguous shard [g*V/G, (g+1)*V/G) on a stream of its own -- no traffic between devices while scanning -- and the ONE
// exchange is the hand-over of the per-variant result pieces onto member 0.  Per-sample counters
// (get_sample_stats) are sums over variants: ncclReduce onto member 0.
//
// The unit in four parts:
//   route      decided once per member when a call is planned (plan_call): member 0 produces IN PLACE; a second context on
//              member 0's device hands over by a device-LOCAL copy; another device over the group's COMMunicator
//              (ncclCommInitAll over the members' devices: one process, RCCL over xGMI, every peer on its own link into member 0)
//   hand_over  the one routine that moves bytes onto member 0, given a list of transfers: grouped ncclSend / ncclRecv, or
//              hipMemcpyAsync.  The scans' pieces and the epistasis ranking's top lists both go through it
//   rccl_group the one place an RCCL group is opened; it is ended whatever happens in between
//   group_scan the skeleton of hpgv_group_assoc / _tdt / _stats: an entry point brings its checks, its piece table and
//              what one member queues on its scan stream
//
// What has run where: RCCL itself at ONE rank only (the one-GPU test rig: every context on device 0 is rank 0, members 1 and
// up take the local copy).  The exchange logic -- which communicator, which peer, which offset, several senders in one
// group, the reduce over several ranks beside local adds -- has been executed at two to eight ranks over a stand-in
// communicator (tests/c/fake_rccl.hip through HPGV_RCCL_LIB, ranks dealt by the test switch group_fake_ranks).  Several
// GPUs are still unmeasured on hardware.
//
// librccl is loaded with dlopen when the communicator is first asked for: libhpgv.so itself has no RCCL dependency, a
// single-device user never loads it, and inside a process that already holds an RCCL (torch's) the same copy is used.
//
// Streams: every member has a scan stream and a transfer stream.  A call queues, per member: [wait until the transfer
// that last read this generation's scratch is done] scan + statistics kernels -> event -> (transfer stream) hand-over of the
// pieces.  Two generations of scratch per member let the transfers of call k run under the scans of call k + 1.  A call
// that fails after it has queued anything returns with every stream of the group idle (drain).
#include "hpgv_epi_host.h"

#include <dlfcn.h>
#include <thread>
// types and enums only: every function is reached through dlsym.  A build box without the RCCL headers still builds the
// library: the few declarations the group scan uses are restated below (values as in rccl.h; RCCL keeps them ABI-stable).
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
typedef struct ncclComm *ncclComm_t;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclInt32 = 2 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
extern "C" {
ncclResult_t ncclCommInitAll(ncclComm_t *comms, int ndev, const int *devlist);
ncclResult_t ncclCommDestroy(ncclComm_t comm);
ncclResult_t ncclCommCount(const ncclComm_t comm, int *count);
const char *ncclGetErrorString(ncclResult_t result);
ncclResult_t ncclGroupStart(void);
ncclResult_t ncclGroupEnd(void);
ncclResult_t ncclSend(const void *sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclRecv(void *recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclReduce(const void *sendbuff, void *recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op, int root,
                        ncclComm_t comm, hipStream_t stream);
}
#endif

// what the unit calls of librccl: GroupState holds nccl<name> as <name>, load_rccl resolves them, the probe asks for them
#define RCCL_SYMBOLS(X) X(CommInitAll) X(CommDestroy) X(CommCount) X(GetErrorString) X(GroupStart) X(GroupEnd) X(Send) X(Recv) X(Reduce)

struct GroupMember {
    hipStream_t scan = nullptr, xfer = nullptr;
    hipEvent_t scan_done[2] = {nullptr, nullptr}, xfer_done[2] = {nullptr, nullptr};
    bool xfer_pending[2] = {false, false};
    DevBuf scratch[2];              // this member's results on their way to member 0, one per generation of calls
    DevBuf miss[2];                 // int32: per-sample counters of this member's shard, per generation like the scratch
    int rank = 0;                   // RCCL rank of the member's device; 0: member 0's device
};

struct GroupState {
    std::mutex mu;                  // one group call is queued at a time
    void *dl = nullptr;
#define X(name) decltype(&nccl##name) name = nullptr;
    RCCL_SYMBOLS(X)
#undef X
    std::vector<ncclComm_t> comms;  // one per distinct device, rank r = r-th distinct device in member order
    std::vector<int> devs;
    std::vector<GroupMember> m;
    DevBuf lists;                   // member 0's device: the members' top lists of a ranking call, in member order
    unsigned gen = 0;
    bool ready = false;
};

namespace {

// several contexts of member 0's device add their counters at the same time, and member 0's own scan may still be counting
__global__ void k_add_i32(int32_t *__restrict__ dst, const int32_t *__restrict__ src, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && src[i]) atomicAdd(&dst[i], src[i]);
}

// dlopen of librccl under its usual names ($HPGV_RCCL_LIB first); `tried` collects why each candidate failed
void *open_rccl(std::string &tried) {
    // The communicator must sit on the SAME HIP / HSA runtime this library is bound to.  A process may hold a second ROCm stack
    // (importing torch after this library loads torch's bundled copies beside /opt/rocm's): a bare dlopen("librccl.so.1") then
    // hands back whichever librccl is already loaded, and one bound to the other stack finds its HSA uninitialised
    // ("no ROCm-capable device").  So the librccl NEXT TO the HIP runtime in use is tried first, by full path.
    std::string beside1, beside2;
    {
        Dl_info info;
        if (dladdr((const void *)&hipGetDeviceCount, &info) && info.dli_fname) {
            std::string dir(info.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) { dir.resize(slash + 1); beside1 = dir + "librccl.so.1"; beside2 = dir + "librccl.so"; }
        }
    }
    const char *env = getenv("HPGV_RCCL_LIB");
    const char *names[] = {env, beside1.c_str(), beside2.c_str(), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char *n : names) {
        if (!n || !*n) continue;
        void *dl = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (dl) return dl;
        const char *e = dlerror();                      // ONE call: dlerror() clears the message it returns
        tried += std::string(tried.empty() ? "" : "; ") + std::string(e ? e : n);
    }
    return nullptr;
}

int load_rccl(hpgv_ctx *g, GroupState *S) {
    if (S->dl) return HPGV_OK;
    std::string tried;
    S->dl = open_rccl(tried);
    if (!S->dl)
        return fail(g, HPGV_ERR_UNSUPPORTED, "the group-wide scan gathers its results over RCCL and librccl could not be loaded (%s); "
                                             "set HPGV_RCCL_LIB to its path", tried.c_str());
    const char *lacks = nullptr;
#define X(name) if (!lacks && !(S->name = (decltype(S->name))dlsym(S->dl, "nccl" #name))) lacks = "nccl" #name;
    RCCL_SYMBOLS(X)
#undef X
    if (!lacks) return HPGV_OK;
    dlclose(S->dl);
    S->dl = nullptr;
    return fail(g, HPGV_ERR_UNSUPPORTED, "librccl lacks %s", lacks);
}

// The ONE place an RCCL group is opened.  `calls` queues the group's operations and returns the first result that is not
// ncclSuccess; the group is ended whatever it returns -- no path leaves this function with the group open -- and the first
// failure of the three is the call's error.
template <class Calls>
int rccl_group(hpgv_ctx *g, GroupState *S, const char *what, Calls &&calls) {
    ncclResult_t r = S->GroupStart();
    if (r == ncclSuccess) {
        r = calls();
        const ncclResult_t ended = S->GroupEnd();
        if (r == ncclSuccess) r = ended;
    }
    return r == ncclSuccess ? HPGV_OK : fail(g, HPGV_ERR_HIP, "%s over the group's communicator failed: %s", what, S->GetErrorString(r));
}

// every stream of the group idle and no transfer pending; the first error of the waits
hipError_t quiesce(hpgv_ctx *g, GroupState *S) {
    hipError_t first = hipSuccess;
    for (size_t k = 0; k < S->m.size() && k < g->members.size(); ++k) {
        GroupMember &M = S->m[k];
        DeviceGuard dg(g->members[k]->device);
        for (hipStream_t st : {M.scan, M.xfer}) {
            const hipError_t e = st ? hipStreamSynchronize(st) : hipSuccess;
            if (first == hipSuccess) first = e;
        }
        M.xfer_pending[0] = M.xfer_pending[1] = false;
    }
    return first;
}

void shard_of(int64_t V, int G, int g, int64_t *lo, int64_t *hi) {
    *lo = (int64_t)((__int128)V * g / G);
    *hi = (int64_t)((__int128)V * (g + 1) / G);
}

// one result piece: `elem` bytes per variant, gathered into dst (member 0's device, variant v at dst + v * elem); a piece
// without a destination is computed into scratch and stays there
struct Piece { size_t elem; void *dst; };

// how a member's results reach member 0: it is member 0 and produces them where they belong; it is another context on member
// 0's device and copies them there (RCCL refuses one device twice: the one-GPU test rig); it sits on another device and sends
// them through the communicator -- as member 0 does to itself with the test switch group_self_exchange
enum class Route { in_place, local_copy, comm };

struct Transfer { int member; const void *src; void *dst; size_t bytes; };      // src on the member's device, dst on member 0's

struct Plan {
    hpgv_ctx *g;
    GroupState *S;
    int G, gen;
    std::vector<Route> route;
    std::vector<int64_t> lo, n;
    std::vector<char *> base;           // where member k's piece 0 starts in its scratch (in place: nowhere, see piece_at)
};

// cuts the shards, gives every member its route, makes the scratch of this generation ready and the scan stream wait for
// the transfer that last read it
int plan_call(hpgv_ctx *g, int64_t V, const std::vector<Piece> &pieces, Plan &P) {
    if (V < 0) return fail(g, HPGV_ERR_INVALID, "n_variants < 0");
    GroupState *S = g->grp;
    P.g = g; P.S = S; P.G = (int)g->members.size();
    P.gen = (int)(S->gen++ & 1u);
    P.lo.resize(P.G); P.n.resize(P.G); P.route.resize(P.G); P.base.assign(P.G, nullptr);
    size_t bytes_per_variant = 0;
    for (const Piece &pc : pieces) bytes_per_variant += pc.elem;
    for (int k = 0; k < P.G; ++k) {
        int64_t lo, hi;
        shard_of(V, P.G, k, &lo, &hi);
        if (hi - lo > 0x7fffffff) return fail(g, HPGV_ERR_UNSUPPORTED, "a member's shard has more than 2^31 - 1 variants");
        P.lo[k] = lo; P.n[k] = hi - lo;
        hpgv_ctx *mc = g->members[k];
        GroupMember &M = S->m[k];
        P.route[k] = k == 0 ? (g->group_self_exchange ? Route::comm : Route::in_place) : M.rank == 0 ? Route::local_copy : Route::comm;
        DeviceGuard dg(mc->device);
        // the transfer of two calls ago read this generation's scratch (member 0: wrote the caller's arrays of that call,
        // which a caller alternating between two result sets hands in again now)
        if (M.xfer_pending[P.gen]) {
            HIPCHK(mc, hipStreamWaitEvent(M.scan, M.xfer_done[P.gen], 0));
            M.xfer_pending[P.gen] = false;
        }
        if (P.route[k] == Route::in_place) continue;
        const size_t bytes = (size_t)P.n[k] * bytes_per_variant + 256;
        HIPCHK(mc, M.scratch[P.gen].reserve(bytes, round_up(bytes + bytes / 16, 256)));
        P.base[k] = M.scratch[P.gen].as<char>();
    }
    return HPGV_OK;
}

// a call that fails after plan_call may have work queued on members' streams and no event recorded for it: the streams are
// drained, so that the scratch of this generation and the caller's arrays are quiet when the error returns
int drain(const Plan &P, int rc) {
    (void)quiesce(P.g, P.S);
    (void)hipGetLastError();
    return rc;
}

// where member k produces its piece i: in the destination itself, or in its scratch behind the pieces in front of it
char *piece_at(const Plan &P, const std::vector<Piece> &pieces, int k, size_t i) {
    if (P.route[k] == Route::in_place) return pieces[i].dst ? (char *)pieces[i].dst + (size_t)P.lo[k] * pieces[i].elem : nullptr;
    size_t before = 0;
    for (size_t j = 0; j < i; ++j) before += pieces[j].elem;
    return P.base[k] + (size_t)P.n[k] * before;
}

// the pieces of every member that does not produce in place, as transfers onto member 0
std::vector<Transfer> piece_transfers(const Plan &P, const std::vector<Piece> &pieces) {
    std::vector<Transfer> T;
    for (int k = 0; k < P.G; ++k) {
        if (P.route[k] == Route::in_place || P.n[k] == 0) continue;
        for (size_t i = 0; i < pieces.size(); ++i)
            if (pieces[i].dst)
                T.push_back({k, piece_at(P, pieces, k, i), (char *)pieces[i].dst + (size_t)P.lo[k] * pieces[i].elem, (size_t)P.n[k] * pieces[i].elem});
    }
    return T;
}

// The ONE hand-over onto member 0, after the members' work is queued on their scan streams: every transfer stream waits for
// its member's scan, then carries that member's transfers by its route -- the communicator's in one RCCL group, then member
// by member the local copies -- and xfer_done marks the end of what it carried.
int hand_over(Plan &P, const std::vector<Transfer> &T) {
    hpgv_ctx *g = P.g;
    GroupState *S = P.S;
    for (int k = 0; k < P.G; ++k) {
        hpgv_ctx *mc = g->members[k];
        GroupMember &M = S->m[k];
        DeviceGuard dg(mc->device);
        HIPCHK(mc, hipEventRecord(M.scan_done[P.gen], M.scan));
        if (P.route[k] != Route::in_place) HIPCHK(mc, hipStreamWaitEvent(M.xfer, M.scan_done[P.gen], 0));
    }
    const auto goes = [&](const Transfer &t, Route r) { return P.route[t.member] == r; };
    if (std::any_of(T.begin(), T.end(), [&](const Transfer &t) { return goes(t, Route::comm); })) {
        const int rc = rccl_group(g, S, "the hand-over onto member 0", [&]() -> ncclResult_t {
            for (const Transfer &t : T) {
                if (!goes(t, Route::comm)) continue;
                GroupMember &M = S->m[(size_t)t.member];
                ncclResult_t r = S->Send(t.src, t.bytes, ncclInt8, 0, S->comms[(size_t)M.rank], M.xfer);
                if (r == ncclSuccess) r = S->Recv(t.dst, t.bytes, ncclInt8, M.rank, S->comms[0], S->m[0].xfer);
                if (r != ncclSuccess) return r;
            }
            return ncclSuccess;
        });
        if (rc) return rc;
    }
    for (int k = 0; k < P.G; ++k) {
        hpgv_ctx *mc = g->members[k];
        GroupMember &M = S->m[k];
        DeviceGuard dg(mc->device);
        for (const Transfer &t : T)
            if (t.member == k && goes(t, Route::local_copy)) HIPCHK(mc, hipMemcpyAsync(t.dst, t.src, t.bytes, hipMemcpyDeviceToDevice, M.xfer));
        HIPCHK(mc, hipEventRecord(M.xfer_done[P.gen], M.xfer));     // (member 0 in place: the event its next call of this generation waits for)
        M.xfer_pending[P.gen] = true;
    }
    return HPGV_OK;
}

int no_step(Plan &) { return HPGV_OK; }

// The skeleton of the three scans, after the entry point's own argument checks.  member(k, mc, stream, gt, n, at) queues
// member k's *_dev calls for its n variants, piece i produced at at[i]; `before` and `after` are what a call queues
// around the scans and their hand-over (the per-sample counters of hpgv_group_stats).
template <class Member, class Before, class After>
int group_scan(hpgv_ctx *g, const uint8_t *const *d_gt, int64_t V, const std::vector<Piece> &pieces, Member member, Before before, After after) {
    int rc = hpgv_group_comm_init(g);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g->grp->mu);
    Plan P;
    rc = plan_call(g, V, pieces, P);
    if (rc) return rc;
    rc = before(P);
    std::vector<void *> at(pieces.size());
    for (int k = 0; k < P.G && !rc; ++k) {
        if (P.n[k] == 0) continue;
        if (!d_gt[k]) { rc = fail(g, HPGV_ERR_INVALID, "member %d has %lld variants but no matrix", k, (long long)P.n[k]); break; }
        for (size_t i = 0; i < pieces.size(); ++i) at[i] = piece_at(P, pieces, k, i);
        rc = member(k, g->members[(size_t)k], P.S->m[(size_t)k].scan, d_gt[k], (int)P.n[k], at.data());
    }
    if (!rc) rc = hand_over(P, piece_transfers(P, pieces));
    if (!rc) rc = after(P);
    return rc ? drain(P, rc) : HPGV_OK;
}

// ---- the per-sample counters of hpgv_group_stats: sums over variants, so every member counts its shard and the counts are
//      added up on member 0.  Member 0 is where they are added, whichever way its pieces go: it counts straight into the
//      caller's array.  The others count into an array of their own and follow their route: a context on member 0's device adds
//      with k_add_i32, another device takes part in the ncclReduce. ----

// before the scans: where member k counts (miss[k]), zeroed on its scan stream.  d_total = nullptr: no counters are asked for
int counters_begin(Plan &P, int32_t *d_total, int n_samples, std::vector<int32_t *> &miss) {
    hpgv_ctx *g = P.g;
    if (!d_total) return HPGV_OK;
    if (!g->members[0]->stats.set) return fail(g, HPGV_ERR_STATE, "hpgv_set_stats_cohort has not been called");
    for (int k = 0; k < P.G && n_samples > 0; ++k) {
        hpgv_ctx *mc = g->members[(size_t)k];
        GroupMember &M = P.S->m[(size_t)k];
        DeviceGuard dg(mc->device);
        if (k == 0) {
            // the caller's array is the one destination every member ADDS into: the previous call's adds and its ncclReduce (the
            // OTHER generation's transfers) may still be running when this call's memset is queued.  plan_call made member 0's
            // scan wait for this generation only; with counters, it also waits for the other one.
            if (M.xfer_pending[P.gen ^ 1]) HIPCHK(g, hipStreamWaitEvent(M.scan, M.xfer_done[P.gen ^ 1], 0));
            miss[0] = d_total;
        } else {
            HIPCHK(mc, M.miss[P.gen].reserve((size_t)n_samples * sizeof(int32_t)));
            miss[(size_t)k] = M.miss[P.gen].as<int32_t>();
        }
        HIPCHK(mc, hipMemsetAsync(miss[(size_t)k], 0, (size_t)n_samples * sizeof(int32_t), M.scan));
    }
    return HPGV_OK;
}

// after the hand-over: a context on member 0's device adds its own on ITS transfer stream (which the next call of this
// generation waits for before it overwrites them), then one ncclReduce (sum, in place on member 0) over the communicator's
// ranks on member 0's transfer stream, behind those adds and member 0's own scan
int counters_reduce(Plan &P, int32_t *d_total, int n_samples) {
    if (!d_total || n_samples <= 0) return HPGV_OK;
    hpgv_ctx *g = P.g;
    GroupState *S = P.S;
    GroupMember &M0 = S->m[0];
    {
        DeviceGuard dg(g->members[0]->device);
        HIPCHK(g, hipStreamWaitEvent(M0.xfer, M0.scan_done[P.gen], 0));
        for (int k = 1; k < P.G; ++k) {
            GroupMember &M = S->m[(size_t)k];
            if (P.route[k] != Route::local_copy) continue;
            HIPCHK(g, hipStreamWaitEvent(M.xfer, M0.scan_done[P.gen], 0));      // member 0's memset of the counters is behind this event
            hipLaunchKernelGGL(k_add_i32, dim3((unsigned)((n_samples + 255) / 256)), dim3(256), 0, M.xfer, d_total,
                               M.miss[P.gen].as<int32_t>(), n_samples);
            HIPCHK(g, hipGetLastError());
            HIPCHK(g, hipEventRecord(M.xfer_done[P.gen], M.xfer));
            HIPCHK(g, hipStreamWaitEvent(M0.xfer, M.xfer_done[P.gen], 0));
        }
    }
    const int rc = rccl_group(g, S, "the reduce of the per-sample counters", [&]() -> ncclResult_t {
        ncclResult_t r = S->Reduce(d_total, d_total, (size_t)n_samples, ncclInt32, ncclSum, 0, S->comms[0], M0.xfer);
        for (int k = 1; k < P.G && r == ncclSuccess; ++k) {
            GroupMember &M = S->m[(size_t)k];
            int32_t *own = M.miss[P.gen].as<int32_t>();
            if (P.route[k] == Route::comm) r = S->Reduce(own, own, (size_t)n_samples, ncclInt32, ncclSum, 0, S->comms[(size_t)M.rank], M.xfer);
        }
        return r;
    });
    if (rc) return rc;
    for (int k = 0; k < P.G; ++k) {
        hpgv_ctx *mc = g->members[(size_t)k];
        GroupMember &M = S->m[(size_t)k];
        DeviceGuard dg(mc->device);
        HIPCHK(mc, hipEventRecord(M.xfer_done[P.gen], M.xfer));
        M.xfer_pending[P.gen] = true;
    }
    return HPGV_OK;
}

// ranks = the distinct devices in member order (a device may repeat only when it is member 0's; the test switch
// group_fake_ranks deals ranks by member instead), the communicator over them, and every member's streams and events.
// What a failure leaves behind, hpgv_group_release takes down.
int comm_setup(hpgv_ctx *g, GroupState *S) {
    const int G = (int)g->members.size();
    S->devs.clear();
    S->m.assign((size_t)G, GroupMember());
    // the test switch group_fake_ranks = n: the first n members share rank 0, every later member is a rank of its own in
    // member order, and the device list has one entry per rank -- repeated devices, which only a stand-in communicator takes
    const int shared = (int)std::min<long>(g->group_fake_ranks, G);
    for (int k = 0; k < G; ++k) {
        const int dev = g->members[(size_t)k]->device;
        if (shared > 0) {
            S->m[(size_t)k].rank = k < shared ? 0 : k - shared + 1;
            if (k == 0 || k >= shared) S->devs.push_back(dev);
            continue;
        }
        int r = -1;
        for (size_t i = 0; i < S->devs.size(); ++i) if (S->devs[i] == dev) r = (int)i;
        if (r > 0) return fail(g, HPGV_ERR_UNSUPPORTED, "device %d is listed twice and is not member 0's: only member 0's device may repeat (the one-GPU test rig)", dev);
        if (r < 0) { r = (int)S->devs.size(); S->devs.push_back(dev); }
        S->m[(size_t)k].rank = r;
    }
    if (int rc = load_rccl(g, S)) return rc;
    S->comms.assign(S->devs.size(), nullptr);
    const ncclResult_t r = S->CommInitAll(S->comms.data(), (int)S->devs.size(), S->devs.data());
    if (r != ncclSuccess) {
        S->comms.clear();
        return fail(g, HPGV_ERR_HIP, "ncclCommInitAll over %d device(s) failed: %s", (int)S->devs.size(), S->GetErrorString(r));
    }
    for (int k = 0; k < G; ++k) {
        hpgv_ctx *mc = g->members[(size_t)k];
        GroupMember &M = S->m[(size_t)k];
        DeviceGuard dg(mc->device);
        hipError_t e = hipStreamCreateWithFlags(&M.scan, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&M.xfer, hipStreamNonBlocking);
        for (int i = 0; i < 2 && e == hipSuccess; ++i) {
            e = hipEventCreateWithFlags(&M.scan_done[i], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&M.xfer_done[i], hipEventDisableTiming);
        }
        if (e != hipSuccess) return fail(g, HPGV_ERR_HIP, "group streams on device %d: %s", mc->device, hipGetErrorString(e));
    }
    return HPGV_OK;
}

}  // namespace

void hpgv_group_release(hpgv_ctx *g) {
    if (!g || !g->grp) return;
    GroupState *S = g->grp;
    (void)quiesce(g, S);
    if (S->CommDestroy)
        for (ncclComm_t c : S->comms) if (c) (void)S->CommDestroy(c);
    for (size_t k = 0; k < S->m.size() && k < g->members.size(); ++k) {
        GroupMember &M = S->m[k];
        DeviceGuard dg(g->members[k]->device);
        if (k == 0) S->lists.release();
        for (int i = 0; i < 2; ++i) {
            M.scratch[i].release();
            M.miss[i].release();
            if (M.scan_done[i]) (void)hipEventDestroy(M.scan_done[i]);
            if (M.xfer_done[i]) (void)hipEventDestroy(M.xfer_done[i]);
        }
        if (M.scan) (void)hipStreamDestroy(M.scan);
        if (M.xfer) (void)hipStreamDestroy(M.xfer);
    }
    // the library stays loaded: other groups (and the process's own RCCL users) may hold it
    delete S;
    g->grp = nullptr;
}

extern "C" {

int hpgv_group_comm_init(hpgv_ctx *g) {
    HPGV_ABI_TRY
    if (!is_group(g)) return fail(g, HPGV_ERR_INVALID, "hpgv_group_comm_init needs a group context (hpgv_create_multi)");
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->grp && g->grp->ready) return HPGV_OK;
    if (!g->grp) g->grp = new GroupState();
    const int rc = comm_setup(g, g->grp);
    if (rc) hpgv_group_release(g);
    else g->grp->ready = true;
    return rc;
    HPGV_ABI_CATCH(g)
}

int hpgv_group_rccl_probe(char *why, size_t why_cap) {
    try {
        std::string tried;
        void *dl = open_rccl(tried);
        if (why && why_cap) snprintf(why, why_cap, "%s", tried.c_str());
        if (!dl) return HPGV_ERR_UNSUPPORTED;
#define X(name) && dlsym(dl, "nccl" #name)
        const bool ok = true RCCL_SYMBOLS(X);
#undef X
        dlclose(dl);
        return ok ? HPGV_OK : HPGV_ERR_UNSUPPORTED;
    } catch (...) { return HPGV_ERR_NOMEM; }
}

int hpgv_group_comm_ranks(const hpgv_ctx *g) {
    if (!is_group(g)) return 0;
    // g->mu guards g->grp itself: hpgv_group_comm_init may delete the state on a failure path
    std::lock_guard<std::mutex> lk(const_cast<hpgv_ctx *>(g)->mu);
    if (!g->grp || !g->grp->ready || g->grp->comms.empty()) return 0;
    int n = 0;
    if (g->grp->CommCount(g->grp->comms[0], &n) != ncclSuccess) return 0;
    return n;
}

int hpgv_group_shard(const hpgv_ctx *g, int64_t n_variants, int member, int64_t *lo, int64_t *hi) {
    if (!g || !lo || !hi || n_variants < 0) return HPGV_ERR_INVALID;
    const int G = hpgv_group_size(g);
    if (member < 0 || member >= G) return HPGV_ERR_INVALID;
    shard_of(n_variants, G, member, lo, hi);
    return HPGV_OK;
}

int hpgv_group_sync(hpgv_ctx *g) {
    if (!is_group(g)) return fail(g, HPGV_ERR_INVALID, "hpgv_group_sync needs a group context");
    GroupState *S = nullptr;
    {   // g->mu guards g->grp itself (see hpgv_group_comm_ranks); a ready state lives until hpgv_destroy
        std::lock_guard<std::mutex> lk(g->mu);
        if (g->grp && g->grp->ready) S = g->grp;
    }
    if (!S) return HPGV_OK;
    std::lock_guard<std::mutex> lk(S->mu);
    HIPCHK(g, quiesce(g, S));
    return HPGV_OK;
}

int hpgv_group_assoc(hpgv_ctx *g, int task, const uint8_t *const *d_gt, const uint8_t *const *d_is_x, int64_t V,
                     int32_t *d_counts, double *d_odds, double *d_chisq, double *d_p) {
    HPGV_ABI_TRY
    if (!is_group(g)) return fail(g, HPGV_ERR_INVALID, "hpgv_group_assoc needs a group context (hpgv_create_multi)");
    if (task != HPGV_TASK_CHISQ && task != HPGV_TASK_FISHER) return fail(g, HPGV_ERR_INVALID, "task must be HPGV_TASK_CHISQ or HPGV_TASK_FISHER");
    if (!d_gt || (V > 0 && (!d_counts || !d_odds || !d_p || (task == HPGV_TASK_CHISQ && !d_chisq))))
        return fail(g, HPGV_ERR_INVALID, "bad group assoc arguments");
    const bool chisq = task == HPGV_TASK_CHISQ;
    const std::vector<Piece> pieces = {{16, d_counts}, {8, d_odds}, {8, chisq ? d_chisq : nullptr}, {8, d_p}};
    const auto member = [&](int k, hpgv_ctx *mc, hipStream_t st, const uint8_t *gt, int n, void *const *at) {
        int32_t *c = (int32_t *)at[0];
        double *o = (double *)at[1], *x = (double *)at[2], *p = (double *)at[3];
        const int rc = hpgv_assoc_scan_dev(mc, gt, n, d_is_x ? d_is_x[k] : nullptr, c, st);
        return rc ? rc : chisq ? hpgv_assoc_chisq_dev(mc, c, n, o, x, p, st) : hpgv_assoc_fisher_dev(mc, c, n, o, p, st);
    };
    return group_scan(g, d_gt, V, pieces, member, no_step, no_step);
    HPGV_ABI_CATCH(g)
}

int hpgv_group_tdt(hpgv_ctx *g, const uint8_t *const *d_gt, const uint8_t *const *d_is_x, int64_t V, int32_t *d_tu,
                   double *d_odds, double *d_chisq, double *d_p) {
    HPGV_ABI_TRY
    if (!is_group(g)) return fail(g, HPGV_ERR_INVALID, "hpgv_group_tdt needs a group context (hpgv_create_multi)");
    if (!d_gt || (V > 0 && (!d_tu || !d_odds || !d_chisq || !d_p))) return fail(g, HPGV_ERR_INVALID, "bad group tdt arguments");
    const std::vector<Piece> pieces = {{8, d_tu}, {8, d_odds}, {8, d_chisq}, {8, d_p}};
    const auto member = [&](int k, hpgv_ctx *mc, hipStream_t st, const uint8_t *gt, int n, void *const *at) {
        int32_t *tu = (int32_t *)at[0];
        const int rc = hpgv_tdt_scan_dev(mc, gt, n, d_is_x ? d_is_x[k] : nullptr, tu, st);
        return rc ? rc : hpgv_tdt_stats_dev(mc, tu, n, (double *)at[1], (double *)at[2], (double *)at[3], st);
    };
    return group_scan(g, d_gt, V, pieces, member, no_step, no_step);
    HPGV_ABI_CATCH(g)
}

int hpgv_group_stats(hpgv_ctx *g, const uint8_t *const *d_gt, int64_t V, int32_t *d_counts8, double *d_hwe_chi2,
                     double *d_hwe_p, int32_t *d_sample_missing) {
    HPGV_ABI_TRY
    if (!is_group(g)) return fail(g, HPGV_ERR_INVALID, "hpgv_group_stats needs a group context (hpgv_create_multi)");
    if (!d_gt || (V > 0 && (!d_counts8 || !d_hwe_chi2 || !d_hwe_p))) return fail(g, HPGV_ERR_INVALID, "bad group stats arguments");
    const std::vector<Piece> pieces = {{32, d_counts8}, {8, d_hwe_chi2}, {8, d_hwe_p}};
    const int n_samples = g->members[0]->stats.n_samples;
    std::vector<int32_t *> miss(g->members.size(), nullptr);          // where every member counts missing genotypes per sample, if asked for
    const auto member = [&](int k, hpgv_ctx *mc, hipStream_t st, const uint8_t *gt, int n, void *const *at) {
        int32_t *c8 = (int32_t *)at[0];
        int rc = hpgv_stats_scan_dev(mc, gt, n, c8, st);
        if (!rc) rc = hpgv_stats_hwe_dev(mc, c8, n, (double *)at[1], (double *)at[2], st);
        // k_sample_missing takes at most 65535 bands of rows per launch
        const int step = 65535 * hpgv::SAMPLE_STATS_ROWS;
        for (int v0 = 0; v0 < n && !rc && miss[(size_t)k]; v0 += step)
            rc = hpgv_sample_missing_dev(mc, gt + (size_t)v0 * mc->stats.pitch, std::min(step, n - v0), miss[(size_t)k], st);
        return rc;
    };
    return group_scan(g, d_gt, V, pieces, member, [&](Plan &P) { return counters_begin(P, d_sample_missing, n_samples, miss); },
                      [&](Plan &P) { return counters_reduce(P, d_sample_missing, n_samples); });
    HPGV_ABI_CATCH(g)
}

}  // extern "C"

// ---- the epistasis scan over the devices of a group (the reference deals block coordinates to its workers,
//      singlenode/epistasis_runner.c:114-145).  Every combination of `order` SNPs belongs to its FIRST SNP; the first SNPs are
//      cut into G runs of (nearly) equal numbers of combinations -- for pairs at multiples of 64 rows, the tile scan's unit --
//      member g ranks its run on its own device (hpgv_epi_{pairs,triples,order}_models, one host thread per member), and the
//      ONE exchange is the hand-over of the members' per-fold top lists (num_folds x max_ranking_size records of 64 bytes)
//      onto member 0, where they merge into the whole ranking: a model is in the whole top N only if it is in the top N of its
//      own share.

namespace {

// combinations of `order` SNPs out of V that begin with one of the first `rows` SNPs
long double epi_combs_before(int V, int order, int rows) {
    auto choose = [](int n, int k) -> long double { if (k < 0 || n < k) return 0.0L; long double r = 1.0L; for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i; return r; };
    return choose(V, order) - choose(V - std::min(rows, V), order);
}

// first SNP where member k's share begins: the first boundary (a multiple of `unit`) with at least k / G of the work before it
int epi_cut(int V, int order, int G, int k, int unit) {
    if (k <= 0) return 0;
    if (k >= G) return V;
    const long double target = epi_combs_before(V, order, V) * k / G;
    int lo = 0, hi = (V + unit - 1) / unit;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (epi_combs_before(V, order, std::min(mid * unit, V)) >= target) hi = mid; else lo = mid + 1;
    }
    return std::min(lo * unit, V);
}

// The gather of a ranking: the members' lists (`bytes` each, on the host) onto member 0's device and back to the host in
// member order.  To the hand-over this is a scan of G "variants" of `bytes` bytes: member k's shard is [k, k + 1), its one
// piece is its list, uploaded where a scan would have produced it -- on the transfer stream, behind whatever still reads
// this generation's scratch.
int gather_lists(hpgv_ctx *g, const std::vector<std::vector<EpiModel>> &lists, size_t bytes, std::vector<EpiModel> &all) {
    GroupState *S = g->grp;
    const int G = (int)g->members.size();
    { DeviceGuard dg(g->members[0]->device); HIPCHK(g, S->lists.reserve(bytes * (size_t)G)); }
    const std::vector<Piece> pieces = {{bytes, S->lists.p}};
    Plan P;
    int rc = plan_call(g, G, pieces, P);
    if (rc) return rc;
    for (int k = 0; k < G && !rc; ++k) {
        DeviceGuard dg(g->members[(size_t)k]->device);
        const hipError_t e = hipMemcpyAsync(piece_at(P, pieces, k, 0), lists[(size_t)k].data(), bytes, hipMemcpyHostToDevice, S->m[(size_t)k].xfer);
        if (e != hipSuccess) rc = fail(g, HPGV_ERR_HIP, "upload of member %d's top lists: %s", k, hipGetErrorString(e));
    }
    if (!rc) rc = hand_over(P, piece_transfers(P, pieces));
    if (!rc) {
        const hipError_t e = quiesce(g, S);
        if (e != hipSuccess) rc = fail(g, HPGV_ERR_HIP, "the gather of the top lists: %s", hipGetErrorString(e));
    }
    if (rc) return drain(P, rc);
    DeviceGuard dg(g->members[0]->device);
    HIPCHK(g, hipMemcpy(all.data(), S->lists.p, bytes * (size_t)G, hipMemcpyDeviceToHost));
    return HPGV_OK;
}

}  // namespace

extern "C" {

int hpgv_group_epi_share(const hpgv_ctx *g, int order, int member, int *i_begin, int *i_end) {
    if (!g || !i_begin || !i_end || order < 2 || order > 5) return HPGV_ERR_INVALID;
    const int G = hpgv_group_size(g);
    if (member < 0 || member >= G) return HPGV_ERR_INVALID;
    const hpgv_ctx *m0 = first_member(g);
    const int V = m0->epi.V, unit = order == 2 ? 64 : 1;
    *i_begin = epi_cut(V, order, G, member, unit);
    *i_end = epi_cut(V, order, G, member + 1, unit);
    return HPGV_OK;
}

int hpgv_group_epi_rank(hpgv_ctx *g, int order, int subset, int max_ranking_size, int32_t *combs_out, double *accuracy,
                        uint32_t *risky_mask, int32_t *n_ranked, float *scan_ms) {
    HPGV_ABI_TRY
    if (!is_group(g)) return fail(g, HPGV_ERR_INVALID, "hpgv_group_epi_rank needs a group context (hpgv_create_multi)");
    if (order < 2 || order > 5) return fail(g, HPGV_ERR_UNSUPPORTED, "combinations of %d SNPs are not supported (2 to 5)", order);
    if (max_ranking_size < 1 || max_ranking_size > 65536 || !combs_out || !accuracy || !risky_mask || !n_ranked)
        return fail(g, HPGV_ERR_INVALID, "bad ranking arguments");
    int rc = hpgv_group_comm_init(g);
    if (rc) return rc;
    GroupState *S = g->grp;
    std::lock_guard<std::mutex> lk(S->mu);
    const int G = (int)g->members.size(), N = max_ranking_size;
    const int nf = g->members[0]->epi.num_folds;
    if (!g->members[0]->epi.have_folds) return fail(g, HPGV_ERR_STATE, "hpgv_epi_set_dataset has not been called");
    for (int k = 1; k < G; ++k)
        if (!g->members[(size_t)k]->epi.have_folds || g->members[(size_t)k]->epi.V != g->members[0]->epi.V || g->members[(size_t)k]->epi.num_folds != nf)
            return fail(g, HPGV_ERR_STATE, "member %d does not hold the dataset and folds of member 0: set them through the group context", k);
    const size_t n_rec = (size_t)nf * (size_t)N;
    // ---- every member ranks its share on a host thread of its own ----
    std::vector<std::vector<EpiModel>> lists((size_t)G);
    std::vector<int> rcs((size_t)G, HPGV_OK);
    std::vector<float> ms((size_t)G, 0.f);
    {
        std::vector<std::thread> th;
        for (int k = 0; k < G; ++k)
            th.emplace_back([&, k]() {
                try {
                    hpgv_ctx *mc = g->members[(size_t)k];
                    int lo = 0, hi = 0;
                    (void)hpgv_group_epi_share(g, order, k, &lo, &hi);
                    float *t_ms = scan_ms ? &ms[(size_t)k] : nullptr;
                    auto &L = lists[(size_t)k];
                    rcs[(size_t)k] = order == 2 ? hpgv_epi_pairs_models(mc, lo, hi, subset, N, true, L, t_ms)
                                   : order == 3 ? hpgv_epi_triples_models(mc, lo, hi, subset, N, true, L, t_ms)
                                                : hpgv_epi_order_models(mc, order, lo, hi, subset, N, true, L, t_ms);
                } catch (...) { rcs[(size_t)k] = HPGV_ERR_NOMEM; }
            });
        for (auto &t : th) t.join();
    }
    for (int k = 0; k < G; ++k)
        if (rcs[(size_t)k]) return fail(g, rcs[(size_t)k], "member %d: %s", k, hpgv_last_error(g->members[(size_t)k]));
    std::vector<EpiModel> all(n_rec * (size_t)G);
    rc = gather_lists(g, lists, n_rec * sizeof(EpiModel), all);
    if (rc) return rc;
    // ---- merge: per fold the best N of the members' lists (add_to_model_ranking, model.c:478-517: higher accuracy, then the
    //      smaller combination) ----
    std::vector<EpiModel> merged(n_rec), t;
    for (int f = 0; f < nf; ++f) {
        t.clear();
        for (int k = 0; k < G; ++k)
            for (int e = 0; e < N; ++e) { const EpiModel &R = all[(size_t)k * n_rec + (size_t)f * (size_t)N + (size_t)e]; if (R.used) t.push_back(R); }
        std::sort(t.begin(), t.end(), epi_better<EpiModel>);
        if ((int)t.size() > N) t.resize((size_t)N);
        std::copy(t.begin(), t.end(), merged.begin() + (size_t)f * (size_t)N);
    }
    int32_t *const comb[5] = {combs_out, combs_out + 1, combs_out + 2, combs_out + 3, combs_out + 4};
    epi_scatter(merged, N, order, comb, (size_t)order, accuracy, risky_mask, hpgv::EPI_MASK_WORDS, n_ranked);
    if (scan_ms) { float m = 0.f; for (float x : ms) m = std::max(m, x); *scan_ms = m; }       // the members scan side by side: the slowest one
    return HPGV_OK;
    HPGV_ABI_CATCH(g)
}

}  // extern "C"
