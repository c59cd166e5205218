// fake_rccl.hip -- a stand-in communicator for the group hand-over tests (libfake_rccl.so, loaded through HPGV_RCCL_LIB).
//
// It exports the nine RCCL entry points libhpgv.so resolves (RCCL_SYMBOLS in csrc/hpgv_group_capi.hip) and nothing else,
// written from RCCL's public API: one process, ncclCommInitAll, point-to-point and reduce calls inside ncclGroupStart /
// ncclGroupEnd.  Unlike RCCL it accepts a device list that names one device several times, so a one-GPU box can run the
// exchange logic at several ranks.
//
// It never blocks the host: stream operations and events only.  Calls are RECORDED until the outermost ncclGroupEnd, which
// checks the whole group first -- every send meets a receive of the same count and datatype between the same two ranks (in
// order of issue), every rank of a world takes part in a reduce exactly once with the same count and root -- and queues
// nothing unless all of it fits.  Where RCCL would wait for a peer that never comes, this returns ncclInvalidUsage.
//
// $FAKE_RCCL_LOG: when the last communicator of a world is destroyed, one line with the world's totals is appended,
//   ranks=<n> sends=<n> send_bytes=<n> reduces=<n> reduce_elems=<n>
// (sends: matched pairs carried out; reduces: ncclReduce calls carried out, one per rank; reduce_elems: their counts).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

// the public types, values as in rccl.h
typedef struct ncclComm *ncclComm_t;
typedef enum { ncclSuccess = 0, ncclUnhandledCudaError = 1, ncclSystemError = 2, ncclInternalError = 3, ncclInvalidArgument = 4,
               ncclInvalidUsage = 5, ncclRemoteError = 6, ncclInProgress = 7 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclUint8 = 1, ncclInt32 = 2, ncclUint32 = 3, ncclInt64 = 4, ncclUint64 = 5, ncclFloat16 = 6,
               ncclFloat32 = 7, ncclFloat64 = 8, ncclBfloat16 = 9 } ncclDataType_t;
typedef enum { ncclSum = 0, ncclProd = 1, ncclMax = 2, ncclMin = 3, ncclAvg = 4 } ncclRedOp_t;

struct World {
    int n = 0, alive = 0;
    unsigned long long sends = 0, send_bytes = 0, reduces = 0, reduce_elems = 0;
};

struct ncclComm {
    World *w;
    int rank, dev;
    hipEvent_t arrived, finished;       // "my stream has reached the call" / "what I carried out on my stream is done"
};

namespace {

enum class Kind { send, recv, reduce };

struct Op {
    Kind kind;
    ncclComm *c;
    int peer;                           // send: to, recv: from, reduce: root
    const void *src;
    void *dst;
    size_t count;
    ncclDataType_t type;
    hipStream_t st;
    bool met = false;
};

std::mutex g_mu;                        // the worlds' counters and lifetimes
thread_local int t_depth = 0;           // open ncclGroupStart calls of this thread
thread_local ncclResult_t t_err = ncclSuccess;
thread_local std::vector<Op> t_ops;

size_t size_of(ncclDataType_t t) {
    switch (t) {
    case ncclInt8: case ncclUint8: return 1;
    case ncclFloat16: case ncclBfloat16: return 2;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    }
    return 0;
}

__global__ void k_fake_add_i32(int32_t *__restrict__ dst, const int32_t *__restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] += src[i];
}

struct OnDevice {
    int prev = -1;
    bool ok;
    explicit OnDevice(int dev) { ok = hipGetDevice(&prev) == hipSuccess && (prev == dev || hipSetDevice(dev) == hipSuccess); }
    ~OnDevice() { if (prev >= 0) (void)hipSetDevice(prev); }
};

#define HIP_OR_FAIL(call) do { if ((call) != hipSuccess) return ncclUnhandledCudaError; } while (0)

// stream `waiter` (on w's device) goes on only after what is queued on `st` (c's stream) now
ncclResult_t after(ncclComm *c, hipEvent_t ev, hipStream_t st, ncclComm *w, hipStream_t waiter) {
    { OnDevice d(c->dev); if (!d.ok) return ncclUnhandledCudaError; HIP_OR_FAIL(hipEventRecord(ev, st)); }
    OnDevice d(w->dev);
    if (!d.ok) return ncclUnhandledCudaError;
    HIP_OR_FAIL(hipStreamWaitEvent(waiter, ev, 0));
    return ncclSuccess;
}

ncclResult_t carry_pair(const Op &s, const Op &r) {
    const size_t bytes = s.count * size_of(s.type);
    const bool one_stream = s.st == r.st && s.c->dev == r.c->dev;
    if (!one_stream) if (ncclResult_t e = after(s.c, s.c->arrived, s.st, r.c, r.st)) return e;
    if (bytes) {
        OnDevice d(r.c->dev);
        if (!d.ok) return ncclUnhandledCudaError;
        HIP_OR_FAIL(hipMemcpyAsync(r.dst, s.src, bytes, hipMemcpyDeviceToDevice, r.st));
    }
    if (!one_stream) if (ncclResult_t e = after(r.c, r.c->finished, r.st, s.c, s.st)) return e;
    std::lock_guard<std::mutex> lk(g_mu);
    s.c->w->sends += 1;
    s.c->w->send_bytes += bytes;
    return ncclSuccess;
}

// `ops`: the reduce calls of one world, one per rank
ncclResult_t carry_reduce(const std::vector<const Op *> &ops) {
    const Op *root = nullptr;
    for (const Op *o : ops) if (o->c->rank == o->peer) root = o;
    for (const Op *o : ops)
        if (o != root && !(o->st == root->st && o->c->dev == root->c->dev))
            if (ncclResult_t e = after(o->c, o->c->arrived, o->st, root->c, root->st)) return e;
    {
        OnDevice d(root->c->dev);
        if (!d.ok) return ncclUnhandledCudaError;
        if (root->count && root->dst != root->src)
            HIP_OR_FAIL(hipMemcpyAsync(root->dst, root->src, root->count * sizeof(int32_t), hipMemcpyDeviceToDevice, root->st));
        for (const Op *o : ops) {
            if (o == root || !root->count) continue;
            const unsigned blocks = (unsigned)std::min<size_t>((root->count + 255) / 256, 4096);
            hipLaunchKernelGGL(k_fake_add_i32, dim3(blocks), dim3(256), 0, root->st, (int32_t *)root->dst, (const int32_t *)o->src, root->count);
            HIP_OR_FAIL(hipGetLastError());
        }
    }
    for (const Op *o : ops)
        if (o != root && !(o->st == root->st && o->c->dev == root->c->dev))
            if (ncclResult_t e = after(root->c, root->c->finished, root->st, o->c, o->st)) return e;
    std::lock_guard<std::mutex> lk(g_mu);
    root->c->w->reduces += ops.size();
    root->c->w->reduce_elems += ops.size() * root->count;
    return ncclSuccess;
}

// the recorded group: checked as a whole, then carried out.  Nothing is queued unless everything fits.
ncclResult_t end_group(std::vector<Op> &ops) {
    std::vector<std::pair<const Op *, const Op *>> pairs;
    for (Op &s : ops) {
        if (s.kind != Kind::send) continue;
        for (Op &r : ops) {             // the first receive not yet met between the same two ranks: order of issue
            if (r.kind != Kind::recv || r.met || r.c->w != s.c->w || r.c->rank != s.peer || r.peer != s.c->rank) continue;
            if (r.count != s.count || r.type != s.type) return ncclInvalidUsage;
            r.met = s.met = true;
            pairs.push_back({&s, &r});
            break;
        }
        if (!s.met) return ncclInvalidUsage;
    }
    for (const Op &r : ops) if (r.kind == Kind::recv && !r.met) return ncclInvalidUsage;
    std::vector<std::vector<const Op *>> reduces;
    for (const Op &o : ops) {
        if (o.kind != Kind::reduce) continue;
        std::vector<const Op *> *mine = nullptr;
        for (auto &v : reduces) if (v[0]->c->w == o.c->w) mine = &v;
        if (!mine) { reduces.emplace_back(); mine = &reduces.back(); }
        for (const Op *p : *mine) if (p->c->rank == o.c->rank || p->count != o.count || p->peer != o.peer) return ncclInvalidUsage;
        mine->push_back(&o);
    }
    for (const auto &v : reduces) if ((int)v.size() != v[0]->c->w->n) return ncclInvalidUsage;
    for (const auto &p : pairs) if (ncclResult_t e = carry_pair(*p.first, *p.second)) return e;
    for (const auto &v : reduces) if (ncclResult_t e = carry_reduce(v)) return e;
    return ncclSuccess;
}

// a call's verdict: inside a group the first error is also the group's
ncclResult_t said(ncclResult_t r) {
    if (r != ncclSuccess && t_depth > 0 && t_err == ncclSuccess) t_err = r;
    return r;
}

}  // namespace

extern "C" {

ncclResult_t ncclCommInitAll(ncclComm_t *comms, int ndev, const int *devlist) {
    if (!comms || ndev < 1) return ncclInvalidArgument;
    int have = 0;
    if (hipGetDeviceCount(&have) != hipSuccess) return ncclUnhandledCudaError;
    for (int r = 0; r < ndev; ++r) if (devlist && (devlist[r] < 0 || devlist[r] >= have)) return ncclInvalidArgument;
    if (!devlist && ndev > have) return ncclInvalidArgument;
    World *w = new World();
    w->n = ndev;
    for (int r = 0; r < ndev; ++r) comms[r] = nullptr;
    for (int r = 0; r < ndev; ++r) {
        ncclComm *c = new ncclComm{w, r, devlist ? devlist[r] : r, nullptr, nullptr};
        OnDevice d(c->dev);
        const bool ok = d.ok && hipEventCreateWithFlags(&c->arrived, hipEventDisableTiming) == hipSuccess &&
                        hipEventCreateWithFlags(&c->finished, hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            if (c->arrived) (void)hipEventDestroy(c->arrived);
            delete c;
            for (int q = 0; q < r; ++q) { (void)hipEventDestroy(comms[q]->arrived); (void)hipEventDestroy(comms[q]->finished); delete comms[q]; comms[q] = nullptr; }
            delete w;
            return ncclUnhandledCudaError;
        }
        comms[r] = c;
        w->alive += 1;
    }
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
    if (!comm) return ncclInvalidArgument;
    World *w = comm->w;
    { OnDevice d(comm->dev); (void)hipEventDestroy(comm->arrived); (void)hipEventDestroy(comm->finished); }
    delete comm;
    std::lock_guard<std::mutex> lk(g_mu);
    if (--w->alive > 0) return ncclSuccess;
    const char *path = getenv("FAKE_RCCL_LOG");
    if (path && *path) {
        if (FILE *f = fopen(path, "a")) {
            fprintf(f, "ranks=%d sends=%llu send_bytes=%llu reduces=%llu reduce_elems=%llu\n", w->n, w->sends, w->send_bytes, w->reduces, w->reduce_elems);
            fclose(f);
        }
    }
    delete w;
    return ncclSuccess;
}

ncclResult_t ncclCommCount(const ncclComm_t comm, int *count) {
    if (!comm || !count) return ncclInvalidArgument;
    *count = comm->w->n;
    return ncclSuccess;
}

const char *ncclGetErrorString(ncclResult_t result) {
    switch (result) {
    case ncclSuccess: return "no error";
    case ncclUnhandledCudaError: return "unhandled HIP error";
    case ncclSystemError: return "unhandled system error";
    case ncclInternalError: return "internal error";
    case ncclInvalidArgument: return "invalid argument";
    case ncclInvalidUsage: return "invalid usage (stand-in: RCCL would wait for a peer that never comes)";
    case ncclRemoteError: return "remote process exited or there was a network error";
    case ncclInProgress: return "operation in progress";
    }
    return "unknown result code";
}

ncclResult_t ncclGroupStart(void) {
    if (t_depth++ == 0) { t_err = ncclSuccess; t_ops.clear(); }
    return ncclSuccess;
}

ncclResult_t ncclGroupEnd(void) {
    if (t_depth == 0) return ncclInvalidUsage;
    if (--t_depth > 0) return ncclSuccess;
    ncclResult_t r = t_err;
    try {
        if (r == ncclSuccess) r = end_group(t_ops);
    } catch (...) { r = ncclSystemError; }
    t_ops.clear();
    t_err = ncclSuccess;
    return r;
}

static ncclResult_t record(Kind kind, const void *src, void *dst, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t st) {
    // (a reduce's receive buffer matters at the root only)
    const bool reads = kind != Kind::recv, writes = kind == Kind::recv || (kind == Kind::reduce && comm && comm->rank == peer);
    if (!comm || peer < 0 || peer >= comm->w->n || !size_of(type) || (count && ((reads && !src) || (writes && !dst))))
        return said(ncclInvalidArgument);
    try {
        t_ops.push_back(Op{kind, comm, peer, src, dst, count, type, st});
    } catch (...) { return said(ncclSystemError); }
    return ncclSuccess;
}

ncclResult_t ncclSend(const void *sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream) {
    if (t_depth == 0) return ncclInvalidUsage;     // alone it would wait for its receive: RCCL blocks here
    return record(Kind::send, sendbuff, nullptr, count, datatype, peer, comm, stream);
}

ncclResult_t ncclRecv(void *recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream) {
    if (t_depth == 0) return ncclInvalidUsage;
    return record(Kind::recv, nullptr, recvbuff, count, datatype, peer, comm, stream);
}

ncclResult_t ncclReduce(const void *sendbuff, void *recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op, int root,
                        ncclComm_t comm, hipStream_t stream) {
    if (datatype != ncclInt32 || op != ncclSum) return said(ncclInvalidArgument);
    if (t_depth > 0) return record(Kind::reduce, sendbuff, recvbuff, count, datatype, root, comm, stream);
    // outside a group: a group of this one call -- complete in a world of one rank only
    (void)ncclGroupStart();
    (void)record(Kind::reduce, sendbuff, recvbuff, count, datatype, root, comm, stream);
    return ncclGroupEnd();
}

}  // extern "C"
