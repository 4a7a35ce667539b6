// Multi-GPU layer, the communicator half: RCCL over xGMI (bound at run time) or a host-staged callback transport, the host-level
// set-up collectives, and the peer-write all-reduce of a GCR step's scalars.  The row-block partition plan is comm_plan.h; the
// distributed Sparse operator and its halo transports are halo.hip.  The reference is a single-process CPU code:
// everything here is new design for one process per MI355X.  Per GCR iteration: 1 halo exchange per SpMV (halo.hip) and 2 all-reduces
// of a handful of doubles (4, then 1 + 2*lim), in place on device memory, on the compute stream — results never visit the host.
#include <dlfcn.h>

#include <algorithm>

#include "comm_internal.h"
#include "reduce.h"
#include "pw_tail_dev.h"

namespace mgcr {

RcclApi &rccl() { static RcclApi api; return api; }

static int rccl_load() {
    RcclApi &a = rccl();
    if (a.handle) return MGCR_OK;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names) {
        a.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (a.handle) break;
    }
    MGCR_CHECK(a.handle, MGCR_ERR_COMM, "cannot dlopen librccl.so.1: %s", dlerror());
#define SYM(field, name)                                                        \
    a.field = reinterpret_cast<decltype(a.field)>(dlsym(a.handle, name));       \
    MGCR_CHECK(a.field, MGCR_ERR_COMM, "librccl lacks symbol %s", name)
    SYM(GetUniqueId, "ncclGetUniqueId");
    SYM(CommInitRank, "ncclCommInitRank");
    SYM(CommDestroy, "ncclCommDestroy");
    SYM(AllReduce, "ncclAllReduce");
    SYM(Send, "ncclSend");
    SYM(Recv, "ncclRecv");
    SYM(GroupStart, "ncclGroupStart");
    SYM(GroupEnd, "ncclGroupEnd");
    SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    return MGCR_OK;
}

// live communicators: every host synchronisation point that hands distributed results back asks each of them whether a
// peer-write wait timed out since the last look (comm_check_all) — an operator apply, a V-cycle or a nested solve on a
// distributed operator must not return plausible numbers computed from a halo that never arrived
struct LiveComms {
    std::mutex mtx;
    std::vector<Comm *> v;
};
static LiveComms &live_comms() {
    static LiveComms l;
    return l;
}
static void comm_register(Comm *c) {
    std::lock_guard<std::mutex> lk(live_comms().mtx);
    live_comms().v.push_back(c);
}
static void comm_unregister(Comm *c) {
    std::lock_guard<std::mutex> lk(live_comms().mtx);
    auto &v = live_comms().v;
    v.erase(std::remove(v.begin(), v.end(), c), v.end());
}

int comm_device_ready(Comm *c) {
    if (c->comm_stream) return MGCR_OK;
    MGCR_TRY(require_ctx());
    MGCR_HIP(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    MGCR_HIP(hipEventCreateWithFlags(&c->ev_ready, hipEventDisableTiming));
    MGCR_HIP(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
    MGCR_HIP(hipHostMalloc((void **)&c->h_pin, sizeof(double) * 1024, hipHostMallocDefault));
    return MGCR_OK;
}

static int stage_reserve(Comm *c, size_t doubles) {
    if (doubles <= c->d_stage_cap) return MGCR_OK;
    if (c->d_stage) hipFree(c->d_stage);
    c->d_stage = nullptr;
    MGCR_HIP(hipMalloc((void **)&c->d_stage, sizeof(double) * doubles));
    c->d_stage_cap = doubles;
    return MGCR_OK;
}

// ---- host-level collectives (set-up) ----
int comm_allreduce_host(Comm *c, double *buf, int64_t count) {
    if (c->nranks == 1 && !(c->is_rccl && comm_collectives(c))) return MGCR_OK;
    if (!c->is_rccl) {
        int rc = c->allreduce(c->user, buf, count);
        MGCR_CHECK(rc == 0, MGCR_ERR_COMM, "allreduce callback failed (%d)", rc);
        return MGCR_OK;
    }
    MGCR_TRY(comm_device_ready(c));
    MGCR_TRY(stage_reserve(c, (size_t)count));
    hipStream_t st = ctx().stream;
    MGCR_HIP(hipMemcpyAsync(c->d_stage, buf, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, st));
    MGCR_NCCL(rccl().AllReduce(c->d_stage, c->d_stage, (size_t)count, ncclDouble, ncclSum, c->nccl, st));
    MGCR_HIP(hipMemcpyAsync(buf, c->d_stage, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, st));
    MGCR_HIP(hipStreamSynchronize(st));
    return MGCR_OK;
}

int comm_agree(Comm *c, bool *good) {
    double flag = *good ? 0. : 1.;
    MGCR_TRY(comm_allreduce_host(c, &flag, 1));
    *good = flag == 0.;
    return MGCR_OK;
}

int comm_exchange_host(Comm *c, int npeers, const int *peers, const double *const *send, const int64_t *scount, double *const *recv,
                       const int64_t *rcount) {
    if (npeers == 0) return MGCR_OK;
    if (!c->is_rccl) {
        int rc = c->exchange(c->user, npeers, peers, send, scount, recv, rcount);
        MGCR_CHECK(rc == 0, MGCR_ERR_COMM, "exchange callback failed (%d)", rc);
        return MGCR_OK;
    }
    MGCR_TRY(comm_device_ready(c));
    size_t tot = 0;
    for (int p = 0; p < npeers; p++) tot += (size_t)scount[p] + (size_t)rcount[p];
    MGCR_TRY(stage_reserve(c, tot));
    hipStream_t st = ctx().stream;
    std::vector<double *> ds((size_t)npeers), dr((size_t)npeers);
    size_t off = 0;
    for (int p = 0; p < npeers; p++) {
        ds[(size_t)p] = c->d_stage + off; off += (size_t)scount[p];
        dr[(size_t)p] = c->d_stage + off; off += (size_t)rcount[p];
        if (scount[p]) MGCR_HIP(hipMemcpyAsync(ds[(size_t)p], send[p], sizeof(double) * (size_t)scount[p], hipMemcpyHostToDevice, st));
    }
    MGCR_NCCL(rccl().GroupStart());
    for (int p = 0; p < npeers; p++) {
        if (scount[p]) MGCR_NCCL(rccl().Send(ds[(size_t)p], (size_t)scount[p], ncclDouble, peers[p], c->nccl, st));
        if (rcount[p]) MGCR_NCCL(rccl().Recv(dr[(size_t)p], (size_t)rcount[p], ncclDouble, peers[p], c->nccl, st));
    }
    MGCR_NCCL(rccl().GroupEnd());
    for (int p = 0; p < npeers; p++)
        if (rcount[p]) MGCR_HIP(hipMemcpyAsync(recv[p], dr[(size_t)p], sizeof(double) * (size_t)rcount[p], hipMemcpyDeviceToHost, st));
    MGCR_HIP(hipStreamSynchronize(st));
    return MGCR_OK;
}

int ipc_map_peers(Comm *c, void *mine, int n, const int32_t *ranks, void **mapped, bool *good) {
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t size");
    const size_t nr = (size_t)c->nranks;
    hipIpcMemHandle_t h;
    memset(&h, 0, sizeof(h));
    unsigned char *b = reinterpret_cast<unsigned char *>(&h);
    for (int i = 0; i < n; i++) mapped[i] = nullptr;
    *good = false;
    // all-gather of the handles (one double per byte: the set-up all-reduce sums doubles) + "I am fine" count
    std::vector<double> g(nr * 64 + 1, 0.);
    if (mine && hipIpcGetMemHandle(&h, mine) == hipSuccess) {
        for (int i = 0; i < 64; i++) g[(size_t)c->rank * 64 + i] = (double)b[i];
        g[nr * 64] = 1.;
    }
    MGCR_TRY(comm_allreduce_host(c, g.data(), (int64_t)g.size()));
    bool ok = (size_t)g[nr * 64] == nr;
    for (int i = 0; i < n && ok; i++) {
        if (ranks[i] == c->rank) { mapped[i] = mine; continue; }
        for (int k = 0; k < 64; k++) b[k] = (unsigned char)g[(size_t)ranks[i] * 64 + k];
        ok = hipIpcOpenMemHandle(&mapped[i], h, hipIpcMemLazyEnablePeerAccess) == hipSuccess;
        if (!ok) mapped[i] = nullptr;
    }
    (void)hipGetLastError();
    MGCR_TRY(comm_agree(c, &ok));   // nobody writes into a peer's memory before everybody has mapped all it needs
    if (!ok) ipc_unmap(mine, n, mapped);
    *good = ok;
    return MGCR_OK;
}

void ipc_unmap(const void *mine, int n, void **mapped) {
    for (int i = 0; i < n; i++) {
        if (mapped[i] && mapped[i] != mine) hipIpcCloseMemHandle(mapped[i]);
        mapped[i] = nullptr;
    }
}

// ------------------------------------------------------------------------------------------------
// Peer-write all-reduce for the scalars of a GCR step (4, then 1 + 2*lim doubles).
//
// An RCCL all-reduce of a few doubles costs its launch plus a ring/tree protocol, twice per iteration on
// the critical path between dependent kernels.  Here the kernel that folds the workgroup partials (one
// wave per scalar, blas1.hip fold_kernel) also exchanges them: lane j stores the wave's sum straight into
// rank j's mailbox over xGMI and polls its own mailbox for rank j's sum; the wave then adds the values in
// RANK ORDER, so every rank obtains the same bits.  No further launch, no second pass.
//
// Wire format (the "LL" idea: data and flag travel in ONE 8-byte store, which the fabric never tears, so
// no ordering between separate stores is needed): a double goes as two words {lo32 | seq<<32},
// {hi32 | seq<<32}; the receiver spins until both words carry the expected sequence number.  Mailboxes
// are zero-initialised and seq is never 0.  Two slots (seq & 1): a rank finishes all-reduce s only after
// every peer has SENT s, i.e. after every peer finished s-1, so nobody can still be reading the slot that
// s+1 overwrites.  Mailboxes are uncached (fine-grained) device memory shared with hipIpc handles — the
// allocation class RCCL itself uses for its peer buffers.
//
// The path validates itself when the communicator's first distributed operator is created (a few
// all-reduces with known answers, every wait bounded by a wall-clock limit); if any rank fails to map a
// mailbox, times out or sees a wrong sum, ALL ranks fall back to RCCL (or the host transport).
// MGCR_PEER_ALLREDUCE=0 turns it off.
// ------------------------------------------------------------------------------------------------
struct PwPeers {
    uint64_t *mb[PW_MAX_RANKS];
};
constexpr size_t PW_MBOX_WORDS = (size_t)2 * PW_MAX_RANKS * PW_MAX_SCALARS * 2;
long long pw_timeout_run() {
    static const long long ticks = [] {
        long long ms = 20000;
        if (const char *e = getenv("MGCR_PEER_TIMEOUT_MS")) ms = atoll(e);
        ms = ms < 1 ? 1 : ms > 30000 ? 30000 : ms;
        return ms * 100000LL;
    }();
    return ticks;
}

__global__ void __launch_bounds__(64) fold_pw_kernel(const double *__restrict__ pa, int na, const double *__restrict__ pb, int nb,
                                                     double *__restrict__ out, int nblk, PwPeers peers, int rank, int nranks,
                                                     uint32_t seq, int *err, long long timeout) {
    const int k = blockIdx.x, lane = threadIdx.x;
    double acc;
    if (nblk > 0) {  // fold scalar k exactly as fold_kernel does
        const double *src = k < na ? pa + (size_t)k * RED_MAX_BLOCKS : pb + (size_t)(k - na) * RED_MAX_BLOCKS;
        acc = wave_fold_slab(src, nblk);
    } else {
        acc = out[k];  // already folded: all-reduce in place
    }
    const double tot = pw_exchange_scalar(peers.mb, rank, nranks, seq, err, timeout, k, acc);   // (pw_tail_dev.h: shared with the producer kernels' tails)
    if (lane == 0) out[k] = tot;
}

static uint32_t pw_next_seq(Comm *c) {
    c->pw_seq = pw_advance(c->pw_seq);
    return c->pw_seq;
}

static int pw_launch(Comm *c, const double *pa, int na, const double *pb, int nb, double *out, int nblk) {
    PwPeers peers;
    for (int r = 0; r < PW_MAX_RANKS; r++) peers.mb[r] = (uint64_t *)c->pw_peer[r < c->nranks ? r : c->rank];
    hipLaunchKernelGGL(fold_pw_kernel, dim3(na + nb), dim3(64), 0, ctx().stream, pa, na, pb, nb, out, nblk, peers, c->rank, c->nranks,
                       pw_next_seq(c), c->pw_err, c->pw_on ? pw_timeout_run() : PW_TIMEOUT_TEST);
    MGCR_HIP(hipGetLastError());
    return MGCR_OK;
}

// The fold + exchange of a reduction inside the kernel that produces its partials (pw_tail_dev.h)
static EnvSwitch g_pw_tail("MGCR_PW_TAIL");
static int64_t g_pw_tail_count = 0;
bool set_pw_tail_enabled(bool on) { return g_pw_tail.set(on); }
int64_t comm_pw_tail_count() { return g_pw_tail_count; }
bool comm_pw_tail_begin(Comm *c, PwTail *t) {
    if (!c || !c->pw_on || !g_pw_tail.on() || c->nranks < 2) return false;
    if (!c->pw_ticket) {
        if (hipMalloc((void **)&c->pw_ticket, sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); c->pw_ticket = nullptr; return false; }
        if (hipMemsetAsync(c->pw_ticket, 0, sizeof(unsigned), ctx().stream) != hipSuccess) return false;
    }
    for (int r = 0; r < PW_MAX_RANKS; r++) t->mb[r] = (uint64_t *)c->pw_peer[r < c->nranks ? r : c->rank];
    t->rank = c->rank;
    t->nranks = c->nranks;
    t->seq = pw_next_seq(c);
    t->err = c->pw_err;
    t->timeout = pw_timeout_run();
    t->ticket = c->pw_ticket;
    g_pw_tail_count++;
    return true;
}

static void pw_release(Comm *c) {
    ipc_unmap(c->pw_mbox, PW_MAX_RANKS, c->pw_peer);
    if (c->pw_mbox) hipFree(c->pw_mbox);
    c->pw_mbox = nullptr;
    if (c->pw_err) hipHostFree(c->pw_err);
    c->pw_err = nullptr;
    if (c->pw_ticket) hipFree(c->pw_ticket);
    c->pw_ticket = nullptr;
    c->pw_on = false;
}

// self-test: PW_TEST rounds over PW_TEST_N scalars with known sums, through the production kernel
static bool pw_selftest(Comm *c) {
    constexpr int PW_TEST = 6, PW_TEST_N = 33;
    DevBuf<double> d;
    bool good = d.alloc(PW_TEST_N);
    std::vector<double> h((size_t)PW_TEST_N);
    for (int t = 0; t < PW_TEST && good; t++) {
        for (int k = 0; k < PW_TEST_N; k++) h[(size_t)k] = 1.0 / (double)(1 + c->rank + 3 * k + 7 * t);
        good = hipMemcpy(d.p, h.data(), sizeof(double) * PW_TEST_N, hipMemcpyHostToDevice) == hipSuccess;
        if (good) good = pw_launch(c, nullptr, PW_TEST_N, nullptr, 0, d.p, 0) == MGCR_OK;
        if (good) good = hipStreamSynchronize(ctx().stream) == hipSuccess && hipMemcpy(h.data(), d.p, sizeof(double) * PW_TEST_N, hipMemcpyDeviceToHost) == hipSuccess;
        for (int k = 0; k < PW_TEST_N && good; k++) {
            double want = 0.;
            for (int r = 0; r < c->nranks; r++) want += 1.0 / (double)(1 + r + 3 * k + 7 * t);
            good = h[(size_t)k] == want;
        }
        if (good) good = *(volatile int *)c->pw_err == 0;
    }
    if (!good) (void)hipGetLastError();
    return good;
}

// Collective (every rank of the communicator calls it at the same point): map the mailboxes, run the
// self-test, agree on the outcome.  Never fails the caller: on any problem the communicator simply keeps
// its RCCL / host all-reduce.
int comm_pw_setup(Comm *c) {
    if (c->pw_tried) return MGCR_OK;
    c->pw_tried = true;
    if (c->nranks < 2 || c->nranks > PW_MAX_RANKS) return MGCR_OK;
    if (getenv("MGCR_PEER_ALLREDUCE") && atoi(getenv("MGCR_PEER_ALLREDUCE")) == 0) return MGCR_OK;
    MGCR_TRY(comm_device_ready(c));
    // own mailbox: uncached device memory, zeroed BEFORE anybody can learn its handle
    bool ok = hipExtMallocWithFlags((void **)&c->pw_mbox, PW_MBOX_WORDS * sizeof(uint64_t), hipDeviceMallocUncached) == hipSuccess &&
              hipHostMalloc((void **)&c->pw_err, sizeof(int), hipHostMallocMapped) == hipSuccess;
    if (ok) {
        *c->pw_err = 0;
        ok = hipMemset(c->pw_mbox, 0, PW_MBOX_WORDS * sizeof(uint64_t)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    }
    if (!ok) (void)hipGetLastError();
    int32_t ranks[PW_MAX_RANKS];
    for (int r = 0; r < c->nranks; r++) ranks[r] = r;
    bool good = false;
    MGCR_TRY(ipc_map_peers(c, ok ? c->pw_mbox : nullptr, c->nranks, ranks, c->pw_peer, &good));
    if (good) {
        good = pw_selftest(c);
        MGCR_TRY(comm_agree(c, &good));
    }
    if (good) {
        c->pw_on = true;
    } else {
        hipDeviceSynchronize();
        pw_release(c);
        (void)hipGetLastError();
    }
    return MGCR_OK;
}

int comm_nranks(Comm *c) { return c ? c->nranks : 1; }

// does a solve on this communicator go through the fold + all-reduce path?  (MGCR_TEST_FORCE_COLLECTIVES=1
// turns it on for a 1-rank communicator too, so that the RCCL calls can be exercised on a single GPU)
bool comm_collectives(Comm *c) {
    if (!c) return false;
    if (c->nranks > 1) return true;
    static const bool force = getenv("MGCR_TEST_FORCE_COLLECTIVES") && atoi(getenv("MGCR_TEST_FORCE_COLLECTIVES")) != 0;
    return force;
}

// in-place sum over ranks of `count` doubles in device memory, ordered on the compute stream
int comm_allreduce_dev(Comm *c, double *dbuf, int count) {
    if (!c || !comm_collectives(c)) return MGCR_OK;
    hipStream_t st = ctx().stream;
    if (c->pw_on && count <= PW_MAX_SCALARS) return pw_launch(c, nullptr, count, nullptr, 0, dbuf, 0);
    if (c->is_rccl) {
        MGCR_NCCL(rccl().AllReduce(dbuf, dbuf, (size_t)count, ncclDouble, ncclSum, c->nccl, st));
        return MGCR_OK;
    }
    MGCR_TRY(comm_device_ready(c));
    MGCR_CHECK(count <= 1024, MGCR_ERR_UNSUPPORTED, "all-reduce of %d scalars exceeds the staging buffer", count);
    MGCR_HIP(hipMemcpyAsync(c->h_pin, dbuf, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, st));
    MGCR_HIP(hipStreamSynchronize(st));
    MGCR_TRY(comm_allreduce_host(c, c->h_pin, count));
    MGCR_HIP(hipMemcpyAsync(dbuf, c->h_pin, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, st));
    MGCR_HIP(hipStreamSynchronize(st));  // h_pin is reused by the next call
    return MGCR_OK;
}

// out[0..na) = sum over ranks of the folded partials pa, out[na..na+nb) likewise of pb (slabs of RED_MAX_BLOCKS per
// scalar, nblk workgroup partials each; blas1.hip k_fold2): one kernel when the peer-write all-reduce is up
int comm_fold_allreduce(Comm *c, const double *pa, int na, const double *pb, int nb, double *out, int nblk) {
    if (c && c->pw_on && comm_collectives(c) && na + nb <= PW_MAX_SCALARS) return pw_launch(c, pa, na, pb, nb, out, nblk);
    MGCR_TRY(k_fold2(pa, na, out, pb, nb, out + na, nblk));
    return comm_allreduce_dev(c, out, na + nb);
}

// did a peer-write wait time out since the last check?  (called where a distributed solve hands back to the host)
int comm_check(Comm *c) {
    if (c && c->pw_err && *(volatile int *)c->pw_err != 0) {
        *(volatile int *)c->pw_err = 0;
        set_error("peer-write exchange (all-reduce or halo): a rank did not arrive within the time limit; the communicator is no longer usable");
        return MGCR_ERR_COMM;
    }
    return MGCR_OK;
}

int comm_live_count() {
    std::lock_guard<std::mutex> lk(live_comms().mtx);
    return (int)live_comms().v.size();
}
int comm_check_all() {
    std::lock_guard<std::mutex> lk(live_comms().mtx);
    int rc = MGCR_OK;
    for (Comm *c : live_comms().v) {
        int r = comm_check(c);
        if (r != MGCR_OK) rc = r;
    }
    return rc;
}

int comm_allreduce_kind(Comm *c) { return c->pw_on ? 2 : c->is_rccl ? 1 : 0; }

}  // namespace mgcr

using namespace mgcr;

#define LOCK() std::lock_guard<std::recursive_mutex> lk__(ctx().mtx)

extern "C" {

int mgcr_rccl_unique_id(void *id128) {
    MGCR_CHECK(id128, MGCR_ERR_INVALID, "null id buffer");
    MGCR_TRY(rccl_load());
    ncclUniqueId id;
    MGCR_NCCL(rccl().GetUniqueId(&id));
    static_assert(sizeof(id) == MGCR_RCCL_ID_BYTES, "ncclUniqueId size");
    memcpy(id128, &id, sizeof(id));
    return MGCR_OK;
}

int mgcr_comm_create_rccl(int rank, int nranks, const void *id128, mgcr_comm_t *out) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(out && id128 && nranks >= 1 && rank >= 0 && rank < nranks, MGCR_ERR_INVALID, "mgcr_comm_create_rccl: bad argument");
    MGCR_TRY(rccl_load());
    LOCK();
    mgcr_comm_s *c = new mgcr_comm_s();
    c->rank = rank; c->nranks = nranks; c->is_rccl = true;
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclResult_t r = rccl().CommInitRank(&c->nccl, nranks, id, rank);
    if (r != ncclSuccess) {
        set_error("ncclCommInitRank failed: %s", rccl().GetErrorString(r));
        delete c;
        return MGCR_ERR_COMM;
    }
    int rc = comm_device_ready(c);
    if (rc != MGCR_OK) { delete c; return rc; }
    c->pw_seq = pw_seq0();
    comm_register(c);
    *out = c;
    return MGCR_OK;
}

int mgcr_comm_create_host(int rank, int nranks, mgcr_allreduce_cb allreduce, mgcr_exchange_cb exchange, void *user, mgcr_comm_t *out) {
    MGCR_CHECK(out && nranks >= 1 && rank >= 0 && rank < nranks && (nranks == 1 || (allreduce && exchange)), MGCR_ERR_INVALID,
               "mgcr_comm_create_host: bad argument");
    mgcr_comm_s *c = new mgcr_comm_s();
    c->rank = rank; c->nranks = nranks; c->is_rccl = false;
    c->allreduce = allreduce; c->exchange = exchange; c->user = user;
    c->pw_seq = pw_seq0();
    comm_register(c);
    *out = c;
    return MGCR_OK;
}

int mgcr_comm_allreduce_sum(mgcr_comm_t c, double *buf, int32_t count) {
    MGCR_CHECK(c && buf && count > 0, MGCR_ERR_INVALID, "mgcr_comm_allreduce_sum: bad argument");
    return comm_allreduce_host(c, buf, count);
}

int mgcr_comm_allreduce_kind(mgcr_comm_t c, int32_t *kind) {
    MGCR_CHECK(c && kind, MGCR_ERR_INVALID, "mgcr_comm_allreduce_kind: null argument");
    *kind = comm_allreduce_kind(c);
    return MGCR_OK;
}

int mgcr_comm_bench_allreduce(mgcr_comm_t c, int32_t count, int32_t reps, double *us_avg) {
    MGCR_CHECK(c && count > 0 && count <= 64 && reps > 0 && us_avg, MGCR_ERR_INVALID, "mgcr_comm_bench_allreduce: bad argument");
    MGCR_TRY(require_ctx());
    MGCR_TRY(comm_pw_setup(c));
    Context &cx = ctx();
    DevBuf<double> d;
    MGCR_HIP(d.malloc(64));
    MGCR_HIP(hipMemsetAsync(d.p, 0, sizeof(double) * 64, cx.stream));
    int rc = comm_allreduce_dev(c, d.p, count);  // warm-up
    MGCR_HIP(hipEventRecord(cx.ev0, cx.stream));
    for (int i = 0; i < reps && rc == MGCR_OK; i++) rc = comm_allreduce_dev(c, d.p, count);
    MGCR_HIP(hipEventRecord(cx.ev1, cx.stream));
    MGCR_HIP(hipEventSynchronize(cx.ev1));
    float ms = 0.f;
    hipEventElapsedTime(&ms, cx.ev0, cx.ev1);
    *us_avg = 1e3 * (double)ms / reps;
    if (rc == MGCR_OK) rc = comm_check(c);
    return rc;
}

int mgcr_comm_destroy(mgcr_comm_t c) {
    if (!c) return MGCR_OK;
    comm_unregister(c);
    if (ctx().ready) {
        hipStreamSynchronize(ctx().stream);
        if (c->comm_stream) hipStreamSynchronize(c->comm_stream);
    }
    pw_release(c);
    if (c->is_rccl && c->nccl) rccl().CommDestroy(c->nccl);
    if (c->comm_stream) hipStreamDestroy(c->comm_stream);
    if (c->ev_ready) hipEventDestroy(c->ev_ready);
    if (c->ev_done) hipEventDestroy(c->ev_done);
    if (c->d_stage) hipFree(c->d_stage);
    if (c->h_pin) hipHostFree(c->h_pin);
    delete c;
    return MGCR_OK;
}

}  // extern "C"
