// Multi-GPU layer, the operator half: the collectives that build a row-block partition plan (its arithmetic is comm_plan.h), the
// distributed Sparse / HierarchicalSparse operator state, and the three halo transports — peer-write kernels, ncclSend/ncclRecv
// pairs inside one group, host-staged callbacks.  One halo exchange per SpMV, overlapped with the rows that touch no remote column.
// The communicator and the set-up collectives are comm.hip.
#include <algorithm>
#include <memory>

#include "comm_internal.h"

namespace mgcr {

#define PLAN_STAGE(code, call) do { const std::string e__ = (call); MGCR_CHECK(e__.empty(), (code), "%s", e__.c_str()); } while (0)

// Collective: comm_plan.h's stages with the collectives between them.  The plan is the caller's (mgcr_plan_destroy, or
// dist_attach, which hands it to the DistCsr).
static int plan_build(Comm *c, int64_t n_global, int64_t row0, int64_t nloc, const int64_t *rowptr, const int64_t *col,
                      std::unique_ptr<Plan> *out) {
    MGCR_CHECK(c, MGCR_ERR_INVALID, "mgcr_plan_create: bad row block");
    auto P = std::make_unique<Plan>();
    P->comm = c;
    const size_t R = (size_t)c->nranks, rank = (size_t)c->rank;
    PLAN_STAGE(MGCR_ERR_INVALID, plan_begin(*P, n_global, row0, nloc, rowptr));
    std::vector<double> tmp(R, 0.);   // row offsets of all ranks
    tmp[rank] = (double)row0;
    MGCR_TRY(comm_allreduce_host(c, tmp.data(), (int64_t)R));
    PLAN_STAGE(MGCR_ERR_INVALID, plan_offsets(*P, tmp.data(), (int)R));
    std::vector<double> M(R * R, 0.);   // counts matrix: M[r][q] = number of entries rank r needs from rank q
    PLAN_STAGE(MGCR_ERR_INVALID, plan_remote(*P, col, M.data() + rank * R));
    MGCR_TRY(comm_allreduce_host(c, M.data(), (int64_t)(R * R)));
    plan_peers(*P, M.data(), (int)R, (int)rank);
    // tell every peer which of its rows I need (global ids, sent as bit patterns in doubles)
    HostExchange ex;
    for (size_t p = 0; p < P->peers.size(); p++)
        ex.add(reinterpret_cast<const double *>(P->halo_gid.data() + P->recv_off[p]), P->recv_count[p],
               reinterpret_cast<double *>(P->send_rows[p].data()), (int64_t)P->send_rows[p].size());
    MGCR_TRY(ex.run(c, P->peers));
    PLAN_STAGE(MGCR_ERR_COMM, plan_send_rows(*P));
    plan_columns(*P, rowptr, col);
    *out = std::move(P);
    return MGCR_OK;
}

// ---- distributed operator state ----
struct DistCsr {
    Comm *comm = nullptr;      // borrowed
    Plan *plan = nullptr;      // owned (dist_free)
    cplx *xh = nullptr;        // halo segment [n_halo]
    cplx *sendbuf = nullptr;   // packed send data (all peers)
    int32_t *send_idx = nullptr;
    SendLists send;            // per peer: its part of send_idx / sendbuf, or the contiguous range of x that needs no packing
    std::vector<double> h_send, h_recv;  // host staging (callback transport)
    // peer-write halo exchange (below): receive slots mapped into the neighbours
    bool pw_on = false;
    unsigned char *pw_rx = nullptr;        // own receive buffer (comm_plan.h PwRxLayout; uncached, hipIpc)
    std::vector<void *> pw_peer_rx;        // per peer: its pw_rx as mapped here
    struct HaloPwPeer *pw_tab = nullptr;   // device table, one entry per peer
    int *pw_ticket = nullptr;              // device: workgroups of the running exchange that have stored their rows
    uint32_t pw_seq = 0;
    unsigned pw_grid_x = 1;
    long long pw_timeout = 0;              // of the exchange begun last: its wait half (dist_halo_end) takes the same one
    bool pw_wait_pending = false;          // a split exchange has stored and published; its wait kernel is still to be launched (dist_halo_end)
};

static EnvSwitch g_halo_overlap("MGCR_HALO_OVERLAP", false);
bool dist_halo_overlaps() { return g_halo_overlap.on(); }

__global__ void __launch_bounds__(256) pack_kernel(int64_t n, const int32_t *__restrict__ idx, const cplx *__restrict__ x,
                                                   cplx *__restrict__ out, const int *__restrict__ skip, int skip_it) {
    if (skip && skip[0] < skip[1] + skip_it) return;  // {stop_at, base}: see gcr.hip DevState
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = x[idx[i]];
}

// ------------------------------------------------------------------------------------------------
// Peer-write halo exchange.  With RCCL one exchange is an ncclSend/ncclRecv group: a kernel launch plus
// its handshake on the critical path of every operator apply, for a payload of one grid plane
// (262 KB at 128^3).  Here ONE kernel does it: its workgroups store this rank's boundary rows straight
// into the neighbours' receive slots over xGMI (plain 16-byte stores into uncached, hipIpc-mapped memory),
// fence, and take a ticket; the last workgroup then publishes the sequence number in every neighbour's
// flag word (release, system scope) and waits — bounded — for the neighbours' flags in its own.  When the
// kernel retires the halo has arrived, and the apply kernel reads it in place from the receive slot.
// Two slots (seq & 1): a neighbour publishes s+1 only after its apply s has run (stream order), and this
// rank starts s+2 only after it has seen the neighbour's s+1, so the slot that s+2 overwrites is free.
// The peer lists are symmetric (A lists B iff B lists A: one's send is the other's receive).
// Validated by a self-test at dist_csr_create (global row numbers through both slots); on any failure
// all ranks keep the RCCL / host exchange.  MGCR_PEER_HALO=0 turns it off.
// ------------------------------------------------------------------------------------------------
struct HaloPwPeer {
    cplx *dst[2];                 // where this rank's rows land in the peer's receive slots
    uint64_t *flag_remote[2];     // the peer's flag word for this rank
    const uint64_t *flag_local[2];  // this rank's flag word for the peer
    int64_t send_off, send_cnt;   // this rank's send list for the peer (send_idx)
    cplx *rx_local[2];            // where the peer's rows land in this rank's receive slots ...
    int64_t recv_cnt;             // ... and how many: poisoned with NaN when the peer never arrives
};

// what the last workgroup of an exchange (or the wait kernel) does for peer q: wait — bounded — for the neighbour's flag
__device__ __forceinline__ void halo_pw_wait_peer(const HaloPwPeer &q, int slot, uint32_t seq, int *err, long long timeout) {
    const long long t0 = wall_clock64();
    bool ok = false;
    if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) {
        for (;;) {
            if (__hip_atomic_load(q.flag_local[slot], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) == (uint64_t)seq) { ok = true; break; }
            if (wall_clock64() - t0 > timeout) break;
            __builtin_amdgcn_s_sleep(2);
        }
    }
    if (!ok) {
        // the neighbour never published: flag it (every host synchronisation point turns the flag into MGCR_ERR_COMM,
        // comm_check_all) and poison the rows it owed with NaN, as the all-reduce does with its sums — a missed
        // check must not be able to yield plausible numbers from a stale or half-written slot
        __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int64_t i = 0; i < q.recv_cnt; i++) q.rx_local[slot][i] = make_double2(nan, nan);
    }
}

// WAIT = false: the exchange is SPLIT — this kernel stores and publishes, and halo_pw_wait_kernel, launched after the rows
// that need no halo have been multiplied, waits for the neighbours (spmv.hip csr_apply_t): the wait — the neighbour's own
// kernels plus the link — then overlaps with the interior rows instead of preceding them.  Same protocol: the wait kernel is
// never skipped and precedes this rank's next exchange in stream order, so every exchange remains a rendezvous.
template <bool WAIT>
__global__ void __launch_bounds__(256) halo_pw_kernel(const HaloPwPeer *__restrict__ tab, int npeer, const int32_t *__restrict__ idx,
                                                      const cplx *__restrict__ x, uint32_t seq, int *ticket, int *err, long long timeout) {
    const int p = blockIdx.y, slot = (int)(seq & 1u);
    const HaloPwPeer pe = tab[p];
    cplx *dst = pe.dst[slot];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pe.send_cnt; i += (int64_t)gridDim.x * 256)
        dst[i] = x[idx[pe.send_off + i]];
    __threadfence_system();   // this thread's remote stores have landed
    __syncthreads();
    __shared__ int last;
    if (threadIdx.x == 0) last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (int)(gridDim.x * gridDim.y) - 1;
    __syncthreads();
    if (!last) return;
    // every workgroup's rows are in place: publish, then wait for the neighbours
    if ((int)threadIdx.x < npeer) {
        const HaloPwPeer q = tab[threadIdx.x];
        __hip_atomic_store(q.flag_remote[slot], (uint64_t)seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        if (WAIT) halo_pw_wait_peer(q, slot, seq, err, timeout);
    }
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// second half of a split exchange: one wave, lane p waits for peer p
__global__ void __launch_bounds__(64) halo_pw_wait_kernel(const HaloPwPeer *__restrict__ tab, int npeer, uint32_t seq, int *err, long long timeout) {
    if ((int)threadIdx.x < npeer) halo_pw_wait_peer(tab[threadIdx.x], (int)(seq & 1u), seq, err, timeout);
}

__global__ void __launch_bounds__(256) halo_test_fill_kernel(cplx *x, int64_t n, int64_t row0, double im) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = make_double2((double)(row0 + i), im);
}

static PwRxLayout halo_pw_layout(const DistCsr *d) { return PwRxLayout{pw_rx_slot_bytes(d->plan->halo_gid.size()), PW_MAX_RANKS}; }

static const cplx *halo_pw_slot(const DistCsr *d, uint32_t seq) { return reinterpret_cast<const cplx *>(d->pw_rx + halo_pw_layout(d).slot((int)(seq & 1u))); }

// MGCR_HALO_SPLIT=0 / mgcr_set_option("halo_split", 0): the stand-alone apply waits for its halo before any row, as the fused GCR steps do
static EnvSwitch g_halo_split("MGCR_HALO_SPLIT");
bool set_halo_split(bool on) { return g_halo_split.set(on); }
static int halo_pw_launch(DistCsr *d, const cplx *x, bool split = false) {
    Comm *c = d->comm;
    const int np = (int)d->plan->peers.size();
    MGCR_CHECK(np <= 64, MGCR_ERR_UNSUPPORTED, "peer-write halo exchange: at most 64 neighbours");
    d->pw_seq = pw_advance(d->pw_seq);
    d->pw_timeout = d->pw_on ? pw_timeout_run() : PW_TIMEOUT_TEST;
    split = split && g_halo_split.on();
    dispatch_bool(!split, [&](auto WAIT) -> int {
        hipLaunchKernelGGL(halo_pw_kernel<decltype(WAIT)::value>, dim3(d->pw_grid_x, (unsigned)np), dim3(256), 0, ctx().stream,
                           (const HaloPwPeer *)d->pw_tab, np, (const int32_t *)d->send_idx, x, d->pw_seq, d->pw_ticket, c->pw_err, d->pw_timeout);
        return MGCR_OK;
    });
    MGCR_HIP(hipGetLastError());
    d->pw_wait_pending = split;
    return MGCR_OK;
}
static int64_t g_halo_split_count = 0;
int64_t dist_halo_split_count() { return g_halo_split_count; }

static void halo_pw_release(DistCsr *d) {
    ipc_unmap(d->pw_rx, (int)d->pw_peer_rx.size(), d->pw_peer_rx.data());
    d->pw_peer_rx.clear();
    hipFree(d->pw_rx); hipFree(d->pw_tab); hipFree(d->pw_ticket);
    d->pw_rx = nullptr; d->pw_tab = nullptr; d->pw_ticket = nullptr;
    d->pw_on = false;
}

// the device table: where this rank's rows and flag land in each neighbour's buffer (laid out by ITS slot size:
// theirs[2 p] = where my rows start in its halo segment, theirs[2 p + 1] = its slot_bytes) and where the neighbour's land here
static bool halo_pw_fill_table(DistCsr *d, const std::vector<double> &theirs) {
    const Plan *P = d->plan;
    const PwRxLayout L = halo_pw_layout(d);
    std::vector<HaloPwPeer> tab(P->peers.size());
    int64_t max_cnt = 0;
    for (size_t p = 0; p < tab.size(); p++) {
        const PwRxLayout Lp{(size_t)theirs[2 * p + 1], PW_MAX_RANKS};
        unsigned char *rb = (unsigned char *)d->pw_peer_rx[p];
        HaloPwPeer &e = tab[p];
        for (int sl = 0; sl < 2; sl++) {
            e.dst[sl] = reinterpret_cast<cplx *>(rb + Lp.slot(sl)) + (int64_t)theirs[2 * p];
            e.flag_remote[sl] = reinterpret_cast<uint64_t *>(rb + Lp.flag(sl, d->comm->rank));
            e.flag_local[sl] = reinterpret_cast<const uint64_t *>(d->pw_rx + L.flag(sl, P->peers[p]));
            e.rx_local[sl] = reinterpret_cast<cplx *>(d->pw_rx + L.slot(sl)) + P->recv_off[p];
        }
        e.send_off = d->send.off[p]; e.send_cnt = d->send.cnt[p]; e.recv_cnt = P->recv_count[p];
        max_cnt = std::max(max_cnt, e.send_cnt);
    }
    d->pw_grid_x = (unsigned)std::min<int64_t>(std::max<int64_t>((max_cnt + 255) / 256, 1), 1024);
    return hipMemcpy(d->pw_tab, tab.data(), sizeof(HaloPwPeer) * tab.size(), hipMemcpyHostToDevice) == hipSuccess;
}

// self-test through both slots: x holds the global row numbers, the halo must then hold halo_gid
static bool halo_pw_selftest(DistCsr *d) {
    const Plan *P = d->plan;
    const size_t nh = P->halo_gid.size();
    DevBuf<cplx> xt;
    bool good = xt.alloc((size_t)std::max<int64_t>(P->nloc, 1));
    std::vector<cplx> got(nh);
    for (int t = 0; t < 2 && good; t++) {
        const double im = 0.5 + t;
        if (P->nloc) hipLaunchKernelGGL(halo_test_fill_kernel, dim3((unsigned)((P->nloc + 255) / 256)), dim3(256), 0, ctx().stream, xt.p, P->nloc, P->row0, im);
        good = halo_pw_launch(d, xt.p) == MGCR_OK && hipStreamSynchronize(ctx().stream) == hipSuccess;
        if (good && nh) good = hipMemcpy(got.data(), halo_pw_slot(d, d->pw_seq), sizeof(cplx) * nh, hipMemcpyDeviceToHost) == hipSuccess;
        for (size_t j = 0; j < nh && good; j++) good = got[j].x == (double)P->halo_gid[j] && got[j].y == im;
        if (good) good = *(volatile int *)d->comm->pw_err == 0;
    }
    if (!good) (void)hipGetLastError();
    return good;
}

// Collective over the communicator, called by dist_attach once the send lists are on the device.
// Never fails the caller for a transport reason: on any problem every rank keeps the RCCL / host exchange.
static int halo_pw_setup(DistCsr *d) {
    Comm *c = d->comm;
    Plan *P = d->plan;
    if (!c->pw_on) return MGCR_OK;   // same mechanism as the peer-write all-reduce: only where that one validated
    if (getenv("MGCR_PEER_HALO") && atoi(getenv("MGCR_PEER_HALO")) == 0) return MGCR_OK;
    const size_t np = P->peers.size();
    const PwRxLayout L = halo_pw_layout(d);
    // own receive buffer: uncached device memory, zeroed BEFORE anybody can learn its handle
    bool ok = hipExtMallocWithFlags((void **)&d->pw_rx, L.total(), hipDeviceMallocUncached) == hipSuccess;
    if (ok) ok = hipMemset(d->pw_rx, 0, L.total()) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (ok) ok = hipMalloc((void **)&d->pw_ticket, sizeof(int)) == hipSuccess && hipMemset(d->pw_ticket, 0, sizeof(int)) == hipSuccess;
    if (ok && np) ok = hipMalloc((void **)&d->pw_tab, sizeof(HaloPwPeer) * np) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    // every neighbour learns where its rows start in my halo segment and my slot size (my flag block follows from that)
    std::vector<double> mine(2 * np), theirs(2 * np, 0.);
    HostExchange ex;
    for (size_t p = 0; p < np; p++) {
        mine[2 * p] = (double)P->recv_off[p];
        mine[2 * p + 1] = (double)L.slot_bytes;
        ex.add(&mine[2 * p], 2, &theirs[2 * p], 2);
    }
    MGCR_TRY(ex.run(c, P->peers));
    d->pw_peer_rx.assign(np, nullptr);
    bool good = false;
    MGCR_TRY(ipc_map_peers(c, ok ? d->pw_rx : nullptr, (int)np, P->peers.data(), d->pw_peer_rx.data(), &good));
    if (good) {   // from here on neighbours may store into pw_rx
        if (np) good = halo_pw_fill_table(d, theirs) && halo_pw_selftest(d);
        MGCR_TRY(comm_agree(c, &good));
    }
    d->pw_on = good && np > 0;
    if (!d->pw_on) {
        if (!good) {
            hipDeviceSynchronize();
            *(volatile int *)c->pw_err = 0;
        }
        halo_pw_release(d);
        (void)hipGetLastError();
    }
    return MGCR_OK;
}

// the halo segment the exchange begun last delivers into (call after dist_halo_begin)
const cplx *dist_halo_ptr(DistCsr *d) { return d->pw_on ? halo_pw_slot(d, d->pw_seq) : d->xh; }

int dist_halo_begin(DistCsr *d, const cplx *x, bool overlap_interior) {
    Comm *c = d->comm;
    Plan *P = d->plan;
    const int np = (int)P->peers.size();
    if (np == 0) return MGCR_OK;
    if (d->pw_on) return halo_pw_launch(d, x, overlap_interior);
    hipStream_t main = ctx().stream;
    int64_t tot_send = d->send.off.empty() ? 0 : d->send.off.back() + d->send.cnt.back();
    // pack the non-contiguous send lists
    for (int p = 0; p < np; p++)
        if (d->send.contig[(size_t)p] < 0 && d->send.cnt[(size_t)p]) {
            hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((d->send.cnt[(size_t)p] + 255) / 256)), dim3(256), 0, main,
                               d->send.cnt[(size_t)p], d->send_idx + d->send.off[(size_t)p], x, d->sendbuf + d->send.off[(size_t)p],
                               get_apply_skip().p, get_apply_skip().it);
            MGCR_HIP(hipGetLastError());
        }
    if (c->is_rccl) {
        // Default: the exchange is ordered on the compute stream, like the all-reduces — every RCCL
        // call of this communicator then sits on one stream, in the same order on every rank.
        // MGCR_HALO_OVERLAP=1 moves it to the communication stream so that it overlaps the interior
        // rows (to be switched on once it has been exercised on a multi-GPU node).
        hipStream_t cs = g_halo_overlap.on() ? c->comm_stream : main;
        if (cs != main) {
            MGCR_HIP(hipEventRecord(c->ev_ready, main));
            MGCR_HIP(hipStreamWaitEvent(cs, c->ev_ready, 0));
        }
        MGCR_NCCL(rccl().GroupStart());
        for (int p = 0; p < np; p++) {
            const cplx *src = d->send.contig[(size_t)p] >= 0 ? x + d->send.contig[(size_t)p] : d->sendbuf + d->send.off[(size_t)p];
            if (d->send.cnt[(size_t)p])
                MGCR_NCCL(rccl().Send(src, (size_t)d->send.cnt[(size_t)p] * 2, ncclDouble, P->peers[(size_t)p], c->nccl, cs));
            if (P->recv_count[(size_t)p])
                MGCR_NCCL(rccl().Recv(d->xh + P->recv_off[(size_t)p], (size_t)P->recv_count[(size_t)p] * 2, ncclDouble, P->peers[(size_t)p], c->nccl, cs));
        }
        MGCR_NCCL(rccl().GroupEnd());
        if (cs != main) MGCR_HIP(hipEventRecord(c->ev_done, cs));
        return MGCR_OK;
    }
    // host-staged transport: device -> host, callback, host -> device (synchronous)
    d->h_send.resize((size_t)tot_send * 2);
    d->h_recv.resize(P->halo_gid.size() * 2);
    HostExchange ex;
    for (int p = 0; p < np; p++) {
        const cplx *src = d->send.contig[(size_t)p] >= 0 ? x + d->send.contig[(size_t)p] : d->sendbuf + d->send.off[(size_t)p];
        if (d->send.cnt[(size_t)p])
            MGCR_HIP(hipMemcpyAsync(d->h_send.data() + 2 * d->send.off[(size_t)p], src, sizeof(cplx) * (size_t)d->send.cnt[(size_t)p], hipMemcpyDeviceToHost, main));
        ex.add(d->h_send.data() + 2 * d->send.off[(size_t)p], 2 * d->send.cnt[(size_t)p], d->h_recv.data() + 2 * P->recv_off[(size_t)p],
               2 * P->recv_count[(size_t)p]);
    }
    MGCR_HIP(hipStreamSynchronize(main));
    MGCR_TRY(ex.run(c, P->peers));
    if (!P->halo_gid.empty())
        MGCR_HIP(hipMemcpyAsync(d->xh, d->h_recv.data(), sizeof(cplx) * P->halo_gid.size(), hipMemcpyHostToDevice, main));
    return MGCR_OK;
}

int dist_halo_end(DistCsr *d) {
    Comm *c = d->comm;
    if (d->pw_wait_pending) {   // second half of a split peer-write exchange (halo_pw_kernel<false>)
        d->pw_wait_pending = false;
        const int np = (int)d->plan->peers.size();
        hipLaunchKernelGGL(halo_pw_wait_kernel, dim3(1), dim3(64), 0, ctx().stream, (const HaloPwPeer *)d->pw_tab, np, d->pw_seq, c->pw_err, d->pw_timeout);
        MGCR_HIP(hipGetLastError());
        g_halo_split_count++;
        return MGCR_OK;
    }
    if (c->is_rccl && g_halo_overlap.on() && !d->plan->peers.empty()) MGCR_HIP(hipStreamWaitEvent(ctx().stream, c->ev_done, 0));
    return MGCR_OK;
}

void dist_info(DistCsr *d, const cplx **xh, int64_t *interior_begin, int64_t *interior_end) {
    *xh = dist_halo_ptr(d);
    *interior_begin = d->plan->interior_begin;
    *interior_end = d->plan->interior_end;
}

Comm *dist_comm(DistCsr *d) { return d->comm; }
void dist_sizes(DistCsr *d, int64_t *nloc, int64_t *nh, int64_t *row0, int64_t *n_global, int *rank, int *nranks) {
    if (nloc) *nloc = d->plan->nloc;
    if (nh) *nh = (int64_t)d->plan->halo_gid.size();
    if (row0) *row0 = d->plan->row0;
    if (n_global) *n_global = d->plan->n_global;
    if (rank) *rank = d->comm->rank;
    if (nranks) *nranks = d->comm->nranks;
}

// host-level halo exchange of w doubles per row (set-up data: aggregate ids, prolongator rows):
// own[nloc*w] -> halo[nh*w], same lists as the SpMV halo
int dist_exchange_rows_host(DistCsr *d, const double *own, int w, double *halo) {
    Plan *P = d->plan;
    const size_t np = P->peers.size();
    std::vector<std::vector<double>> sb(np);
    HostExchange ex;
    for (size_t p = 0; p < np; p++) {
        const std::vector<int64_t> &rows = P->send_rows[p];
        sb[p].resize(rows.size() * (size_t)w);
        for (size_t i = 0; i < rows.size(); i++)
            memcpy(sb[p].data() + i * (size_t)w, own + (size_t)rows[i] * (size_t)w, sizeof(double) * (size_t)w);
        ex.add(sb[p].data(), (int64_t)rows.size() * w, halo + (size_t)P->recv_off[p] * (size_t)w, P->recv_count[p] * w);
    }
    return ex.run(d->comm, P->peers);
}

void dist_free(DistCsr *d) {
    if (!d) return;
    halo_pw_release(d);
    hipFree(d->xh); hipFree(d->sendbuf); hipFree(d->send_idx);
    delete d->plan;
    delete d;
}
int dist_halo_kind(DistCsr *d) { return d->pw_on ? 2 : d->comm->is_rccl ? 1 : 0; }

// the device side of a partition plan: halo segment, send lists, peer-write receive slots (collective: the peer-write
// self-tests run here).  Takes the plan over; *out is the caller's (dist_free, through its Op).
static int dist_attach(Comm *c, std::unique_ptr<Plan> P, DistCsr **out) {
    SendLists s = plan_send_lists(*P);
    const size_t nh = P->halo_gid.size(), tot = s.idx.size();
    DevBuf<cplx> xh, sendbuf;
    DevBuf<int32_t> send_idx;
    hipError_t e = hipSuccess;
    if (nh) e = xh.malloc(nh);
    if (e == hipSuccess && tot) e = sendbuf.malloc(tot);
    if (e == hipSuccess && tot) e = send_idx.malloc(tot);
    if (e == hipSuccess && tot) e = hipMemcpy(send_idx.p, s.idx.data(), sizeof(int32_t) * tot, hipMemcpyHostToDevice);
    MGCR_CHECK(e == hipSuccess, MGCR_ERR_ALLOC, "distributed operator: device allocation failed: %s", hipGetErrorString(e));
    std::unique_ptr<DistCsr, void (*)(DistCsr *)> d(new DistCsr(), dist_free);
    d->comm = c;
    d->plan = P.release();
    d->pw_seq = pw_seq0();
    d->xh = xh.release(); d->sendbuf = sendbuf.release(); d->send_idx = send_idx.release();
    d->send = std::move(s);
    MGCR_TRY(comm_device_ready(c));
    MGCR_TRY(comm_pw_setup(c));
    MGCR_TRY(halo_pw_setup(d.get()));
    *out = d.release();
    return MGCR_OK;
}

int dist_csr_create(Comm *c, int64_t n_global, int64_t row0, int64_t nloc, const int64_t *rowptr, const int64_t *col,
                    const double *val_ri, Op *op) {
    std::unique_ptr<Plan> P;
    MGCR_TRY(plan_build(c, n_global, row0, nloc, rowptr, col, &P));
    MGCR_TRY(csr_build_device(nloc, nloc + (int64_t)P->halo_gid.size(), rowptr, P->col_local.data(), val_ri, &op->csr));
    std::vector<int64_t>().swap(P->col_local);
    const int rc = dist_attach(c, std::move(P), &op->dist);
    if (rc != MGCR_OK) { csr_free(&op->csr); return rc; }
    op->comm = c;
    return MGCR_OK;
}

// Row block of a distributed HierarchicalSparse (src/HierarchicalSparse.h:101-161): block rows [brow0, brow0 + nbloc) of
// nb_global, block columns GLOBAL.  The partition plan is made at BLOCK granularity (a halo entry = one block row of x,
// bs values) and expanded to the element lists the halo machinery above works on (comm_plan.h plan_expand); the apply reads a
// block column's bs values from x (owned) or in place from the halo segment.
int dist_bcsr_create(Comm *c, int64_t nb_global, int64_t brow0, int32_t nbloc, int32_t bs, const int32_t *browptr,
                     const int64_t *bcol_global, const double *blocks_ri, Op *op) {
    MGCR_CHECK(bs >= 1 && nbloc >= 0 && browptr && browptr[0] == 0, MGCR_ERR_INVALID, "dist_bcsr_create: bad argument");
    std::vector<int64_t> rp(browptr, browptr + nbloc + 1);
    std::unique_ptr<Plan> B;
    MGCR_TRY(plan_build(c, nb_global, brow0, nbloc, rp.data(), bcol_global, &B));
    const int64_t nhb = (int64_t)B->halo_gid.size();
    MGCR_CHECK(((int64_t)nbloc + nhb) * bs < ((int64_t)1 << 31), MGCR_ERR_UNSUPPORTED, "row block too large");
    std::vector<int32_t> bcol_local(B->col_local.begin(), B->col_local.end());
    MGCR_TRY(bcsr_build_device(nbloc, (int32_t)(nbloc + nhb), bs, browptr, bcol_local.data(), blocks_ri, &op->bcsr));
    const int rc = dist_attach(c, std::make_unique<Plan>(plan_expand(*B, bs)), &op->dist);
    if (rc != MGCR_OK) { bcsr_free(&op->bcsr); return rc; }
    op->comm = c;
    return MGCR_OK;
}

}  // namespace mgcr

using namespace mgcr;
struct mgcr_plan_s : mgcr::Plan {};

// an Op of `rows` local rows (Fields of a distributed operator hold this rank's rows), filled by `create` under the context lock
template <typename F>
static int dist_op_create(OpKind kind, int64_t rows, mgcr_op_t *out, F &&create) {
    std::lock_guard<std::recursive_mutex> lk(ctx().mtx);
    std::unique_ptr<mgcr_op_s> op(new mgcr_op_s());
    op->kind = kind;
    op->dim = op->nrow = rows;
    MGCR_TRY(create(op.get()));
    *out = op.release();
    return MGCR_OK;
}

extern "C" {

int mgcr_plan_create(mgcr_comm_t comm, int64_t n_global, int64_t row0, int64_t nrow_local, const int64_t *rowptr,
                     const int64_t *col_global, mgcr_plan_t *out) {
    MGCR_CHECK(comm && out && rowptr, MGCR_ERR_INVALID, "mgcr_plan_create: null argument");
    std::unique_ptr<Plan> P;
    MGCR_TRY(plan_build(comm, n_global, row0, nrow_local, rowptr, col_global, &P));
    *out = static_cast<mgcr_plan_s *>(P.release());
    return MGCR_OK;
}

int mgcr_plan_info(mgcr_plan_t plan, int64_t *n_halo, int32_t *npeers, int64_t *interior_begin, int64_t *interior_end) {
    MGCR_CHECK(plan, MGCR_ERR_INVALID, "null plan");
    if (n_halo) *n_halo = (int64_t)plan->halo_gid.size();
    if (npeers) *npeers = (int32_t)plan->peers.size();
    if (interior_begin) *interior_begin = plan->interior_begin;
    if (interior_end) *interior_end = plan->interior_end;
    return MGCR_OK;
}

int mgcr_plan_peers(mgcr_plan_t plan, int32_t *peers, int64_t *send_counts, int64_t *recv_counts) {
    MGCR_CHECK(plan, MGCR_ERR_INVALID, "null plan");
    for (size_t p = 0; p < plan->peers.size(); p++) {
        if (peers) peers[p] = plan->peers[p];
        if (send_counts) send_counts[p] = (int64_t)plan->send_rows[p].size();
        if (recv_counts) recv_counts[p] = plan->recv_count[p];
    }
    return MGCR_OK;
}

int mgcr_plan_local_columns(mgcr_plan_t plan, int64_t *col_local) {
    MGCR_CHECK(plan && col_local, MGCR_ERR_INVALID, "null argument");
    MGCR_CHECK((int64_t)plan->col_local.size() == plan->nnz, MGCR_ERR_INVALID, "plan no longer holds its column map");
    memcpy(col_local, plan->col_local.data(), sizeof(int64_t) * (size_t)plan->nnz);
    return MGCR_OK;
}

int mgcr_plan_send_indices(mgcr_plan_t plan, int32_t peer_slot, int64_t *local_rows) {
    MGCR_CHECK(plan && local_rows && peer_slot >= 0 && peer_slot < (int32_t)plan->peers.size(), MGCR_ERR_INVALID, "bad argument");
    const std::vector<int64_t> &r = plan->send_rows[(size_t)peer_slot];
    memcpy(local_rows, r.data(), sizeof(int64_t) * r.size());
    return MGCR_OK;
}

int mgcr_plan_halo_globals(mgcr_plan_t plan, int64_t *global_cols) {
    MGCR_CHECK(plan && global_cols, MGCR_ERR_INVALID, "null argument");
    memcpy(global_cols, plan->halo_gid.data(), sizeof(int64_t) * plan->halo_gid.size());
    return MGCR_OK;
}

int mgcr_plan_destroy(mgcr_plan_t plan) {
    delete static_cast<mgcr::Plan *>(plan);
    return MGCR_OK;
}

int mgcr_dbcsr_create(mgcr_comm_t comm, int64_t nb_global, int64_t brow0, int32_t nbrow_local, int32_t bs, const int32_t *browptr,
                      const int64_t *bcol_global, const double *blocks_ri, mgcr_op_t *out) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(comm && out && browptr && (bcol_global || browptr[nbrow_local] == 0) && (blocks_ri || browptr[nbrow_local] == 0),
               MGCR_ERR_INVALID, "mgcr_dbcsr_create: null argument");
    return dist_op_create(OP_BCSR, (int64_t)nbrow_local * bs, out, [&](Op *op) {
        return dist_bcsr_create(comm, nb_global, brow0, nbrow_local, bs, browptr, bcol_global, blocks_ri, op);
    });
}

int mgcr_dcsr_create(mgcr_comm_t comm, int64_t n_global, int64_t row0, int64_t nrow_local, const int64_t *rowptr,
                     const int64_t *col_global, const double *val_ri, mgcr_op_t *out) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(comm && out && rowptr, MGCR_ERR_INVALID, "mgcr_dcsr_create: null argument");
    return dist_op_create(OP_CSR, nrow_local, out, [&](Op *op) { return dist_csr_create(comm, n_global, row0, nrow_local, rowptr, col_global, val_ri, op); });
}

}  // extern "C"
