// What comm.hip (communicator, host collectives, peer-write all-reduce) and halo.hip (distributed operator, halo transports) share.
#pragma once
#include <rccl/rccl.h>

#include "internal.h"
#include "comm_plan.h"

namespace mgcr {

// RCCL, bound at run time (comm.hip rccl_load)
struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi &rccl();

#define MGCR_NCCL(call)                                                                                                              \
    do {                                                                                                                             \
        ncclResult_t r__ = (call);                                                                                                   \
        MGCR_CHECK(r__ == ncclSuccess, MGCR_ERR_COMM, "RCCL error %d (%s) in %s", (int)r__, rccl().GetErrorString(r__), #call);    \
    } while (0)

struct Comm {
    int rank = 0, nranks = 1;
    bool is_rccl = false;
    ncclComm_t nccl = nullptr;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_ready = nullptr, ev_done = nullptr;
    mgcr_allreduce_cb allreduce = nullptr;
    mgcr_exchange_cb exchange = nullptr;
    void *user = nullptr;
    // staging for host-level collectives over RCCL (set-up only)
    double *d_stage = nullptr;
    size_t d_stage_cap = 0;
    double *h_pin = nullptr;  // pinned, for the host-staged transport's scalar all-reduces
    // peer-write all-reduce of the per-iteration scalars (comm.hip): mailboxes mapped into every rank
    bool pw_tried = false, pw_on = false;
    uint64_t *pw_mbox = nullptr;             // this rank's mailbox (uncached device memory, shared by hipIpc)
    void *pw_peer[PW_MAX_RANKS] = {};        // pw_peer[r]: rank r's mailbox (uint64_t words) as mapped here (own one for r == rank)
    uint32_t pw_seq = 0;                     // sequence number of the last all-reduce (never 0 on the wire)
    int *pw_err = nullptr;                   // pinned host word the kernel sets when a wait timed out
    unsigned *pw_ticket = nullptr;           // device counter of the producer kernels' fold tails (pw_tail_dev.h)
};

// first sequence number of the peer-write exchanges (tests start just below the 32-bit wrap: MGCR_TEST_PW_SEQ0)
inline uint32_t pw_seq0() {
    const char *e = getenv("MGCR_TEST_PW_SEQ0");
    return e ? (uint32_t)strtoul(e, nullptr, 0) : 0u;
}
// wall_clock64 runs at 100 MHz.  Self-tests (ranks just synchronised by a set-up collective): 3 s.  Production: 20 s — the
// ranks of one solve may arrive skewed (one of them still reading a file), but a wave must never spin anywhere near the
// driver's compute-queue watchdog (60 s).
constexpr long long PW_TIMEOUT_TEST = 300000000LL;
long long pw_timeout_run();   // MGCR_PEER_TIMEOUT_MS (tests shorten it), clamped to 1 ms .. 30 s

int comm_device_ready(Comm *c);
int comm_pw_setup(Comm *c);   // collective; never fails its caller for a transport reason
// host-level neighbour exchange (set-up), counts in doubles; the all-reduce next to it, comm_allreduce_host, is in internal.h
int comm_exchange_host(Comm *c, int npeers, const int *peers, const double *const *send, const int64_t *scount, double *const *recv,
                       const int64_t *rcount);
int comm_agree(Comm *c, bool *good);   // *good = every rank came with *good set

// the argument arrays of comm_exchange_host: one add() per peer, in the order of `peers`
struct HostExchange {
    std::vector<const double *> sp;
    std::vector<double *> rp;
    std::vector<int64_t> sc, rcv;
    void add(const double *send, int64_t scount, double *recv, int64_t rcount) { sp.push_back(send); sc.push_back(scount); rp.push_back(recv); rcv.push_back(rcount); }
    int run(Comm *c, const std::vector<int32_t> &peers) { return comm_exchange_host(c, (int)peers.size(), peers.data(), sp.data(), sc.data(), rp.data(), rcv.data()); }
};

// Collective: shares one hipIpc allocation per rank.  `mine` is this rank's uncached device allocation, already zeroed and
// synchronised (nullptr: it could not be made).  All-gathers the handles, opens those of ranks[0..n) into mapped[] (own rank:
// `mine` itself) and agrees on the outcome: *good is the same on every rank, and nobody may store into a peer's memory before
// it is known.  When it is false, nothing is left open.  ipc_unmap closes what this opened.
int ipc_map_peers(Comm *c, void *mine, int n, const int32_t *ranks, void **mapped, bool *good);
void ipc_unmap(const void *mine, int n, void **mapped);

}  // namespace mgcr

struct mgcr_comm_s : mgcr::Comm {};
