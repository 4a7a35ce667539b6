// The row-block partition plan of a distributed operator as pure host arithmetic, cut into stages at its collectives: plain data
// in, plain data out, no HIP or RCCL header — tests/cpp/comm_plan_check.cpp plays all ranks in one process, plan_build (halo.hip)
// puts the collectives between the stages.  A stage that can reject its input returns the error text ("" = fine).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace mgcr {

struct Comm;

struct Plan {
    Comm *comm = nullptr;
    int64_t n_global = 0, row0 = 0, nloc = 0, nnz = 0;
    std::vector<int64_t> offsets;       // row0 of every rank, + n_global
    std::vector<int64_t> halo_gid;      // sorted global ids of the remote columns (grouped by owner, ascending)
    std::vector<int32_t> peers;         // ranks exchanged with (ascending)
    std::vector<int64_t> recv_count, recv_off;            // per peer: entries of the halo segment
    std::vector<std::vector<int64_t>> send_rows;          // per peer: my local rows it needs, in its halo order
    std::vector<int64_t> col_local;     // nnz
    int64_t interior_begin = 0, interior_end = 0;         // rows [begin, end) reference no halo column
};

inline int owner_of(const std::vector<int64_t> &offsets, int64_t gid) {
    return (int)(std::upper_bound(offsets.begin(), offsets.end(), gid) - offsets.begin()) - 1;
}

// Next sequence number of a peer-write exchange.  Never 0 (mailboxes start zeroed), and the slot parity (seq & 1) must keep
// alternating: after 0xFFFFFFFF (odd) comes 2, not 1 — two consecutive exchanges in one slot would let a fast rank overwrite
// words a slower peer has not read yet.
inline uint32_t pw_advance(uint32_t seq) { return seq == 0xFFFFFFFFu ? 2u : seq + 1; }

// before the first all-reduce (every rank contributes its row0)
inline std::string plan_begin(Plan &P, int64_t n_global, int64_t row0, int64_t nloc, const int64_t *rowptr) {
    if (!rowptr || row0 < 0 || nloc < 0 || row0 + nloc > n_global) return "mgcr_plan_create: bad row block";
    P.n_global = n_global; P.row0 = row0; P.nloc = nloc; P.nnz = rowptr[nloc];
    return "";
}

// after it: summed[r] = row0 of rank r
inline std::string plan_offsets(Plan &P, const double *summed, int R) {
    P.offsets.resize((size_t)R + 1);
    for (int r = 0; r < R; r++) P.offsets[(size_t)r] = (int64_t)summed[r];
    P.offsets[(size_t)R] = P.n_global;
    for (int r = 0; r < R; r++)
        if (P.offsets[(size_t)r] > P.offsets[(size_t)r + 1]) return "mgcr_plan_create: row blocks must be ordered by rank and contiguous";
    return "";
}

// remote columns -> halo_gid (ascending global id == grouped by owner rank), and this rank's row of the counts matrix:
// need[q] = number of entries this rank needs from rank q
inline std::string plan_remote(Plan &P, const int64_t *col, double *need) {
    std::vector<int64_t> &remote = P.halo_gid;
    remote.clear();
    for (int64_t l = 0; l < P.nnz; l++) {
        const int64_t g = col[l];
        if (g < 0 || g >= P.n_global) return "mgcr_plan_create: column " + std::to_string(g) + " out of range";
        if (g < P.row0 || g >= P.row0 + P.nloc) remote.push_back(g);
    }
    std::sort(remote.begin(), remote.end());
    remote.erase(std::unique(remote.begin(), remote.end()), remote.end());
    for (int64_t g : remote) need[owner_of(P.offsets, g)] += 1.;
    return "";
}

// after the counts all-reduce: M[r * R + q] = number of entries rank r needs from rank q.  A rank is a peer when either
// direction is non-zero, so the peer lists are symmetric; send_rows[p] is sized to receive the peer's request.
inline void plan_peers(Plan &P, const double *M, int R, int rank) {
    int64_t off = 0;
    for (int q = 0; q < R; q++) {
        const int64_t need = (int64_t)M[(size_t)rank * R + q], owed = (int64_t)M[(size_t)q * R + rank];
        if (q == rank || !(need || owed)) continue;
        P.peers.push_back(q);
        P.recv_count.push_back(need);
        P.recv_off.push_back(off);
        off += need;
        P.send_rows.emplace_back((size_t)owed);
    }
}

// after the exchange of ids (halo_gid + recv_off[p] -> the peer's send_rows[.]): global ids -> local rows
inline std::string plan_send_rows(Plan &P) {
    for (std::vector<int64_t> &rows : P.send_rows)
        for (int64_t &g : rows) {
            if (g < P.row0 || g >= P.row0 + P.nloc) return "mgcr_plan_create: peer asked for a row this rank does not own";
            g -= P.row0;
        }
    return "";
}

// local column numbering (owned: g - row0; remote: nloc + slot in halo_gid) and the interior: the longest run of rows without
// a halo column, the first one on a tie (slab partition: all but the first and last plane)
inline void plan_columns(Plan &P, const int64_t *rowptr, const int64_t *col) {
    P.col_local.resize((size_t)P.nnz);
    int64_t best_b = 0, best_e = 0, cur_b = 0;
    for (int64_t r = 0; r <= P.nloc; r++) {
        bool touches = r == P.nloc;   // the end of the block closes the last run
        for (int64_t l = rowptr[r]; r < P.nloc && l < rowptr[r + 1]; l++) {
            const int64_t g = col[l];
            const bool own = g >= P.row0 && g < P.row0 + P.nloc;
            P.col_local[(size_t)l] = own ? g - P.row0 : P.nloc + (std::lower_bound(P.halo_gid.begin(), P.halo_gid.end(), g) - P.halo_gid.begin());
            touches |= !own;
        }
        if (touches) {
            if (r - cur_b > best_e - best_b) { best_b = cur_b; best_e = r; }
            cur_b = r + 1;
        }
    }
    P.interior_begin = best_b;
    P.interior_end = best_e;
}

// block plan -> element plan: block b -> elements b*bs .. b*bs + bs - 1, same order (col_local and nnz stay empty: the
// block operator keeps its block columns)
inline Plan plan_expand(const Plan &B, int64_t bs) {
    Plan P;
    P.comm = B.comm; P.n_global = B.n_global * bs; P.row0 = B.row0 * bs; P.nloc = B.nloc * bs;
    for (int64_t o : B.offsets) P.offsets.push_back(o * bs);
    for (int64_t g : B.halo_gid) for (int64_t k = 0; k < bs; k++) P.halo_gid.push_back(g * bs + k);
    P.peers = B.peers;
    for (size_t p = 0; p < B.peers.size(); p++) {
        P.recv_count.push_back(B.recv_count[p] * bs);
        P.recv_off.push_back(B.recv_off[p] * bs);
        P.send_rows.emplace_back();
        for (int64_t r : B.send_rows[p]) for (int64_t k = 0; k < bs; k++) P.send_rows[p].push_back(r * bs + k);
    }
    P.interior_begin = B.interior_begin * bs;
    P.interior_end = B.interior_end * bs;
    return P;
}

// the send lists as the device sees them: peer p's rows are idx[off[p] .. off[p] + cnt[p]); contig[p] >= 0: they are the
// contiguous range starting there (no packing needed), -1 otherwise and for an empty list
struct SendLists {
    std::vector<int64_t> off, cnt, contig;
    std::vector<int32_t> idx;
};
inline SendLists plan_send_lists(const Plan &P) {
    SendLists s;
    for (const std::vector<int64_t> &rows : P.send_rows) {
        s.off.push_back((int64_t)s.idx.size());
        s.cnt.push_back((int64_t)rows.size());
        bool contig = !rows.empty();
        for (size_t i = 1; i < rows.size() && contig; i++) contig = rows[i] == rows[i - 1] + 1;
        s.contig.push_back(contig ? rows[0] : -1);
        for (int64_t r : rows) s.idx.push_back((int32_t)r);
    }
    return s;
}

// Byte layout of a peer-write receive buffer: [2 slots][slot_bytes] of 16-byte halo entries (a slot rounded up to 256 bytes),
// then [2 slots][max_ranks] 8-byte flag words.  A peer's layout follows from ITS slot_bytes.
struct PwRxLayout {
    size_t slot_bytes, max_ranks;
    size_t slot(int s) const { return (size_t)s * slot_bytes; }
    size_t flag(int s, int rank) const { return 2 * slot_bytes + ((size_t)s * max_ranks + (size_t)rank) * 8; }
    size_t total() const { return flag(2, 0); }
};
inline size_t pw_rx_slot_bytes(size_t n_halo) { return (n_halo * 16 + 255) / 256 * 256; }

}  // namespace mgcr
