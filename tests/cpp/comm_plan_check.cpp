// Runs the partition plan of a distributed operator (csrc/comm_plan.h) for ALL ranks in one process — each stage for every rank,
// the all-reduce a summation of the ranks' buffers, the exchange a copy between them — and prints one line per case and rank;
// tests/test_comm_plan.py builds this with the address and undefined-behaviour sanitizers and compares the lines with values
// worked out by hand.
#include <cstdio>

#include "comm_plan.h"

using namespace mgcr;

static void list(const char *name, const std::vector<int64_t> &v) {
    printf(" %s=", name);
    for (size_t i = 0; i < v.size(); i++) printf(i ? ",%lld" : "%lld", (long long)v[i]);
}
static void show(const Plan &P) {
    list("offsets", P.offsets);
    list("halo", P.halo_gid);
    list("peers", std::vector<int64_t>(P.peers.begin(), P.peers.end()));
    printf(" counts=");   // per peer: (entries received, rows sent) @ start of the peer's part of the halo segment
    for (size_t p = 0; p < P.peers.size(); p++) printf("(%lld,%zu)@%lld", (long long)P.recv_count[p], P.send_rows[p].size(), (long long)P.recv_off[p]);
    printf(" send=");
    for (const auto &rows : P.send_rows) {
        printf("{");
        for (size_t i = 0; i < rows.size(); i++) printf(i ? ",%lld" : "%lld", (long long)rows[i]);
        printf("}");
    }
    list("cols", P.col_local);
    printf(" interior=[%lld,%lld)\n", (long long)P.interior_begin, (long long)P.interior_end);
}

// one rank's row block: first row, and the rows' GLOBAL columns
struct Block {
    int64_t row0;
    std::vector<std::vector<int64_t>> rows;
};

// plan_build for every rank; false (and the text printed) when a stage rejects its input
static bool build(const char *name, int64_t n_global, const std::vector<Block> &blocks, std::vector<Plan> &P) {
    const size_t R = blocks.size();
    std::vector<std::vector<int64_t>> rowptr(R), col(R);
    P.assign(R, Plan());
    std::string err;
    std::vector<double> sum(R, 0.), M(R * R, 0.);
    for (size_t r = 0; r < R && err.empty(); r++) {
        rowptr[r].push_back(0);
        for (const auto &row : blocks[r].rows) {
            col[r].insert(col[r].end(), row.begin(), row.end());
            rowptr[r].push_back((int64_t)col[r].size());
        }
        err = plan_begin(P[r], n_global, blocks[r].row0, (int64_t)blocks[r].rows.size(), rowptr[r].data());
        sum[r] += (double)blocks[r].row0;   // all-reduce: every rank contributes its own entry
    }
    for (size_t r = 0; r < R && err.empty(); r++) err = plan_offsets(P[r], sum.data(), (int)R);
    for (size_t r = 0; r < R && err.empty(); r++) err = plan_remote(P[r], col[r].data(), M.data() + r * R);
    for (size_t r = 0; r < R && err.empty(); r++) plan_peers(P[r], M.data(), (int)R, (int)r);
    for (size_t r = 0; r < R && err.empty(); r++)   // exchange: rank r's request to its peer q lands in q's list for r
        for (size_t p = 0; p < P[r].peers.size(); p++) {
            Plan &Q = P[(size_t)P[r].peers[p]];
            const size_t back = (size_t)(std::find(Q.peers.begin(), Q.peers.end(), (int32_t)r) - Q.peers.begin());
            if (back == Q.peers.size() || Q.send_rows[back].size() != (size_t)P[r].recv_count[p]) { err = "peer lists do not match"; break; }
            std::copy_n(P[r].halo_gid.begin() + P[r].recv_off[p], P[r].recv_count[p], Q.send_rows[back].begin());
        }
    for (size_t r = 0; r < R && err.empty(); r++) err = plan_send_rows(P[r]);
    for (size_t r = 0; r < R && err.empty(); r++) plan_columns(P[r], rowptr[r].data(), col[r].data());
    if (!err.empty()) printf("%s error %s\n", name, err.c_str());
    return err.empty();
}

static void plans(const char *name, int64_t n_global, const std::vector<Block> &blocks) {
    std::vector<Plan> P;
    if (!build(name, n_global, blocks, P)) return;
    for (size_t r = 0; r < P.size(); r++) { printf("%s rank%zu", name, r); show(P[r]); }
}

// rows [row0, row0 + n) of the 1-D 3-point Laplacian on n_global points, or of the identity
static Block laplace(int64_t row0, int64_t n, int64_t n_global) {
    Block b{row0, {}};
    for (int64_t i = row0; i < row0 + n; i++) {
        b.rows.emplace_back();
        for (int64_t j = std::max<int64_t>(i - 1, 0); j <= std::min(i + 1, n_global - 1); j++) b.rows.back().push_back(j);
    }
    return b;
}
static Block identity(int64_t row0, int64_t n) {
    Block b{row0, {}};
    for (int64_t i = row0; i < row0 + n; i++) b.rows.push_back({i});
    return b;
}

static bool same(const Plan &a, const Plan &b) {
    return a.n_global == b.n_global && a.row0 == b.row0 && a.nloc == b.nloc && a.offsets == b.offsets && a.halo_gid == b.halo_gid && a.peers == b.peers &&
           a.recv_count == b.recv_count && a.recv_off == b.recv_off && a.send_rows == b.send_rows && a.interior_begin == b.interior_begin &&
           a.interior_end == b.interior_end;
}

int main() {
    plans("lap1d-3", 12, {laplace(0, 4, 12), laplace(4, 4, 12), laplace(8, 4, 12)});
    plans("lap1d-empty", 12, {laplace(0, 4, 12), laplace(4, 0, 12), laplace(4, 4, 12), laplace(8, 4, 12)});
    {
        Block b0 = identity(0, 2);
        b0.rows[0].push_back(5);   // rank 0 needs a row of rank 2, which needs nothing back
        plans("one-sided", 6, {b0, identity(2, 2), identity(4, 2)});
    }
    {
        Block b0 = identity(0, 4);
        b0.rows[0] = {7, 0, 5, 7};
        plans("unsorted", 8, {b0, identity(4, 4)});
    }
    {
        Block b0 = identity(0, 5);
        b0.rows[2].push_back(5);   // interior runs [0, 2) and [3, 5)
        plans("tie", 10, {b0, identity(5, 5)});
    }
    plans("all-touch", 4, {Block{0, {{0, 2}, {1, 3}}}, identity(2, 2)});

    plans("col-range", 4, {Block{0, {{0, 4}, {1}}}, identity(2, 2)});
    plans("unordered", 4, {identity(2, 2), identity(0, 2)});
    {
        Plan P;
        P.row0 = 4; P.nloc = 4;
        P.send_rows = {{5, 7}};
        const std::string ok = plan_send_rows(P);
        printf("send-rows owned '%s'", ok.c_str());
        list("rows", P.send_rows[0]);
        P.send_rows = {{5, 8}};
        printf("\nsend-rows foreign '%s'\n", plan_send_rows(P).c_str());
    }

    {   // lap1d-3 as a matrix of dense 3 x 3 blocks: plan of the blocks, expanded, against the plan of the element matrix
        std::vector<Block> blocks{laplace(0, 4, 12), laplace(4, 4, 12), laplace(8, 4, 12)}, elems;
        for (const Block &b : blocks) {
            elems.push_back(Block{b.row0 * 3, {}});
            for (const auto &row : b.rows)
                for (int k = 0; k < 3; k++) {
                    elems.back().rows.emplace_back();
                    for (int64_t c : row) for (int j = 0; j < 3; j++) elems.back().rows.back().push_back(c * 3 + j);
                }
        }
        std::vector<Plan> B, E;
        if (build("expand", 12, blocks, B) && build("expand", 36, elems, E))
            for (size_t r = 0; r < B.size(); r++) {
                const Plan X = plan_expand(B[r], 3);
                printf("expand rank%zu same=%d", r, (int)same(X, E[r]));
                show(X);
            }
    }

    {
        Plan P;
        P.send_rows = {{2, 3, 4}, {1, 3}, {5}, {}};
        const SendLists s = plan_send_lists(P);
        printf("sendlists mixed");
        list("off", s.off); list("cnt", s.cnt); list("contig", s.contig);
        list("idx", std::vector<int64_t>(s.idx.begin(), s.idx.end()));
        printf("\n");
    }

    printf("layout slot_bytes %zu %zu %zu %zu\n", pw_rx_slot_bytes(0), pw_rx_slot_bytes(1), pw_rx_slot_bytes(16), pw_rx_slot_bytes(17));
    const PwRxLayout L{pw_rx_slot_bytes(17), 16};
    printf("layout offsets slot=%zu,%zu flag_rank3=%zu,%zu total=%zu\n", L.slot(0), L.slot(1), L.flag(0, 3), L.flag(1, 3), L.total());

    printf("seq advance %u %u %u\n", pw_advance(0u), pw_advance(0xFFFFFFFEu), pw_advance(0xFFFFFFFFu));
    printf("seq wrap");
    uint32_t seq = 0xFFFFFFFDu;
    for (int i = 0; i < 5; i++) { seq = pw_advance(seq); printf(" %u:%u", seq, seq & 1u); }
    printf("\n");
    return 0;
}
