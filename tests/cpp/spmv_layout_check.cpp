// Runs the host decisions of the Sparse format build (csrc/spmv_layout.h) on small inputs and prints one line per case;
// tests/test_spmv_layout.py builds this with the address and undefined-behaviour sanitizers and compares the lines
// with values worked out by hand.
#include <cstdio>
#include <string>

#include "spmv_layout.h"

using namespace mgcr;

template <typename T>
static void list(const char *name, const T *v, size_t n, const char *fmt = " %s=", const char *item = "%lld") {
    printf(fmt, name);
    for (size_t i = 0; i < n; i++) { if (i) printf(","); printf(item, (long long)v[i]); }
}
static void reals(const char *name, const double *v, size_t n) {
    printf(" %s=", name);
    for (size_t i = 0; i < n; i++) printf(i ? ",%g" : "%g", v[i]);
}

static void width(const char *name, int64_t nrow, const std::vector<std::pair<int32_t, int64_t>> &lens) {
    int32_t maxlen = 0;
    for (auto &l : lens) maxlen = std::max(maxlen, l.first);
    std::vector<int64_t> hist((size_t)maxlen + 2, 0);
    for (auto &l : lens) hist[(size_t)l.first] += l.second;
    printf("width %s W=%d\n", name, choose_width(hist, nrow, maxlen));
}

static void tail(const char *name, const std::vector<int32_t> &lens) {
    std::vector<int32_t> tptr(1, 0), long_rows;
    for (int32_t l : lens) tptr.push_back(tptr.back() + l);
    std::vector<TailChunk> chunks;
    deal_tail(tptr, 2048, 256, chunks, long_rows);
    printf("tail %s chunks=", name);
    for (auto &c : chunks) printf("{%d,%d,%d,%d}", c.first, c.last, c.e0, c.e1);
    list("long", long_rows.data(), long_rows.size());
    printf("\n");
}

static void window() {
    // 2500 rows; tail rows 5 (short), 1030 (longer than a chunk), 2499 (short)
    std::vector<int32_t> trows{5, 1030, 2499}, tptr{0, 10, 3010, 3013}, tile_tail, row_tail;
    window_tail_tables(trows, tptr, 2500, 1024, 2048, tile_tail, row_tail);
    printf("window");
    list("tile_tail", tile_tail.data(), tile_tail.size());
    printf(" row_tail=");
    for (size_t r = 0; r < row_tail.size(); r++)
        if (row_tail[r] != -1) printf("[%zu]=%d", r, row_tail[r]);
    printf(" rows=%zu\n", row_tail.size());
}

// a pattern table: rows of (offset, value) pairs, all of width W
struct Table { int npat; int32_t W; std::vector<int32_t> off; std::vector<double> re, im; };
static Table table(int32_t W, const std::vector<std::vector<std::pair<int32_t, double>>> &pats) {
    Table t{(int)pats.size(), W, {}, {}, {}};
    for (auto &p : pats)
        for (auto &e : p) { t.off.push_back(e.first); t.re.push_back(e.second); t.im.push_back(0.); }
    return t;
}
static StenSlots stage1(const char *name, const Table &t) {
    const StenSlots s = sten_stage1(t.off, t.re, t.im, t.npat, t.W, 9);
    printf("stage1 %s view=%d", name, (int)s.view);
    if (s.view) {
        printf(" lead=%d", (int)s.lead);
        list("S", s.S.data(), s.S.size());
        list("bits", s.pbits.data(), s.pbits.size(), " %s=", "0x%llx");
        reals("re", s.re, s.S.size());
        reals("im", s.im, s.S.size());
    }
    printf("\n");
    return s;
}

static void stage2(const char *name, const StenSlots &s1, const std::vector<unsigned long long> &counts, int64_t nrow, bool force) {
    std::vector<unsigned long long> c16(counts);
    c16.resize(16, 0);
    const StenLayout o = sten_stage2(s1, c16, nrow, force, StenLimits{7, 256, 512});
    printf("stage2 %s view=%d", name, (int)o.view);
    if (o.view) {
        list("slot_of", o.slot_of, s1.S.size());
        printf(" kernel_ns=%d stride=%d rare=0x%x pre=%d near=0x%x halo=%d near_f=0x%x halo_f=%d reach=%lld", o.kernel_ns, o.stride, o.rare, o.pre,
               o.near, o.halo, o.near_f, o.halo_f, (long long)o.reach);
        list("off", o.off, (size_t)o.kernel_ns);
        reals("re", o.re, (size_t)o.kernel_ns);
        reals("im", o.im, (size_t)o.kernel_ns);
        list("pmask", o.pmask.data(), o.pmask.size(), " %s=", "0x%llx");
    }
    printf("\n");
}

// stage-1 result written down directly: offsets S, one value per slot, the given presence bits
static StenSlots slots(const std::vector<int32_t> &S, const std::vector<double> &re, bool lead, const std::vector<uint16_t> &pbits) {
    StenSlots s;
    s.view = true; s.lead = lead; s.S = S; s.pbits = pbits;
    for (size_t i = 0; i < re.size(); i++) s.re[i] = re[i];
    return s;
}

// `spmv_layout_check split <len>:<count> ...`: the ELL width, the lanes and the CSR tail the build gives a matrix with this row-length
// histogram (spmv_build.hip: a row's entries beyond W go to the tail) — one line, nothing else (tests/test_mg_shape_cases.py)
static int split(int argc, char **argv) {
    std::vector<std::pair<int32_t, int64_t>> lens;
    int32_t maxlen = 0;
    int64_t nrow = 0;
    for (int a = 2; a < argc; a++) {
        long long len = 0, count = 0;
        if (sscanf(argv[a], "%lld:%lld", &len, &count) != 2 || len < 0 || len >= (1 << 30) || count < 1) return 2;
        lens.push_back({(int32_t)len, (int64_t)count});
        maxlen = std::max(maxlen, (int32_t)len);
        nrow += count;
    }
    std::vector<int64_t> hist((size_t)maxlen + 2, 0);
    for (auto &l : lens) hist[(size_t)l.first] += l.second;
    const int32_t W = choose_width(hist, nrow, maxlen);
    int64_t tail_rows = 0, tail_nnz = 0;
    for (auto &l : lens)
        if (l.first > W) { tail_rows += l.second; tail_nnz += (int64_t)(l.first - W) * l.second; }
    printf("split nrow=%lld W=%d lanes=%d tail_rows=%lld tail_nnz=%lld\n", (long long)nrow, W, choose_lanes(nrow, W), (long long)tail_rows,
           (long long)tail_nnz);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && std::string(argv[1]) == "split") return split(argc, argv);
    width("skew", 1001, {{5, 1000}, {500, 1}});
    width("flat", 100, {{7, 100}});
    printf("lanes %d %d %d\n", choose_lanes(1000, 12), choose_lanes(1000, 7), choose_lanes((int64_t)1 << 18, 12));
    tail("mixed", {100, 3000, 100, 100});
    tail("ones", std::vector<int32_t>(300, 1));
    tail("cap", {2048});
    tail("cap+1", {2049});
    window();

    // 1-D 3-point Laplacian, W = 3: interior, first row (slab padding: last valid column, value 0), last row
    stage1("laplace1d", table(3, {{{-1, -1.}, {0, 2.}, {1, -1.}}, {{0, 2.}, {1, -1.}, {1, 0.}}, {{-1, -1.}, {0, 2.}, {0, 0.}}}));
    stage1("value-differs", table(3, {{{-1, -1.}, {0, 2.}, {1, -1.}}, {{0, 3.}, {1, -1.}, {1, 0.}}}));
    stage1("descending", table(3, {{{0, 2.}, {-1, -1.}, {1, -1.}}}));
    {
        std::vector<std::pair<int32_t, double>> p;
        for (int32_t o = 0; o < 17; o++) p.push_back({o, 1.});
        stage1("17-offsets", table(17, {p}));
    }
    stage1("lead-and-ascending", table(3, {{{5, 3.}, {-1, 1.}, {0, 2.}}, {{-1, 1.}, {0, 2.}, {5, 3.}}}));
    stage1("lead", table(3, {{{5, 3.}, {-1, 1.}, {0, 2.}}, {{-1, 1.}, {0, 2.}, {0, 0.}}}));

    // 7-point stencil of a 64^3 grid; every slot in (nearly) every row
    const int64_t n3 = 64 * 64 * 64;
    const std::vector<int32_t> S7{-4096, -64, -1, 0, 1, 64, 4096};
    const std::vector<double> v7{-1., -1., -1., 6., -1., -1., -1.};
    const std::vector<unsigned long long> c7{258048, 258048, 258048, 262144, 258048, 258048, 258048};
    stage2("poisson64", slots(S7, v7, false, {0x7f, 0x7e}), c7, n3, false);
    stage2("poisson1024", slots({-1048576, -1024, -1, 0, 1, 1024, 1048576}, v7, false, {0x7f}), std::vector<unsigned long long>(7, 1ull << 30),
           (int64_t)1 << 30, false);
    stage2("force-rare", slots(S7, v7, false, {0x7f, 0x7e}), c7, n3, true);
    // row block of 64 planes: two halo slots behind the common ones, one plane (4096 rows) each
    std::vector<int32_t> S9(S7);
    S9.push_back(8192); S9.push_back(262144);
    std::vector<double> v9(v7);
    v9.push_back(-1.); v9.push_back(-1.);
    std::vector<unsigned long long> c9(c7);
    c9.push_back(4096); c9.push_back(4096);
    stage2("row-block", slots(S9, v9, false, {0x7f, 0xfe, 0x17f}), c9, n3, false);
    // the same offsets with the largest one leading its rows
    stage2("lead", slots(S9, v9, true, {0x1ff, 0x17f, 0x0ff}), c9, n3, false);
    stage2("ninth-slot", slots(S9, v9, true, {0x1ff, 0x17f, 0x0ff}), std::vector<unsigned long long>(9, 262144), n3, false);
    std::vector<int32_t> S10(S9);
    S10.push_back(300000);
    std::vector<double> v10(v9);
    v10.push_back(-1.);
    stage2("lead-nine-ascending", slots(S10, v10, true, {0x3ff}), std::vector<unsigned long long>(10, 262144), n3, false);
    return 0;
}
