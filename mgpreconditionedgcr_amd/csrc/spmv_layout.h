// Host decisions of the Sparse format build (spmv_build.hip) that are pure arithmetic: plain data in, plain data out, no HIP
// header — tests/cpp/spmv_layout_check.cpp runs them on the CPU.  The kernels' sizes (TAIL_CAP, STEN_TILE, ...) come in as arguments.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace mgcr {

// Picks the ELL width that minimises the bytes one SpMV streams, from the row-length histogram.
inline int32_t choose_width(const std::vector<int64_t> &hist, int64_t nrow, int32_t maxlen) {
    // rows_ge[w] = #rows with len >= w ;  tail_nnz(W) = sum_{w > W} rows_ge[w]
    std::vector<int64_t> rows_ge(maxlen + 2, 0);
    for (int32_t w = maxlen; w >= 0; w--) rows_ge[w] = rows_ge[w + 1] + hist[w];
    std::vector<int64_t> tail(maxlen + 2, 0);
    for (int32_t w = maxlen - 1; w >= 0; w--) tail[w] = tail[w + 1] + rows_ge[w + 1];
    int32_t best = maxlen;
    double best_cost = 1e300;
    for (int32_t W = 0; W <= maxlen; W++) {
        // 20 B per stored entry; a tail entry also costs an uncoalesced row visit (~x2) and each
        // tail row a read-modify-write of y plus bookkeeping (~64 B)
        double cost = 20. * (double)W * (double)nrow + 40. * (double)tail[W] + 64. * (double)rows_ge[W + 1];
        if (cost < best_cost) { best_cost = cost; best = W; }
    }
    return best;
}

inline int32_t choose_lanes(int64_t nrow, int32_t W) {
    // one thread per row (entries summed in CSR order, like the reference) whenever that alone
    // fills the machine; otherwise split rows over 2..16 lanes while padding stays below 10 %
    if (W <= 8 || nrow >= (int64_t)1 << 18) return 1;
    int32_t best = 1;
    for (int32_t L = 2; L <= 16; L *= 2) {
        int32_t padded = (W + L - 1) / L * L;
        if ((padded - W) * 10 > W) continue;
        best = L;
        if (nrow * L >= (int64_t)1 << 17) break;
    }
    return best;
}

struct TailChunk { int32_t first, last, e0, e1; };   // one record of CsrDev::tail_chunk (the layout of an int4)
// deals the tail rows (tptr: their entry ranges) to workgroups: runs of consecutive tail rows of at most `cap` entries / `max_rows`
// rows, and the rows longer than a chunk on their own
inline void deal_tail(const std::vector<int32_t> &tptr, int32_t cap, int32_t max_rows, std::vector<TailChunk> &chunks,
                      std::vector<int32_t> &long_rows) {
    const int32_t nt = (int32_t)tptr.size() - 1;
    int32_t i = 0;
    while (i < nt) {
        if (tptr[(size_t)i + 1] - tptr[(size_t)i] > cap) { long_rows.push_back(i); i++; continue; }
        const int32_t first = i, e0 = tptr[(size_t)i];
        while (i < nt && i - first < max_rows && tptr[(size_t)i + 1] - e0 <= cap) i++;
        chunks.push_back(TailChunk{first, i, e0, tptr[(size_t)i]});
    }
}

// window kernel (tiles of `win_rows` rows): per tile its first tail row; per row its index into the tail-row list (-1: none or long)
inline void window_tail_tables(const std::vector<int32_t> &trows, const std::vector<int32_t> &tptr, int64_t nrow, int32_t win_rows,
                               int32_t cap, std::vector<int32_t> &tile_tail, std::vector<int32_t> &row_tail) {
    const int64_t ntiles = (nrow + win_rows - 1) / win_rows;
    tile_tail.assign((size_t)ntiles + 1, (int32_t)trows.size());
    row_tail.assign((size_t)nrow, -1);
    for (int32_t t = (int32_t)trows.size() - 1; t >= 0; t--) {
        tile_tail[(size_t)(trows[(size_t)t] / win_rows)] = t;
        if (tptr[(size_t)t + 1] - tptr[(size_t)t] <= cap) row_tail[(size_t)trows[(size_t)t]] = t;
    }
    for (int64_t q = ntiles - 1; q >= 0; q--)   // tiles without tail rows: the next tile's first
        if (tile_tail[(size_t)q] > tile_tail[(size_t)q + 1]) tile_tail[(size_t)q] = tile_tail[(size_t)q + 1];
}

// ---- stencil view, stage 1: is the mode-1 dictionary (off, re, im: [npat][W]) a family of sub-stencils of one stencil? ----
struct StenSlots {
    bool view = false;             // false: no view
    bool lead = false;             // the slot with the largest offset comes first in the rows that have it
    std::vector<int32_t> S;        // ascending offsets of all patterns' non-zero entries
    std::vector<uint16_t> pbits;   // per pattern: which slots it has (bit s = slot s of S)
    double re[16] = {}, im[16] = {};   // the one value of each slot
};
inline StenSlots sten_stage1(const std::vector<int32_t> &off, const std::vector<double> &re, const std::vector<double> &im, int npat,
                             int32_t W, int max_slots) {
    StenSlots o;
    const size_t ne = (size_t)npat * W;
    for (size_t e = 0; e < ne; e++)
        if (re[e] != 0. || im[e] != 0.) o.S.push_back(off[e]);
    std::sort(o.S.begin(), o.S.end());
    o.S.erase(std::unique(o.S.begin(), o.S.end()), o.S.end());
    const int ns = (int)o.S.size();
    if (ns < 1 || ns > max_slots) return o;
    o.pbits.assign((size_t)npat, 0);
    std::vector<char> have((size_t)ns, 0);
    // The slot with the largest offset may come FIRST in the rows that have it: the halo column of a row block's first plane (rows
    // handed over in global column order — the neighbour below has the smallest global column and, as local column nloc + k, the
    // largest offset).  Such a LEADING slot is summed before the others (kernel slot 7 of the rare layout, RowMat::sten_pre), so the
    // row sum keeps its storage order.  lead_mode: 0 undecided, 1 leading, 2 in ascending position.
    int lead_mode = 0;
    for (int p = 0; p < npat; p++) {
        int last = -1, count = 0;
        bool lead_here = false;
        for (int32_t w = 0; w < W; w++) {
            const size_t e = (size_t)p * W + w;
            if (re[e] == 0. && im[e] == 0.) continue;
            const int s = (int)(std::lower_bound(o.S.begin(), o.S.end(), off[e]) - o.S.begin());
            if (count == 0 && s == ns - 1 && ns > 1) lead_here = true;      // (decided below, once the pattern is known to have more entries)
            else {
                if (s <= last) return o;   // a repeated or descending column: not a sub-stencil in storage order
                last = s;
                if (s == ns - 1 && ns > 1 && count > 0) {
                    if (lead_mode == 1) return o;
                    lead_mode = 2;
                }
            }
            count++;
            if (!have[(size_t)s]) { have[(size_t)s] = 1; o.re[s] = re[e]; o.im[s] = im[e]; }
            else if (memcmp(&o.re[s], &re[e], sizeof(double)) || memcmp(&o.im[s], &im[e], sizeof(double))) return o;  // value differs between patterns
            o.pbits[(size_t)p] |= (uint16_t)(1u << s);
        }
        if (lead_here && count > 1) {
            if (lead_mode == 2) return o;
            lead_mode = 1;
        }
    }
    o.lead = lead_mode == 1; o.view = true;
    return o;
}

// ---- stage 2: the layout the kernels read (spmv_dev.h sten_row_product), from counts[s] = rows that have slot s ----
struct StenLimits { int common, near_tile, near_fused; };   // STEN_COMMON, STEN_TILE / 2, RED_THREADS / 2
struct StenLayout {
    bool view = false;             // false: no view (more than `common` slots besides a leading one)
    int slot_of[16] = {};          // slot of S -> kernel slot
    int32_t kernel_ns = 0, stride = 0, pre = 0, halo = 0, halo_f = 0;   // kernel_ns: common or common + 2
    uint32_t rare = 0, near = 0, near_f = 0;
    int32_t off[16] = {};          // offsets and values in kernel layout
    double re[16] = {}, im[16] = {};
    int64_t reach = -1;            // rare-tail layout: largest |offset| of the common slots (-1: the dictionary's stays)
    std::vector<uint16_t> pmask;   // per pattern: its kernel slots
};
inline StenLayout sten_stage2(const StenSlots &s1, const std::vector<unsigned long long> &counts, int64_t nrow, bool force_rare,
                              const StenLimits &lim) {
    StenLayout o;
    const int ns = (int)s1.S.size(), C = lim.common;
    const bool lead = s1.lead;
    // Rare tail: the slots fewer than 1/16 of the rows have are the LAST one or two of the list (halo columns of a slab's first /
    // last plane: local column nloc + slot lies behind every owned column) and at most 7 common ones remain: common slots -> 0..6,
    // rare ones -> 7, 8.  Otherwise every slot is treated as common, 7 or 9 of them.
    // A leading slot (stage 1) always takes the rare layout: kernel slot 7, summed first; one rare slot behind the common ones may
    // then follow as slot 8.
    int nrare = 0;
    const int nsl = lead ? ns - 1 : ns;    // the slots in ascending position
    while (nrare < (lead ? 1 : 2) && nrare < nsl - 1 && (int64_t)counts[(size_t)(nsl - 1 - nrare)] * 16 < nrow) nrare++;
    if (lead && nrare == 0 && nsl == C + 1) nrare = 1;   // (the upper halo column of a block of few planes: not rare by count, but the ninth slot)
    bool tail = (nrare > 0 || lead) && nsl - nrare <= C;
    for (int s = 0; tail && !lead && s < nsl - nrare; s++)
        if ((int64_t)counts[(size_t)s] * 16 < nrow) tail = false;   // a rare slot among the common ones: no special treatment
    if (lead && !tail) return o;   // (the dictionary kernels keep the storage order)
    if (ns <= C && force_rare) { tail = true; nrare = 0; }   // measurement aid: a single-GPU operator through the kernels of a distributed row block
    for (int s = 0; s < ns; s++) {
        if (lead && s == ns - 1) o.slot_of[s] = C;                                           // summed first
        else if (tail && s >= nsl - nrare) o.slot_of[s] = C + (lead ? 1 : 0) + (s - (nsl - nrare));
        else o.slot_of[s] = s;
    }
    o.view = true;
    o.kernel_ns = tail || ns > C ? C + 2 : C;
    o.stride = o.kernel_ns == C ? 8 : 16;
    o.rare = tail ? 3u << C : 0u; o.pre = lead ? 1 : 0;
    o.pmask.assign(s1.pbits.size(), 0);
    for (size_t p = 0; p < s1.pbits.size(); p++)
        for (int s = 0; s < ns; s++)
            if (s1.pbits[p] >> s & 1u) o.pmask[p] |= (uint16_t)(1u << o.slot_of[s]);
    for (int s = 0; s < ns; s++) { o.off[o.slot_of[s]] = s1.S[(size_t)s]; o.re[o.slot_of[s]] = s1.re[s]; o.im[o.slot_of[s]] = s1.im[s]; }
    // slots close to the diagonal (|offset| <= STEN_TILE / 2, e.g. +-1 and +-n of a 3-D grid up to n = 256) are read by several rows
    // of the same workgroup: the stand-alone kernel stages x once in an LDS window and serves them from there (near, halo); the
    // same for the fused GCR step kernels, whose window spans RED_THREADS rows (near_f, halo_f)
    auto near = [&](int32_t within, uint32_t &mask, int32_t &halo) {
        for (int s = 0; s < ns; s++) {
            if (tail && o.slot_of[s] >= C) continue;
            const int32_t a = s1.S[(size_t)s] < 0 ? -s1.S[(size_t)s] : s1.S[(size_t)s];
            if (a <= within) { mask |= 1u << o.slot_of[s]; halo = std::max(halo, a); }
        }
        if (halo < 32) { mask = 0; halo = 0; }   // only +-1-like neighbours: L1 serves those as well
    };
    near(lim.near_tile, o.near, o.halo);
    near(lim.near_fused, o.near_f, o.halo_f);
    if (tail) {
        // how far a row's gathers reach decides the row -> workgroup map of the GCR step kernels (gcr_dev.h): the two
        // rare slots (halo columns, "nloc rows away") concern one plane each and must not count
        o.reach = 0;
        for (int s = 0; s < ns; s++)
            if (o.slot_of[s] < C) o.reach = std::max<int64_t>(o.reach, s1.S[(size_t)s] < 0 ? -(int64_t)s1.S[(size_t)s] : (int64_t)s1.S[(size_t)s]);
    }
    return o;
}

}  // namespace mgcr
