// The host plan of the even-odd (red-black) preconditioned DiracOp (evenodd.hip): the two-colouring of a pure hopping matrix D,
// its check, the index lists of the two colours and the half matrices D_eo / D_oe.  Pure host code — plain arrays in, plain
// vectors out, no HIP header — tests/cpp/evenodd_plan_check.cpp runs it on the CPU.
//
// The rules:
//   * without a caller parity the graph of D + D^T is two-coloured breadth first.  Components are visited in order of their
//     smallest row, and that row — the component's root — is even; a row without entries is a component of its own, hence even.
//     A row's colour is the parity of its distance from the root;
//   * the parity, computed or given, is then CHECKED against the matrix: the first stored entry (rows ascending, a row's entries
//     in stored order) that joins two rows of equal colour — a diagonal entry, an edge of an odd cycle, a wrong caller bit —
//     makes the plan fail and is named in the message;
//   * even[] / odd[] list the full-system rows of each colour, ascending; index[r] is row r's place in its list;
//   * D_eo (n_e x n_o) holds the even rows, D_oe (n_o x n_e) the odd ones, both CSR: rows in list order, columns renumbered by
//     index[], a row's entries IN STORED ORDER — the half applies then sum a row in the order the full apply does.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace mgcr {

struct HalfCsr {
    int64_t nrow = 0, ncol = 0;
    std::vector<int64_t> rowptr, col;
    std::vector<double> val_ri;   // interleaved (re, im)
};

struct EvenOddPlan {
    int64_t n = 0;
    std::vector<int8_t> parity;        // [n] 0 even, 1 odd
    std::vector<int64_t> even, odd;    // ascending full-system rows
    std::vector<int64_t> index;        // [n] place of the row in its colour's list
    HalfCsr eo, oe;                    // D_eo, D_oe
    int64_t bad_row = -1, bad_col = -1;   // the entry the check refused
};

// breadth-first two-colouring of D + D^T (see the rules above); the matrix is taken as it is, nothing is checked here
inline void evenodd_colour(int64_t n, const int64_t *rowptr, const int64_t *col, std::vector<int8_t> &parity) {
    const int64_t nnz = n > 0 ? rowptr[n] : 0;
    // the transposed pattern: who points at me
    std::vector<int64_t> tptr((size_t)n + 1, 0), tcol((size_t)nnz);
    for (int64_t e = 0; e < nnz; e++) tptr[(size_t)col[e] + 1]++;
    for (int64_t r = 0; r < n; r++) tptr[(size_t)r + 1] += tptr[(size_t)r];
    {
        std::vector<int64_t> fill(tptr.begin(), tptr.end() - 1);
        for (int64_t r = 0; r < n; r++)
            for (int64_t e = rowptr[r]; e < rowptr[r + 1]; e++) tcol[(size_t)fill[(size_t)col[e]]++] = r;
    }
    parity.assign((size_t)n, (int8_t)-1);
    std::vector<int64_t> queue;
    queue.reserve((size_t)n);
    for (int64_t root = 0; root < n; root++) {
        if (parity[(size_t)root] >= 0) continue;
        parity[(size_t)root] = 0;
        queue.clear();
        queue.push_back(root);
        for (size_t head = 0; head < queue.size(); head++) {
            const int64_t r = queue[head];
            const int8_t other = (int8_t)(1 - parity[(size_t)r]);
            for (int64_t e = rowptr[r]; e < rowptr[r + 1]; e++) {
                const int64_t c = col[e];
                if (parity[(size_t)c] < 0) { parity[(size_t)c] = other; queue.push_back(c); }
            }
            for (int64_t e = tptr[(size_t)r]; e < tptr[(size_t)r + 1]; e++) {
                const int64_t c = tcol[(size_t)e];
                if (parity[(size_t)c] < 0) { parity[(size_t)c] = other; queue.push_back(c); }
            }
        }
    }
}

// false (with *err and the plan's bad_row / bad_col filled where an entry is to blame): the caller answers MGCR_ERR_INVALID
inline bool evenodd_plan_build(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri, const int8_t *parity_in,
                               EvenOddPlan *out, std::string *err) {
    char msg[256];
    auto fail = [&](const char *m) { if (err) *err = m; return false; };
    if (n < 0 || !rowptr || !out) return fail("even-odd plan: bad argument");
    if (rowptr[0] != 0) return fail("even-odd plan: rowptr[0] must be 0");
    for (int64_t r = 0; r < n; r++)
        if (rowptr[r + 1] < rowptr[r]) {
            snprintf(msg, sizeof msg, "even-odd plan: rowptr is not non-decreasing at row %lld", (long long)r);
            return fail(msg);
        }
    const int64_t nnz = rowptr[n];
    if (nnz > 0 && (!col || !val_ri)) return fail("even-odd plan: null column or value array");
    for (int64_t e = 0; e < nnz; e++)
        if (col[e] < 0 || col[e] >= n) {
            snprintf(msg, sizeof msg, "even-odd plan: column index %lld is outside [0, %lld)", (long long)col[e], (long long)n);
            return fail(msg);
        }
    EvenOddPlan &p = *out;
    p = EvenOddPlan();
    p.n = n;
    if (parity_in) {
        p.parity.assign(parity_in, parity_in + n);
        for (int64_t r = 0; r < n; r++)
            if (p.parity[(size_t)r] != 0 && p.parity[(size_t)r] != 1) {
                snprintf(msg, sizeof msg, "even-odd plan: parity[%lld] = %d is neither 0 (even) nor 1 (odd)", (long long)r, (int)p.parity[(size_t)r]);
                return fail(msg);
            }
    } else {
        evenodd_colour(n, rowptr, col, p.parity);
    }
    for (int64_t r = 0; r < n; r++)
        for (int64_t e = rowptr[r]; e < rowptr[r + 1]; e++)
            if (p.parity[(size_t)r] == p.parity[(size_t)col[e]]) {
                p.bad_row = r;
                p.bad_col = col[e];
                snprintf(msg, sizeof msg,
                         "even-odd plan: entry (row %lld, column %lld) joins two %s rows%s: the matrix must be a pure hopping matrix that couples even to odd rows only",
                         (long long)r, (long long)col[e], p.parity[(size_t)r] ? "odd" : "even", r == col[e] ? " (a diagonal entry)" : "");
                return fail(msg);
            }
    p.index.assign((size_t)n, 0);
    for (int64_t r = 0; r < n; r++) {
        std::vector<int64_t> &list = p.parity[(size_t)r] ? p.odd : p.even;
        p.index[(size_t)r] = (int64_t)list.size();
        list.push_back(r);
    }
    auto half = [&](const std::vector<int64_t> &rows, int64_t ncol, HalfCsr &h) {
        h.nrow = (int64_t)rows.size();
        h.ncol = ncol;
        h.rowptr.assign(1, 0);
        for (int64_t r : rows) {
            for (int64_t e = rowptr[r]; e < rowptr[r + 1]; e++) {
                h.col.push_back(p.index[(size_t)col[e]]);
                h.val_ri.push_back(val_ri[2 * e]);
                h.val_ri.push_back(val_ri[2 * e + 1]);
            }
            h.rowptr.push_back((int64_t)h.col.size());
        }
    };
    half(p.even, (int64_t)p.odd.size(), p.eo);
    half(p.odd, (int64_t)p.even.size(), p.oe);
    return true;
}

// The plan of a matrix that may store a site diagonal (evenodd_diag.hip): the diagonal entries are taken out and added up per row,
// in stored order, into d[n] (interleaved (re, im); 0 for a row without one) — *n_diag counts them —, and evenodd_plan_build runs
// on what is left: the colouring and its check never see a diagonal entry, an odd cycle or a wrong caller bit is refused with the
// message above, and the halves hold the off-diagonal entries in stored order.
inline bool evenodd_plan_build_diag(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri, const int8_t *parity_in,
                                    EvenOddPlan *out, std::vector<double> *d, int64_t *n_diag, std::string *err) {
    auto fail = [&](const char *m) { if (err) *err = m; return false; };
    if (n < 0 || !rowptr || !out || !d) return fail("even-odd plan: bad argument");
    // (everything else about the arrays is checked by evenodd_plan_build, on the copy; what must hold before the copy is made:)
    if (rowptr[0] != 0) return fail("even-odd plan: rowptr[0] must be 0");
    for (int64_t r = 0; r < n; r++)
        if (rowptr[r + 1] < rowptr[r]) {
            char msg[256];
            snprintf(msg, sizeof msg, "even-odd plan: rowptr is not non-decreasing at row %lld", (long long)r);
            return fail(msg);
        }
    const int64_t nnz = rowptr[n];
    if (nnz > 0 && (!col || !val_ri)) return fail("even-odd plan: null column or value array");
    d->assign(2 * (size_t)n, 0.);
    std::vector<int64_t> rp((size_t)n + 1, 0), cc;
    std::vector<double> vv;
    cc.reserve((size_t)nnz);
    vv.reserve(2 * (size_t)nnz);
    int64_t nd = 0;
    for (int64_t r = 0; r < n; r++) {
        for (int64_t e = rowptr[r]; e < rowptr[r + 1]; e++) {
            if (col[e] == r) {
                (*d)[2 * (size_t)r] += val_ri[2 * e];
                (*d)[2 * (size_t)r + 1] += val_ri[2 * e + 1];
                nd++;
            } else {
                cc.push_back(col[e]);
                vv.push_back(val_ri[2 * e]);
                vv.push_back(val_ri[2 * e + 1]);
            }
        }
        rp[(size_t)r + 1] = (int64_t)cc.size();
    }
    if (n_diag) *n_diag = nd;
    return evenodd_plan_build(n, rp.data(), cc.data(), vv.data(), parity_in, out, err);
}

// The plan of a matrix with a dense block per SITE on its diagonal (evenodd_block.hip): sites are runs of bs consecutive rows, row r
// belongs to site r / bs.  The stored entries inside a site are taken out and added up, in stored order, into that site's bs x bs
// block (row-major, interleaved (re, im); 0 where nothing is stored) — *n_in_site counts them —, and what is left, the entries
// between different sites, is coloured and split as above.  The rows of a site share one colour: without a caller parity the SITE
// graph is two-coloured by evenodd_colour (components in order of their smallest site, the root even) and the colour expanded to
// the rows; a caller parity must be constant inside every site (the first row that differs from its site's first row is named).
// evenodd_plan_build then checks the row parity against the inter-site entries — an odd cycle of sites or a wrong caller bit is
// refused with the entry named — and makes the halves.  The lists stay ascending, so half-site s' occupies the half rows
// s' bs .. s' bs + bs - 1, and blocks_even / blocks_odd hold the blocks of the even / odd sites in that order.
constexpr int32_t EO_BLOCK_MAX = 16;
inline bool evenodd_plan_build_block(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri, int32_t bs,
                                     const int8_t *parity_in, EvenOddPlan *out, std::vector<double> *blocks_even,
                                     std::vector<double> *blocks_odd, int64_t *n_in_site, std::string *err) {
    char msg[256];
    auto fail = [&](const char *m) { if (err) *err = m; return false; };
    if (n < 0 || !rowptr || !out || !blocks_even || !blocks_odd) return fail("even-odd plan: bad argument");
    if (bs < 1 || bs > EO_BLOCK_MAX) {
        snprintf(msg, sizeof msg, "even-odd plan: block size bs = %d, 1 .. %d are supported", (int)bs, (int)EO_BLOCK_MAX);
        return fail(msg);
    }
    if (n % bs != 0) {
        snprintf(msg, sizeof msg, "even-odd plan: n = %lld rows are no whole number of sites of bs = %d rows", (long long)n, (int)bs);
        return fail(msg);
    }
    if (rowptr[0] != 0) return fail("even-odd plan: rowptr[0] must be 0");
    for (int64_t r = 0; r < n; r++)
        if (rowptr[r + 1] < rowptr[r]) {
            snprintf(msg, sizeof msg, "even-odd plan: rowptr is not non-decreasing at row %lld", (long long)r);
            return fail(msg);
        }
    const int64_t nnz = rowptr[n];
    if (nnz > 0 && (!col || !val_ri)) return fail("even-odd plan: null column or value array");
    for (int64_t e = 0; e < nnz; e++)
        if (col[e] < 0 || col[e] >= n) {
            snprintf(msg, sizeof msg, "even-odd plan: column index %lld is outside [0, %lld)", (long long)col[e], (long long)n);
            return fail(msg);
        }
    const int64_t ns = n / bs;
    const size_t bb = 2 * (size_t)bs * (size_t)bs;
    std::vector<double> blocks(bb * (size_t)ns, 0.);
    std::vector<int64_t> rp((size_t)n + 1, 0), cc, sp((size_t)ns + 1, 0), sc;
    std::vector<double> vv;
    cc.reserve((size_t)nnz);
    sc.reserve((size_t)nnz);
    vv.reserve(2 * (size_t)nnz);
    int64_t nin = 0;
    for (int64_t r = 0; r < n; r++) {
        const int64_t s = r / bs;
        for (int64_t e = rowptr[r]; e < rowptr[r + 1]; e++) {
            if (col[e] / bs == s) {
                const size_t at = bb * (size_t)s + 2 * ((size_t)(r - s * bs) * (size_t)bs + (size_t)(col[e] - s * bs));
                blocks[at] += val_ri[2 * e];
                blocks[at + 1] += val_ri[2 * e + 1];
                nin++;
            } else {
                cc.push_back(col[e]);
                sc.push_back(col[e] / bs);
                vv.push_back(val_ri[2 * e]);
                vv.push_back(val_ri[2 * e + 1]);
            }
        }
        rp[(size_t)r + 1] = (int64_t)cc.size();
        sp[(size_t)s + 1] = (int64_t)sc.size();
    }
    if (n_in_site) *n_in_site = nin;
    std::vector<int8_t> par((size_t)n, 0);
    if (parity_in) {
        for (int64_t r = 0; r < n; r++) {
            if (parity_in[r] != 0 && parity_in[r] != 1) {
                snprintf(msg, sizeof msg, "even-odd plan: parity[%lld] = %d is neither 0 (even) nor 1 (odd)", (long long)r, (int)parity_in[r]);
                return fail(msg);
            }
            if (parity_in[r] != parity_in[r / bs * bs]) {
                snprintf(msg, sizeof msg, "even-odd plan: parity[%lld] differs from parity[%lld] inside site %lld: the rows of a site share one colour",
                         (long long)r, (long long)(r / bs * bs), (long long)(r / bs));
                return fail(msg);
            }
            par[(size_t)r] = parity_in[r];
        }
    } else {
        std::vector<int8_t> site_par;
        evenodd_colour(ns, sp.data(), sc.data(), site_par);
        for (int64_t r = 0; r < n; r++) par[(size_t)r] = site_par[(size_t)(r / bs)];
    }
    if (!evenodd_plan_build(n, rp.data(), cc.data(), vv.data(), par.data(), out, err)) return false;
    blocks_even->clear();
    blocks_odd->clear();
    for (int64_t s = 0; s < ns; s++) {
        std::vector<double> &dst = par[(size_t)(s * bs)] ? *blocks_odd : *blocks_even;
        dst.insert(dst.end(), blocks.begin() + (ptrdiff_t)(bb * (size_t)s), blocks.begin() + (ptrdiff_t)(bb * (size_t)(s + 1)));
    }
    return true;
}

}  // namespace mgcr
