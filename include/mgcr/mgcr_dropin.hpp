// mgcr_dropin.hpp — the reference's C++ host interface (Mesh / Field / Operator / Sparse / DiracOp /
// Dense / HierarchicalSparse / GCR_Param / MG_Param / GCR / MG / read_data) re-created on top of the
// C ABI of libmgcr_hip.so (include/mgcr.h).  Same class names, template parameters, constructor and
// method signatures as jing2li/MGPreconditionedGCR @ 2024_10_08 (cited per class, paths relative to
// the reference root), so that code written against the reference — e.g. k_critical_mg_precond(),
// src/main.cpp:834-875 — compiles unchanged with `-Iinclude/mgcr` and links `-lmgcr_hip`.
// Written from scratch: no reference code is reused; the data lives in HBM and every operation is a
// HIP kernel.  Error behaviour follows the reference: a failed check prints the message and
// aborts (the reference uses assert / exit(1), src/Fields.h:14,279-283).
#ifndef MGCR_DROPIN_HPP
#define MGCR_DROPIN_HPP

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../mgcr.h"

namespace mgcr_detail {
inline void ok(int rc, const char *what) {
    if (rc != MGCR_OK) {
        std::fprintf(stderr, "%s: %s\n", what, mgcr_last_error());
        std::abort();
    }
}
inline void ensure_init() {
    static bool done = false;
    if (!done) {
        const char *lr = std::getenv("LOCAL_RANK");
        ok(mgcr_init(lr ? std::atoi(lr) : 0), "mgcr_init");
        done = true;
    }
}
typedef std::complex<double> cd;
}  // namespace mgcr_detail

// ------------------------------------------------------------------------------------------------
// Mesh — src/Mesh.h:13-64.  Row-major N-D index algebra and the 4-D sub-block decomposition.
// ------------------------------------------------------------------------------------------------
template <typename num_type>
class Mesh {
public:
    Mesh() = default;
    Mesh(num_type const *index_dims, int num_dims) : dim(index_dims, index_dims + num_dims) {}
    static num_type ind_loc(num_type const *index, num_type const *dims, int ndims) {  // :146-154
        num_type loc = index[0];
        for (int i = 1; i < ndims; i++) loc = loc * dims[i] + index[i];
        return loc;
    }
    num_type ind_loc(num_type const *index) const { return ind_loc(index, dim.data(), (int)dim.size()); }
    static num_type *alloc_loc_ind(num_type loc, num_type const *dims, int ndims) {  // :368-382 (caller delete[]s)
        num_type *ind = new num_type[ndims];
        for (int i = ndims - 1; i >= 0; i--) { ind[i] = loc % dims[i]; loc /= dims[i]; }
        return ind;
    }
    num_type *alloc_loc_ind(num_type loc) const { return alloc_loc_ind(loc, dim.data(), (int)dim.size()); }
    // :236-298 — block_map[block][offset] = spacetime location; block index row-major over block_dim
    void blocking(num_type subblock_dim, const bool *blocked_dimensions) {
        sub_dim = subblock_dim;
        std::vector<num_type> st;
        int c = 0;
        for (size_t i = 0; i < dim.size(); i++)
            if (blocked_dimensions[i]) {
                if (dim[i] % subblock_dim) { std::fprintf(stderr, "Dimension not exactly divisible by block size!\n"); std::abort(); }
                if (c < 4) { blocked_ind[c] = (int)i; block_dim[c] = (int)(dim[i] / subblock_dim); }
                st.push_back(dim[i]);
                c++;
            }
        for (; c < 4; c++) { block_dim[c] = 1; st.push_back(1); }
        num_type nst = 1;
        for (num_type d : st) nst *= d;
        block_map.assign((size_t)get_nblocks(), std::vector<num_type>((size_t)get_block_size(), 0));
        for (num_type loc = 0; loc < nst; loc++) {
            num_type rem = loc, id[4], b = 0, off = 0;
            for (int d = 3; d >= 0; d--) { id[d] = rem % st[(size_t)d]; rem /= st[(size_t)d]; }
            for (int d = 0; d < 4; d++) {
                num_type sd = (st[(size_t)d] == 1) ? 1 : subblock_dim;
                b = b * block_dim[d] + id[d] / sd;
                off = off * subblock_dim + id[d] % sd;
            }
            block_map[(size_t)b][(size_t)off] = loc;
        }
    }
    num_type get_nblocks() const { return (num_type)block_dim[0] * block_dim[1] * block_dim[2] * block_dim[3]; }
    int *get_block_dim() { return block_dim; }
    num_type get_block_size() const { return sub_dim * sub_dim * sub_dim * sub_dim; }
    num_type *get_block_map(num_type block_idx) { return block_map[(size_t)block_idx].data(); }
    num_type get_size() const {
        num_type s = dim.empty() ? 0 : 1;
        for (num_type d : dim) s *= d;
        return s;
    }
    int get_ndim() const { return (int)dim.size(); }
    num_type *get_dims() { return dim.data(); }
    const num_type *get_dims() const { return dim.data(); }

private:
    std::vector<num_type> dim;
    num_type sub_dim = 0;
    int blocked_ind[4] = {0, 0, 0, 0};
    int block_dim[4] = {0, 0, 0, 0};
    std::vector<std::vector<num_type>> block_map;
};

// ------------------------------------------------------------------------------------------------
// Field — src/Fields.h:29-71.  Device-resident; val_at / mod_val_at work through a lazily
// synchronised host mirror so that element-wise legacy code keeps working.
// ------------------------------------------------------------------------------------------------
template <typename num_type>
class Field {
public:
    Field() = default;
    Field(Field const &f) : mesh(f.mesh) { alloc(); if (f.h) { f.to_device(); mgcr_detail::ok(mgcr_vec_copy(h, f.h), "Field copy"); } }
    explicit Field(Mesh<num_type> m) : mesh(std::move(m)) { alloc(); }
    Field(const num_type *dimensions, num_type ndim) : mesh(dimensions, (int)ndim) { alloc(); }
    Field(const num_type *dimensions, num_type ndim, std::complex<double> *field_init) : mesh(dimensions, (int)ndim) {
        alloc();
        mgcr_detail::ok(mgcr_vec_upload(h, reinterpret_cast<const double *>(field_init)), "Field upload");
    }
    ~Field() { if (h) mgcr_vec_destroy(h); }

    // :125-135 — values (rand()%2000)/1000.-1; the reference's g++ build draws the IMAGINARY part
    // first (argument evaluation order); fixed explicitly here
    void init_rand(int seed = 1) {
        num_type n = field_size();
        std::srand((unsigned)seed);
        host.resize((size_t)n);
        for (num_type i = 0; i < n; i++) {
            double im = (std::rand() % 2000) / 1000. - 1;
            double re = (std::rand() % 2000) / 1000. - 1;
            host[(size_t)i] = std::complex<double>(re, im);
        }
        host_valid = true; dev_valid = false;
    }
    void set_zero() { need(); mgcr_detail::ok(mgcr_vec_zero(h), "set_zero"); dev_only(); }
    void set_constant(std::complex<double> c) { need(); double v[2] = {c.real(), c.imag()}; mgcr_detail::ok(mgcr_vec_set_constant(h, v), "set_constant"); dev_only(); }

    num_type *alloc_get_dim() { num_type *o = (num_type *)std::malloc(sizeof(num_type) * (size_t)mesh.get_ndim()); for (int i = 0; i < mesh.get_ndim(); i++) o[i] = mesh.get_dims()[i]; return o; }
    num_type get_ndim() const { return mesh.get_ndim(); }
    num_type field_size() const { return mesh.get_size(); }
    Mesh<num_type> get_mesh() const { return mesh; }
    std::complex<double> val_at(num_type const *index) { return val_at(mesh.ind_loc(index)); }
    std::complex<double> val_at(num_type location) const {
        if (location < 0 || location >= field_size()) { std::fprintf(stderr, "Field memory access out of bound!\n"); std::abort(); }
        to_host();
        return host[(size_t)location];
    }
    void mod_val_at(num_type const *index, std::complex<double> v) { mod_val_at(mesh.ind_loc(index), v); }
    void mod_val_at(num_type location, std::complex<double> v) { to_host(); host[(size_t)location] = v; dev_valid = false; }

    Field operator+(const Field &f) const { return axpy_new(std::complex<double>(1., 0.), f); }
    Field operator-(const Field &f) const { return axpy_new(std::complex<double>(-1., 0.), f); }
    std::complex<double> dot(const Field &f) const {  // :216-226, conj on *this
        to_device(); f.to_device();
        double o[2];
        mgcr_detail::ok(mgcr_dot(h, f.h, o), "dot");
        return std::complex<double>(o[0], o[1]);
    }
    double squarednorm() const { to_device(); double o; mgcr_detail::ok(mgcr_norm2(h, &o), "squarednorm"); return o; }
    double norm() const { return std::sqrt(squarednorm()); }
    Field operator*(std::complex<double> a) const {
        Field o(*this);
        double v[2] = {a.real(), a.imag()};
        mgcr_detail::ok(mgcr_scale(o.h, v), "operator*");
        return o;
    }
    Field &operator=(const Field &f) noexcept {  // :256-286
        if (this == &f) return *this;
        if (!h) { mesh = f.mesh; alloc(); }
        if (field_size() != f.field_size()) { std::printf("Dimension mismatch.\n"); std::exit(1); }
        f.to_device();
        mgcr_detail::ok(mgcr_vec_copy(h, f.h), "operator=");
        dev_only();
        return *this;
    }
    Field &operator+=(const Field &f) { inplace(std::complex<double>(1., 0.), f); return *this; }
    Field &operator-=(const Field &f) { inplace(std::complex<double>(-1., 0.), f); return *this; }
    void normalise() { to_device(); mgcr_detail::ok(mgcr_normalise(h), "normalise"); dev_only(); }
    Field gamma5(int spinor_index) const {  // :310-339: output[index with spinor 0<->2, 1<->3] = field[i]
        Field o(mesh);
        const num_type *d = mesh.get_dims();
        if (d[spinor_index] != 4) { std::fprintf(stderr, "gamma5: the spinor dimension must have 4 entries\n"); std::abort(); }
        long long inner = 1;
        for (int k = spinor_index + 1; k < (int)mesh.get_ndim(); k++) inner *= (long long)d[k];
        to_device();
        mgcr_detail::ok(mgcr_vec_gamma5(h, o.h, inner), "gamma5");
        o.dev_only();
        return o;
    }
    // device handle (synchronised); used by the operator wrappers
    mgcr_vec_t device() const { to_device(); return h; }
    void device_written() { dev_only(); }

protected:
    Mesh<num_type> mesh;

private:
    void alloc() { mgcr_detail::ensure_init(); mgcr_detail::ok(mgcr_vec_create((int64_t)mesh.get_size(), &h), "Field alloc"); dev_valid = true; host_valid = false; }
    void need() { if (!h) alloc(); }
    void dev_only() { dev_valid = true; host_valid = false; }
    void to_host() const {
        if (host_valid) return;
        host.resize((size_t)field_size());
        mgcr_detail::ok(mgcr_vec_download(h, reinterpret_cast<double *>(host.data())), "download");
        host_valid = true;
    }
    void to_device() const {
        if (dev_valid) return;
        mgcr_detail::ok(mgcr_vec_upload(h, reinterpret_cast<const double *>(host.data())), "upload");
        dev_valid = true;
    }
    Field axpy_new(std::complex<double> a, const Field &f) const {
        if (field_size() != f.field_size()) { std::fprintf(stderr, "Lengths of two fields do not match!\n"); std::abort(); }
        Field o(mesh);
        to_device(); f.to_device();
        double v[2] = {a.real(), a.imag()};
        mgcr_detail::ok(mgcr_add_scaled(o.h, h, v, f.h), "operator+-");
        return o;
    }
    void inplace(std::complex<double> a, const Field &f) {
        if (field_size() != f.field_size()) { std::fprintf(stderr, "Field dimensions do not match!\n"); std::abort(); }
        to_device(); f.to_device();
        double v[2] = {a.real(), a.imag()};
        mgcr_detail::ok(mgcr_axpy(v, f.h, h), "operator+=");
        dev_only();
    }
    mutable mgcr_vec_t h = nullptr;
    mutable std::vector<std::complex<double>> host;
    mutable bool host_valid = false, dev_valid = false;
};

// ------------------------------------------------------------------------------------------------
// MultiField — a block of k Fields on one mesh (multi-RHS; the reference has no counterpart, include/mgcr.h
// mgcr_mvec_*).  Lives on the device with the columns interleaved; columns go in and out as Fields.
// ------------------------------------------------------------------------------------------------
template <typename num_type>
class MultiField {
public:
    MultiField(Mesh<num_type> m, int ncols) : mesh(std::move(m)), k(ncols) { alloc(); }
    // k Fields of one size, packed on the device
    explicit MultiField(const std::vector<const Field<num_type> *> &fields) : mesh(first(fields)->get_mesh()), k((int)fields.size()) {
        alloc();
        for (int j = 0; j < k; j++) set_column(j, *fields[(size_t)j]);
    }
    explicit MultiField(const std::vector<Field<num_type>> &fields) : MultiField(pointers(fields)) {}
    MultiField(MultiField const &o) : mesh(o.mesh), k(o.k) { alloc(); for (int j = 0; j < k; j++) set_column(j, o.column(j)); }
    MultiField &operator=(MultiField const &) = delete;
    ~MultiField() { if (h) mgcr_mvec_destroy(h); }

    int ncols() const { return k; }
    num_type field_size() const { return mesh.get_size(); }
    Mesh<num_type> get_mesh() const { return mesh; }
    Field<num_type> column(int j) const {
        Field<num_type> out(mesh);
        mgcr_detail::ok(mgcr_mvec_get_column(h, j, out.device()), "MultiField::column");
        out.device_written();
        return out;
    }
    void set_column(int j, const Field<num_type> &f) {
        if (f.field_size() != field_size()) { std::fprintf(stderr, "Lengths of two fields do not match!\n"); std::abort(); }
        mgcr_detail::ok(mgcr_mvec_set_column(h, j, f.device()), "MultiField::set_column");
    }
    void set_zero() { mgcr_detail::ok(mgcr_mvec_zero(h), "MultiField::set_zero"); }
    // <this_j, f_j> (conj on *this) and |this_j|^2 for every column, in one pass each
    std::vector<std::complex<double>> dot(const MultiField &f) const {
        std::vector<double> o((size_t)2 * k);
        mgcr_detail::ok(mgcr_mvec_dot(h, f.h, o.data()), "MultiField::dot");
        std::vector<std::complex<double>> r((size_t)k);
        for (int j = 0; j < k; j++) r[(size_t)j] = std::complex<double>(o[(size_t)2 * j], o[(size_t)2 * j + 1]);
        return r;
    }
    std::vector<double> squarednorm() const {
        std::vector<double> o((size_t)k);
        mgcr_detail::ok(mgcr_mvec_norm2(h, o.data()), "MultiField::squarednorm");
        return o;
    }
    // this_j += alpha_j x_j
    void axpy(const std::vector<std::complex<double>> &alpha, const MultiField &x) {
        if ((int)alpha.size() != k) { std::fprintf(stderr, "MultiField::axpy: one coefficient per column\n"); std::abort(); }
        mgcr_detail::ok(mgcr_mvec_axpy(reinterpret_cast<const double *>(alpha.data()), x.h, h), "MultiField::axpy");
    }
    mgcr_mvec_t device() const { return h; }

private:
    static const Field<num_type> *first(const std::vector<const Field<num_type> *> &fields) {
        if (fields.empty()) { std::fprintf(stderr, "MultiField: no Fields\n"); std::abort(); }
        return fields[0];
    }
    static std::vector<const Field<num_type> *> pointers(const std::vector<Field<num_type>> &fields) {
        std::vector<const Field<num_type> *> p;
        for (const Field<num_type> &f : fields) p.push_back(&f);
        return p;
    }
    void alloc() { mgcr_detail::ensure_init(); mgcr_detail::ok(mgcr_mvec_create((int64_t)mesh.get_size(), k, &h), "MultiField alloc"); }
    Mesh<num_type> mesh;
    int k = 0;
    mgcr_mvec_t h = nullptr;
};

// ------------------------------------------------------------------------------------------------
// Operator — src/Operator.h:16-29
// ------------------------------------------------------------------------------------------------
template <typename num_type>
class Operator {
public:
    virtual Field<num_type> operator()(const Field<num_type> &) = 0;
    num_type get_dim() const { return dim; }
    virtual void initialise(Operator *) {}
    virtual std::complex<double> val_at(num_type location) const = 0;
    virtual std::complex<double> val_at(num_type row, num_type col) const = 0;
    virtual ~Operator() = default;
    // device handle of this operator (built on demand); nullptr for purely host-defined operators
    virtual mgcr_op_t handle() { return nullptr; }
    // Y = op(X) for a block of Fields: the matrix is streamed once for all columns, column j has the bits of op(X.column(j))
    // (extension, mgcr_op_apply_multi: Sparse, DiracOp, MultiDiracOp, HierarchicalSparse / Dense)
    MultiField<num_type> apply_multi(const MultiField<num_type> &X) {
        mgcr_op_t op = handle();
        if (!op) { std::fprintf(stderr, "Operator has no device representation\n"); std::abort(); }
        num_type rows = (num_type)mgcr_op_nrow(op);
        MultiField<num_type> out(rows == X.field_size() ? X.get_mesh() : Mesh<num_type>(&rows, 1), X.ncols());
        mgcr_detail::ok(mgcr_op_apply_multi(op, X.device(), out.device()), "Operator apply_multi");
        return out;
    }

protected:
    Field<num_type> apply_handle(const Field<num_type> &f, mgcr_op_t op, num_type out_rows) {
        if (f.field_size() != dim) { std::fprintf(stderr, "Sparse matrix dimension does not match Field dimension!\n"); std::abort(); }
        Field<num_type> out = (out_rows == f.field_size()) ? Field<num_type>(f.get_mesh()) : Field<num_type>(&out_rows, 1);
        mgcr_detail::ok(mgcr_op_apply(op, f.device(), out.device()), "Operator apply");
        out.device_written();
        return out;
    }
    num_type dim = 0;
};

// ------------------------------------------------------------------------------------------------
// Sparse — src/Operator.h:56-101 (CSR, malloc-owned arrays like the reference; the device copy is
// (re)built lazily after the host arrays were modified through mod_*_at)
// ------------------------------------------------------------------------------------------------
template <typename num_type>
class Sparse : public Operator<num_type> {
public:
    Sparse() = default;
    explicit Sparse(num_type rows) { ROW = (num_type *)std::malloc(sizeof(num_type) * (size_t)(rows + 1)); nrow = rows; this->dim = rows; }
    Sparse(num_type rows, num_type cols, num_type nnz) {
        nrow = rows; this->dim = cols;
        ROW = (num_type *)std::malloc(sizeof(num_type) * (size_t)(rows + 1));
        ROW[rows] = nnz;
        COL = (num_type *)std::malloc(sizeof(num_type) * (size_t)nnz);
        VAL = (std::complex<double> *)std::malloc(sizeof(std::complex<double>) * (size_t)nnz);
    }
    Sparse(Sparse const &m) { copy_from(m); }
    // adopts the caller's malloc'd arrays (:64)
    Sparse(num_type rows, num_type cols, num_type *row, num_type *col, std::complex<double> *val) { nrow = rows; this->dim = cols; ROW = row; COL = col; VAL = val; }
    // unordered triplets, duplicates summed (:250-294) — generalised: rows may be empty
    Sparse(num_type rows, num_type cols, std::pair<std::complex<double>, std::pair<num_type, num_type>> *t, num_type len) {
        nrow = rows; this->dim = cols;
        std::sort(t, t + len, [&](auto &a, auto &b) { return a.second.first * cols + a.second.second < b.second.first * cols + b.second.second; });
        ROW = (num_type *)std::calloc((size_t)(rows + 1), sizeof(num_type));
        COL = (num_type *)std::malloc(sizeof(num_type) * (size_t)(len ? len : 1));
        VAL = (std::complex<double> *)std::calloc((size_t)(len ? len : 1), sizeof(std::complex<double>));
        num_type n = 0;
        for (num_type l = 0; l < len; l++) {
            if (n > 0 && l > 0 && t[l].second == t[l - 1].second) { VAL[n - 1] += t[l].first; continue; }
            COL[n] = t[l].second.second; VAL[n] = t[l].first; ROW[t[l].second.first + 1]++; n++;
        }
        for (num_type r = 0; r < rows; r++) ROW[r + 1] += ROW[r];
    }
    ~Sparse() override { drop(); if (ROW) std::free(ROW); if (COL) std::free(COL); if (VAL) std::free(VAL); }

    num_type get_nrow() const { return nrow; }
    num_type get_nnz() const { return ROW[nrow]; }
    std::complex<double> val_at(num_type row, num_type col) const override {
        for (num_type i = ROW[row]; i < ROW[row + 1]; i++) if (COL[i] == col) return VAL[i];
        return 0.;
    }
    std::complex<double> val_at(num_type location) const override { return VAL[location]; }
    num_type get_COL(num_type l) const { return COL[l]; }
    num_type get_ROW(num_type l) const { return ROW[l]; }
    void mod_COL_at(num_type l, num_type v) const { COL[l] = v; dirty = true; }
    void mod_ROW_at(num_type l, num_type v) const { ROW[l] = v; dirty = true; }
    void mod_VAL_at(num_type l, std::complex<double> v) const { VAL[l] = v; dirty = true; }
    Field<num_type> operator()(Field<num_type> const &f) override { return this->apply_handle(f, handle(), nrow); }
    Sparse &operator=(const Sparse &m) noexcept { if (this != &m) { drop(); std::free(ROW); std::free(COL); std::free(VAL); copy_from(m); } return *this; }
    // Set-up-time algebra on the host arrays, like the reference's.  dagger (:296-328): conjugate transpose in place;
    // a new row's entries keep the order of the old rows.  operator*(complex) (:535-544).  operator+ / operator-
    // (:404-534) are NOT provided: their merge loops read COL[] one entry past the end of either matrix while the
    // other still has entries, so what they return depends on memory the matrices do not own.
    void dagger() {
        const num_type nnz = get_nnz(), ncol = this->dim;
        auto *NR = (num_type *)std::calloc((size_t)(ncol + 1), sizeof(num_type));
        auto *NC = (num_type *)std::malloc(sizeof(num_type) * (size_t)(nnz ? nnz : 1));
        auto *NV = (std::complex<double> *)std::malloc(sizeof(std::complex<double>) * (size_t)(nnz ? nnz : 1));
        for (num_type l = 0; l < nnz; l++) NR[COL[l] + 1]++;
        for (num_type c = 0; c < ncol; c++) NR[c + 1] += NR[c];
        std::vector<num_type> fill(NR, NR + ncol);
        for (num_type r = 0; r < nrow; r++)
            for (num_type l = ROW[r]; l < ROW[r + 1]; l++) {
                const num_type at = fill[(size_t)COL[l]]++;
                NC[at] = r;
                NV[at] = std::conj(VAL[l]);
            }
        std::free(ROW); std::free(COL); std::free(VAL);
        ROW = NR; COL = NC; VAL = NV;
        this->dim = nrow; nrow = ncol;
        dirty = true;
    }
    Sparse operator*(std::complex<double> a) const {
        Sparse out(*this);
        for (num_type i = 0; i < get_nnz(); i++) out.VAL[i] = VAL[i] * a;
        return out;
    }
    mgcr_op_t handle() override {
        if (!op || dirty) {
            mgcr_detail::ensure_init();
            std::vector<int64_t> rp((size_t)nrow + 1), ci((size_t)ROW[nrow]);
            for (num_type i = 0; i <= nrow; i++) rp[(size_t)i] = (int64_t)ROW[i];
            for (num_type i = 0; i < ROW[nrow]; i++) ci[(size_t)i] = (int64_t)COL[i];
            // a matrix that changed (dagger, mod_*_at) is replaced BEHIND its handle: DiracOp / GCR objects that borrowed
            // the handle — as the reference's keep a Sparse* — go on with the new matrix, and the handle never dangles
            if (op) mgcr_detail::ok(mgcr_csr_replace(op, (int64_t)nrow, (int64_t)this->dim, rp.data(), ci.data(), reinterpret_cast<const double *>(VAL)), "Sparse re-upload");
            else mgcr_detail::ok(mgcr_csr_create((int64_t)nrow, (int64_t)this->dim, rp.data(), ci.data(), reinterpret_cast<const double *>(VAL), &op), "Sparse upload");
            dirty = false;
        }
        return op;
    }

protected:
    std::complex<double> *VAL = nullptr;
    num_type *COL = nullptr, *ROW = nullptr;
    num_type nrow = 0;

private:
    void drop() const { if (op) { mgcr_op_destroy(op); op = nullptr; } }
    void copy_from(const Sparse &m) {
        nrow = m.nrow; this->dim = m.dim;
        num_type nnz = m.get_nnz();
        ROW = (num_type *)std::malloc(sizeof(num_type) * (size_t)(nrow + 1));
        COL = (num_type *)std::malloc(sizeof(num_type) * (size_t)nnz);
        VAL = (std::complex<double> *)std::malloc(sizeof(std::complex<double>) * (size_t)nnz);
        std::memcpy(ROW, m.ROW, sizeof(num_type) * (size_t)(nrow + 1));
        std::memcpy(COL, m.COL, sizeof(num_type) * (size_t)nnz);
        std::memcpy(VAL, m.VAL, sizeof(std::complex<double>) * (size_t)nnz);
        dirty = true;
    }
    mutable mgcr_op_t op = nullptr;
    mutable bool dirty = true;
};

// DiracOp = Id - k*D — src/Operator.h:104-122,555-575 (borrows the Sparse)
template <typename num_type>
class DiracOp : public Operator<num_type> {
public:
    DiracOp(Sparse<num_type> *mat, std::complex<double> k_factor) : k(k_factor), D(mat) { this->dim = D->get_dim(); }
    DiracOp(DiracOp const &o) : k(o.k), D(o.D) { this->dim = D->get_dim(); }
    ~DiracOp() override { if (op) mgcr_op_destroy(op); }
    std::complex<double> val_at(num_type row, num_type col) const override { return 1. - k * D->val_at(row, col); }
    std::complex<double> val_at(num_type location) const override { return 1. - k * D->val_at(location); }
    Field<num_type> operator()(Field<num_type> const &f) override { return this->apply_handle(f, handle(), this->dim); }
    void set_k(std::complex<double> new_k) { k = new_k; if (op) { double v[2] = {k.real(), k.imag()}; mgcr_detail::ok(mgcr_dirac_set_k(op, v), "set_k"); } }
    mgcr_op_t handle() override {
        mgcr_op_t base = D->handle();
        if (!op || base != base_seen) {
            if (op) mgcr_op_destroy(op);
            double v[2] = {k.real(), k.imag()};
            mgcr_detail::ok(mgcr_dirac_create(base, v, &op), "DiracOp");
            base_seen = base;
        }
        return op;
    }

private:
    std::complex<double> k = 0.;
    Sparse<num_type> *D;
    mgcr_op_t op = nullptr, base_seen = nullptr;
};

// MultiDiracOp: Id - ks[j]*D on column j of a block of ks.size() Fields — a hopping-parameter scan (the ladder of
// test_kcritical, src/main.cpp:696-741) as ONE operator (extension, mgcr_dirac_multi_create).  Borrows the Sparse.  Only
// apply_multi and GCR::solve_multi take it; column j has the bits of DiracOp(D, ks[j]) on that column alone.
template <typename num_type>
class MultiDiracOp : public Operator<num_type> {
public:
    MultiDiracOp(Sparse<num_type> *mat, std::vector<std::complex<double>> k_factors) : ks(std::move(k_factors)), D(mat) { this->dim = D->get_dim(); }
    MultiDiracOp(MultiDiracOp const &o) : ks(o.ks), D(o.D) { this->dim = D->get_dim(); }
    ~MultiDiracOp() override { if (op) mgcr_op_destroy(op); }
    int ncols() const { return (int)ks.size(); }
    std::complex<double> val_at(num_type, num_type) const override { return no_single("val_at"); }
    std::complex<double> val_at(num_type) const override { return no_single("val_at"); }
    Field<num_type> operator()(Field<num_type> const &f) override { no_single("operator()"); return f; }
    void set_k(std::vector<std::complex<double>> new_ks) {   // same count; holds for every later apply / solve
        if (new_ks.size() != ks.size()) { std::fprintf(stderr, "MultiDiracOp::set_k: %zu values for %zu columns\n", new_ks.size(), ks.size()); std::abort(); }
        ks = std::move(new_ks);
        if (op) mgcr_detail::ok(mgcr_dirac_multi_set_k(op, reinterpret_cast<const double *>(ks.data())), "MultiDiracOp::set_k");
    }
    mgcr_op_t handle() override {
        mgcr_op_t base = D->handle();
        if (!op || base != base_seen) {
            if (op) mgcr_op_destroy(op);
            mgcr_detail::ok(mgcr_dirac_multi_create(base, (int32_t)ks.size(), reinterpret_cast<const double *>(ks.data()), &op), "MultiDiracOp");
            base_seen = base;
        }
        return op;
    }

private:
    static std::complex<double> no_single(const char *what) {
        std::fprintf(stderr, "MultiDiracOp::%s: one hopping parameter per column of a block; use apply_multi / GCR::solve_multi\n", what);
        std::abort();
    }
    std::vector<std::complex<double>> ks;
    Sparse<num_type> *D;
    mgcr_op_t op = nullptr, base_seen = nullptr;
};

// Dense — src/Operator.h:32-54 (row-major dim x dim; the block kernel of HierarchicalSparse)
template <typename num_type>
class Dense : public Operator<num_type> {
public:
    Dense() = default;
    Dense(Dense const &d) : mat(d.mat) { this->dim = d.dim; }
    Dense(std::complex<double> *matrix, num_type const dimension) : mat(matrix, matrix + dimension * dimension) { this->dim = dimension; }
    ~Dense() override { if (op) mgcr_op_destroy(op); }
    std::complex<double> val_at(num_type location) const override { return mat[(size_t)location]; }
    std::complex<double> val_at(num_type row, num_type col) const override { return mat[(size_t)(row * this->dim + col)]; }
    // Set-up-time algebra (:139-190).  operator+ adds all d*d entries; the reference hands `d` to vec_add (:144), so
    // only the first row of ITS sum is computed and the rest is uninitialised memory.  operator* sums over k in index
    // order (mat_mult, src/utils.cpp:70-81); dagger = conjugate transpose (mat_dagger :84-90).
    Dense operator+(const Dense &B) const {
        Dense out(*this);
        for (size_t e = 0; e < mat.size(); e++) out.mat[e] = mat[e] + B.mat[e];
        return out;
    }
    Dense operator*(const Dense &B) const {
        const size_t d = (size_t)this->dim;
        Dense out(*this);
        for (size_t i = 0; i < d; i++)
            for (size_t j = 0; j < d; j++) {
                std::complex<double> sum(0., 0.);
                for (size_t k = 0; k < d; k++) sum += mat[i * d + k] * B.mat[k * d + j];
                out.mat[i * d + j] = sum;
            }
        return out;
    }
    Dense dagger() const {
        const size_t d = (size_t)this->dim;
        Dense out(*this);
        for (size_t i = 0; i < d; i++)
            for (size_t j = 0; j < d; j++) out.mat[j * d + i] = std::conj(mat[i * d + j]);
        return out;
    }
    Field<num_type> operator()(const Field<num_type> &f) override {
        if (!op) {
            mgcr_detail::ensure_init();
            int32_t bp[2] = {0, 1}, bc[1] = {0};
            mgcr_detail::ok(mgcr_bcsr_create(1, 1, (int32_t)this->dim, bp, bc, reinterpret_cast<const double *>(mat.data()), &op), "Dense upload");
        }
        return this->apply_handle(f, op, this->dim);
    }

private:
    std::vector<std::complex<double>> mat;
    mgcr_op_t op = nullptr;
};

// HierarchicalSparse — src/HierarchicalSparse.h:22-48: block-CSR of Operator<coarse_num_type>
// blocks from unordered triplets; duplicates of a (row,col) pair are kept and summed at apply time.
// Takes ownership of the block operators and deletes them, like the reference (:191-199).
template <typename num_type, typename coarse_num_type>
class HierarchicalSparse : public Operator<num_type> {
public:
    HierarchicalSparse(coarse_num_type block_rows, coarse_num_type block_cols,
                       std::pair<Operator<coarse_num_type> *, std::pair<coarse_num_type, coarse_num_type>> *triplets,
                       coarse_num_type triplet_length) {
        mgcr_detail::ensure_init();
        sub = (int32_t)triplets[0].first->get_dim();
        nbrow = (int32_t)block_rows;
        this->dim = (num_type)block_cols * sub;
        std::vector<int32_t> rows((size_t)triplet_length), cols((size_t)triplet_length);
        std::vector<std::complex<double>> blocks((size_t)triplet_length * sub * sub);
        for (coarse_num_type t = 0; t < triplet_length; t++) {
            rows[(size_t)t] = (int32_t)triplets[t].second.first;
            cols[(size_t)t] = (int32_t)triplets[t].second.second;
            for (int32_t e = 0; e < sub * sub; e++) blocks[(size_t)t * sub * sub + e] = triplets[t].first->val_at((coarse_num_type)e);
            owned.push_back(triplets[t].first);
        }
        nblocks = (int64_t)triplet_length;
        mgcr_detail::ok(mgcr_bcsr_create_from_triplets(nbrow, (int32_t)block_cols, sub, (int32_t)triplet_length, rows.data(), cols.data(),
                                                       reinterpret_cast<const double *>(blocks.data()), &op), "HierarchicalSparse");
        // dense shadow for val_at (:164-188): sums duplicates
        shadow_rows = rows; shadow_cols = cols; shadow = blocks;
    }
    ~HierarchicalSparse() override { for (auto *o : owned) delete o; if (op) mgcr_op_destroy(op); }
    num_type get_nrow() const { return (num_type)nbrow * sub; }
    num_type get_nnz() const { return (num_type)nblocks * sub * sub; }
    std::complex<double> val_at(num_type row, num_type col) const override {
        int32_t br = (int32_t)(row / sub), bc = (int32_t)(col / sub), ro = (int32_t)(row % sub), co = (int32_t)(col % sub);
        std::complex<double> o(0, 0);
        for (size_t t = 0; t < shadow_rows.size(); t++)
            if (shadow_rows[t] == br && shadow_cols[t] == bc) o += shadow[t * sub * sub + (size_t)ro * sub + co];
        return o;
    }
    std::complex<double> val_at(num_type location) const override { return shadow[(size_t)location]; }
    Field<num_type> operator()(Field<num_type> const &f) override { return this->apply_handle(f, op, get_nrow()); }
    mgcr_op_t handle() override { return op; }

private:
    int32_t sub = 0, nbrow = 0;
    int64_t nblocks = 0;
    mgcr_op_t op = nullptr;
    std::vector<Operator<coarse_num_type> *> owned;
    std::vector<int32_t> shadow_rows, shadow_cols;
    std::vector<std::complex<double>> shadow;
};

// ------------------------------------------------------------------------------------------------
// Parameters — src/SolverParam.h
// ------------------------------------------------------------------------------------------------
template <typename num_type>
class SolverParam {
public:
    Operator<num_type> *left_precond = nullptr;
    Operator<num_type> *right_precond = nullptr;
};

template <typename num_type>
class GCR_Param : public SolverParam<num_type> {
public:
    GCR_Param() = default;
    int truncation = 0;
    int restart = 0;
    int max_iter = 100;
    double tol = 1e-16;
    bool verbose = true;
    GCR_Param(int trunc, int re, int max_it, double tau, bool verb, Operator<num_type> *solver_l, Operator<num_type> *solver_r)
        : truncation(trunc), restart(re), max_iter(max_it), tol(tau), verbose(verb) { this->left_precond = solver_l; this->right_precond = solver_r; }
    // extensions (0 = the reference's behaviour), see include/mgcr.h
    bool use_x0 = false, flexible = false;
};

template <typename num_type>
class MG_Param : public SolverParam<num_type> {
public:
    Mesh<num_type> mesh;
    num_type subblock_dim = 0;
    int n_eigen = 0;
    GCR_Param<num_type> *eigenvector_precomp_param = nullptr;
    Operator<num_type> *coarse_solver = nullptr;
    Operator<num_type> *smoother_solver = nullptr;
    bool spacetime[6] = {true, true, true, true, false, false};
    bool spinor[6] = {false, false, false, false, true, false};
    int n_level = 1;
    double damping = 1.0;  // the reference hard-codes 0.1 (src/MG.h:426)
    int coarse_direct_rows = 0;  // extension: > 0 = a coarsest level of at most this many unknowns (<= 2048) is solved directly
    // extension: use these near-null vectors instead of computing n_eigen of them by inverse iteration
    // (e.g. the constant vector: piecewise-constant aggregation for Poisson-like operators)
    const std::vector<Field<num_type>> *null_vectors = nullptr;
    MG_Param() = default;
    MG_Param(Mesh<num_type> m, num_type subblock, int eigenvecs, GCR_Param<num_type> *eigen_param, Operator<num_type> *solver_coarse,
             Operator<num_type> *solver_smooth, int levels, Operator<num_type> *solver_l, Operator<num_type> *solver_r)
        : mesh(std::move(m)), subblock_dim(subblock), n_eigen(eigenvecs), eigenvector_precomp_param(eigen_param),
          coarse_solver(solver_coarse), smoother_solver(solver_smooth), n_level(levels) { this->left_precond = solver_l; this->right_precond = solver_r; }
};

// ------------------------------------------------------------------------------------------------
// GCR — src/GCR.h:18-50
// ------------------------------------------------------------------------------------------------
template <typename num_type>
class GCR : public Operator<num_type> {
public:
    GCR() = default;
    GCR(GCR const &g) : A_operator(g.A_operator), param(g.param) { if (A_operator) this->dim = A_operator->get_dim(); }
    explicit GCR(Operator<num_type> *M, GCR_Param<num_type> *gcr_param) : A_operator(M), param(gcr_param) { this->dim = M->get_dim(); }
    GCR(GCR_Param<num_type> *gcr_param) : param(gcr_param) {}
    // the legacy dense form (src/GCR.h:27,70-75): a row-major dimension x dimension matrix, copied
    GCR(const std::complex<double> *matrix, const num_type dimension) : dense(matrix, matrix + dimension * dimension) { this->dim = dimension; }
    ~GCR() override { if (op) mgcr_op_destroy(op); if (dense_op) mgcr_op_destroy(dense_op); }

    // Legacy raw-pointer solve (src/GCR.h:78-156): r0 = rhs - A x (x0 honoured), directions truncated to the last
    // `truncation`, stops when |r|^2 <= tol — absolute, and tested BEFORE every step, so possibly after none — or after
    // max_iter steps; prints the reference's lines.  On the device: the Dense operator, GCR in truncation mode with use_x0;
    // the relative stopping rule of the Field solve is set to sqrt(tol) / |rhs|, which is the same test.
    void solve(const std::complex<double> *rhs, std::complex<double> *x, const double tol, const int max_iter, const int truncation) {
        if (dense.empty()) { std::fprintf(stderr, "GCR::solve(raw pointers) needs the GCR(matrix, dimension) constructor\n"); std::abort(); }
        mgcr_detail::ensure_init();
        const num_type d = this->dim;
        if (!dense_op) {
            int32_t bp[2] = {0, 1}, bc[1] = {0};
            mgcr_detail::ok(mgcr_bcsr_create(1, 1, (int32_t)d, bp, bc, reinterpret_cast<const double *>(dense.data()), &dense_op), "GCR dense matrix");
        }
        num_type dims1[1] = {d};
        Field<num_type> b(dims1, 1), xf(dims1, 1), r(dims1, 1);
        for (num_type i = 0; i < d; i++) { b.mod_val_at(i, rhs[i]); xf.mod_val_at(i, x[i]); }
        // the test that precedes the first step: |rhs - A x0|^2 > tol ?
        mgcr_detail::ok(mgcr_op_apply(dense_op, xf.device(), r.device()), "GCR dense residual");
        r.device_written();
        Field<num_type> r0 = b - r;
        const double bn2 = b.squarednorm();
        int it = 0;
        double rr = r0.squarednorm();
        if (rr > tol && max_iter > 0 && bn2 > 0.) {
            mgcr_gcr_param p;
            std::memset(&p, 0, sizeof(p));
            p.truncation = truncation; p.restart = 0; p.max_iter = max_iter; p.tol = std::sqrt(tol) / std::sqrt(bn2); p.use_x0 = 1;
            std::vector<double> hist((size_t)max_iter + 1, 0.);
            int32_t n = 0, conv = 0;
            mgcr_detail::ok(mgcr_gcr_solve(dense_op, &p, b.device(), xf.device(), hist.data(), max_iter + 1, &n, &conv), "GCR dense solve");
            xf.device_written();
            it = n;
            const double bn = std::sqrt(bn2);
            for (int k = 1; k <= it; k++) std::printf("Step %d residual norm = %.10e\n", k, hist[(size_t)k] * bn);
            rr = (hist[(size_t)it] * bn) * (hist[(size_t)it] * bn);
            for (num_type i = 0; i < d; i++) x[i] = xf.val_at(i);
        } else if (rr > tol && max_iter > 0) {
            // rhs = 0 with x0 != 0: the reference iterates on r0 = -A x0 and drives x towards 0 (its test is absolute).  The
            // Field solve's test is relative to its right-hand side: hand it r0 AS the right-hand side (r = rhs there whatever
            // x is, src/GCR.h:189) and let it update x0 in place — the same recurrence, tolerance sqrt(tol) / |r0|
            mgcr_gcr_param p;
            std::memset(&p, 0, sizeof(p));
            const double rn = std::sqrt(rr);
            p.truncation = truncation; p.restart = 0; p.max_iter = max_iter; p.tol = std::sqrt(tol) / rn;
            std::vector<double> hist((size_t)max_iter + 1, 0.);
            int32_t n = 0, conv = 0;
            mgcr_detail::ok(mgcr_gcr_solve(dense_op, &p, r0.device(), xf.device(), hist.data(), max_iter + 1, &n, &conv), "GCR dense solve");
            xf.device_written();
            it = n;
            for (int k = 1; k <= it; k++) std::printf("Step %d residual norm = %.10e\n", k, hist[(size_t)k] * rn);
            rr = (hist[(size_t)it] * rn) * (hist[(size_t)it] * rn);
            for (num_type i = 0; i < d; i++) x[i] = xf.val_at(i);
        }
        if (it == max_iter) std::printf("GCR did not converge after %d steps! Residual norm = %.10e\n", max_iter, rr);
        iterations = it;
    }
    void initialise(Operator<num_type> *M) override { A_operator = M; this->dim = M->get_dim(); if (op) mgcr_detail::ok(mgcr_gcr_set_operator(op, M->handle()), "GCR::initialise"); }
    GCR_Param<num_type> *get_param() const { return param; }

    void solve(const Field<num_type> &rhs, Field<num_type> &x) {  // :158-302
        if (rhs.field_size() != this->dim) { std::fprintf(stderr, "Field dimension does not match with Operator!\n"); std::abort(); }
        if (x.field_size() != this->dim) { std::fprintf(stderr, "x dimension does not match with Operator!\n"); std::abort(); }
        if (param->truncation == 0 && param->restart == 0 && param->verbose) std::printf("WARNING: Full GCR solve could incur high memory usage!\n");
        mgcr_gcr_param p = cparam();  // GCR_Param is read at solve time, the work vectors live in the handle
        int cap = (param->max_iter > 0 ? param->max_iter : 1) + 1;
        history.assign((size_t)cap, 0.);
        int32_t it = 0, conv = 0;
        mgcr_op_t self = handle();
        mgcr_detail::ok(mgcr_gcr_set_operator(self, need_handle(A_operator)), "GCR::solve");
        mgcr_detail::ok(mgcr_gcr_set_param(self, &p), "GCR::solve");
        mgcr_detail::ok(mgcr_gcr_solve_op(self, rhs.device(), x.device(), history.data(), cap, &it, &conv), "GCR::solve");
        x.device_written();
        history.resize((size_t)it + 1);
        iterations = it; converged = conv != 0;
        std::ofstream file("../../data/out_data/convergence.txt");  // :168 (silently a no-op when the directory is absent)
        for (int i = 0; i <= it; i++) file << i << "\t" << history[(size_t)i] << "\n";
    }
    // k independent solves A x_j = rhs_j in lockstep (extension, mgcr_gcr_solve_multi: restart mode; the operator a matrix, a
    // DiracOp or a MultiDiracOp).  Unpreconditioned, or — the flexible batched GCR — with GCR_Param::right_precond = M and
    // flexible = true: M a LowPrecisionGCR of the square form, which runs as the k-wide lockstep inner solve, or a Sparse, DiracOp
    // or HierarchicalSparse, applied k-wide to the residual block (Rule F of mgcr.h; M must outlive the solve, as in solve()).
    // X is updated in place; per column: last_history[j][i] = the value
    // solve() would print at step i, last_iterations[j], last_converged[j] — the bits of solve() on that column alone.
    void solve_multi(const MultiField<num_type> &rhs, MultiField<num_type> &x) {
        if (!A_operator) { std::fprintf(stderr, "GCR has no operator (call initialise first)\n"); std::abort(); }
        if (rhs.field_size() != this->dim) { std::fprintf(stderr, "Field dimension does not match with Operator!\n"); std::abort(); }
        if (x.field_size() != this->dim) { std::fprintf(stderr, "x dimension does not match with Operator!\n"); std::abort(); }
        mgcr_gcr_param p = cparam();
        const int k = rhs.ncols(), cap = (param->max_iter > 0 ? param->max_iter : 1) + 1;
        std::vector<double> hist((size_t)k * cap, 0.);
        std::vector<int32_t> it((size_t)k, 0), conv((size_t)k, 0);
        mgcr_detail::ok(mgcr_gcr_solve_multi(need_handle(A_operator), &p, rhs.device(), x.device(), hist.data(), cap, it.data(), conv.data()),
                        "GCR::solve_multi");
        last_history.assign((size_t)k, std::vector<double>());
        last_iterations.assign(it.begin(), it.end());
        last_converged.assign((size_t)k, false);
        for (int j = 0; j < k; j++) {
            last_history[(size_t)j].assign(hist.begin() + (size_t)j * cap, hist.begin() + (size_t)j * cap + it[(size_t)j] + 1);
            last_converged[(size_t)j] = conv[(size_t)j] != 0;
        }
    }
    // Any number of systems through `width` <= 16 columns of one batched solve (extension, mgcr_gcr_solve_queue): a column whose
    // system has stopped takes the next waiting one at the next boundary of the restart cycle.  System s: A x_s = rhs_s, or — ks
    // given, A the Sparse D — (1 - ks[s] D) x_s = rhs_s.  rhs may repeat, the x Fields are distinct and updated in place; per
    // SYSTEM: last_history[s], last_iterations[s], last_converged[s] — the bits of solve() on that system alone.
    void solve_queue(const std::vector<const Field<num_type> *> &rhs, const std::vector<Field<num_type> *> &x, int width,
                     const std::vector<std::complex<double>> *ks = nullptr) {
        if (!A_operator) { std::fprintf(stderr, "GCR has no operator (call initialise first)\n"); std::abort(); }
        if (rhs.size() != x.size() || (ks && ks->size() != rhs.size())) { std::fprintf(stderr, "GCR::solve_queue: one x (and one k) per right-hand side\n"); std::abort(); }
        mgcr_gcr_param p = cparam();
        const int nsys = (int)rhs.size(), cap = (param->max_iter > 0 ? param->max_iter : 1) + 1;
        std::vector<mgcr_vec_t> bh, xh;
        for (int s = 0; s < nsys; s++) { bh.push_back(rhs[(size_t)s]->device()); xh.push_back(x[(size_t)s]->device()); }
        std::vector<double> kri, hist((size_t)nsys * cap, 0.);
        if (ks) for (const std::complex<double> &k : *ks) { kri.push_back(k.real()); kri.push_back(k.imag()); }
        std::vector<int32_t> it((size_t)nsys, 0), conv((size_t)nsys, 0);
        mgcr_detail::ok(mgcr_gcr_solve_queue(need_handle(A_operator), &p, width, nsys, bh.data(), xh.data(), ks ? kri.data() : nullptr, hist.data(), cap,
                                             it.data(), conv.data()),
                        "GCR::solve_queue");
        last_history.assign((size_t)nsys, std::vector<double>());
        last_iterations.assign(it.begin(), it.end());
        last_converged.assign((size_t)nsys, false);
        for (int s = 0; s < nsys; s++) {
            x[(size_t)s]->device_written();
            last_history[(size_t)s].assign(hist.begin() + (size_t)s * cap, hist.begin() + (size_t)s * cap + it[(size_t)s] + 1);
            last_converged[(size_t)s] = conv[(size_t)s] != 0;
        }
    }
    std::vector<std::vector<double>> last_history;
    std::vector<int> last_iterations;
    std::vector<bool> last_converged;

    std::complex<double> val_at(num_type row, num_type col) const override { return A_operator->val_at(row, col); }
    std::complex<double> val_at(num_type location) const override { return A_operator->val_at(location); }
    Field<num_type> operator()(Field<num_type> const &f) override {  // :62-68: x = init_rand(2); solve(f, x)
        Field<num_type> x(f.get_mesh());
        x.init_rand(2);
        solve(f, x);
        return x;
    }
    // GCR as a device operator (smoother / coarse solver / preconditioner): x0 = 0, no host round trips
    mgcr_op_t handle() override {
        if (!op) {
            mgcr_detail::ensure_init();
            mgcr_gcr_param p = cparam();
            mgcr_detail::ok(mgcr_gcr_create(A_operator ? need_handle(A_operator) : nullptr, &p, 1, &op), "GCR handle");
        }
        return op;
    }
    std::vector<double> history;  // hist[k] = value printed at step k
    int iterations = 0;
    bool converged = false;

private:
    static mgcr_op_t need_handle(Operator<num_type> *o) {
        mgcr_op_t h = o->handle();
        if (!h) { std::fprintf(stderr, "Operator has no device representation (only Sparse, DiracOp, HierarchicalSparse, GCR and MG can run on the GPU)\n"); std::abort(); }
        return h;
    }
    mgcr_gcr_param cparam() const {
        mgcr_gcr_param p;
        std::memset(&p, 0, sizeof(p));
        if (param->truncation != 0 && param->restart != 0) { std::fprintf(stderr, "Do not support concurrent restarting and truncation.\n"); std::abort(); }
        p.truncation = param->truncation; p.restart = param->restart; p.max_iter = param->max_iter; p.tol = param->tol;
        p.verbose = param->verbose ? 1 : 0;
        p.left_precond = param->left_precond ? need_handle(param->left_precond) : nullptr;
        p.right_precond = param->right_precond ? need_handle(param->right_precond) : nullptr;
        p.use_x0 = param->use_x0; p.flexible = param->flexible;
        return p;
    }
    Operator<num_type> *A_operator = nullptr;
    GCR_Param<num_type> *param = nullptr;
    mgcr_op_t op = nullptr;
    std::vector<std::complex<double>> dense;   // legacy GCR(matrix, dimension)
    mgcr_op_t dense_op = nullptr;
};

// LowPrecisionGCR: mixed precision (extension, mgcr_gcr32_create) — an fp32 copy of a Sparse (its arrays are copied, so later changes of
// the Sparse are not seen) and a restarted GCR that runs in fp32 on the device, from x0 = 0, without host round trips.  With k:
// A = Id - k*D (Dirac form); without: A = the matrix.  inner: restart (1 .. 16), max_iter (steps enqueued per apply), tol (relative).
// operator()(f) returns y ~ A^-1 f.  Its place is GCR_Param::right_precond of an fp64 solve with flexible = true: the inner solve
// stops on a tolerance, so it is not a linear map, and every other slot refuses it.
template <typename num_type>
class LowPrecisionGCR : public Operator<num_type> {
public:
    LowPrecisionGCR(Sparse<num_type> *mat, std::complex<double> k_factor, const GCR_Param<num_type> *inner) : k(k_factor) { create(mat, true, inner); }
    LowPrecisionGCR(Sparse<num_type> *mat, const GCR_Param<num_type> *inner) { create(mat, false, inner); }
    LowPrecisionGCR(LowPrecisionGCR const &) = delete;
    LowPrecisionGCR &operator=(LowPrecisionGCR const &) = delete;
    ~LowPrecisionGCR() override { if (op) mgcr_op_destroy(op); }
    std::complex<double> val_at(num_type, num_type) const override { return not_stored(); }
    std::complex<double> val_at(num_type) const override { return not_stored(); }
    Field<num_type> operator()(Field<num_type> const &f) override { return this->apply_handle(f, op, this->dim); }
    mgcr_op_t handle() override { return op; }
    void set_k(std::complex<double> new_k) { double v[2] = {new_k.real(), new_k.imag()}; mgcr_detail::ok(mgcr_gcr32_set_k(op, v), "LowPrecisionGCR::set_k"); k = new_k; }
    void set_param(const GCR_Param<num_type> *inner) { mgcr_gcr_param p = cparam(inner); mgcr_detail::ok(mgcr_gcr32_set_param(op, &p), "LowPrecisionGCR::set_param"); }
    // y = fp64(A32 fp32(x)): one matrix apply in fp32
    void apply_matrix(const Field<num_type> &x, Field<num_type> &y) {
        mgcr_detail::ok(mgcr_gcr32_apply_matrix(op, x.device(), y.device()), "LowPrecisionGCR::apply_matrix");
        y.device_written();
    }
    // steps the last apply performed and its last fp32 |r| / |f| (one synchronisation)
    int last(double *rel_res = nullptr) {
        int32_t it = 0;
        double rel = 0.;
        mgcr_detail::ok(mgcr_gcr32_last(op, &it, &rel), "LowPrecisionGCR::last");
        if (rel_res) *rel_res = rel;
        return (int)it;
    }
    struct Info { int64_t n; int32_t ell_width; int64_t tail_rows; bool real_slab; int64_t stored_bytes; };
    Info info() {
        Info i{};
        int32_t real = 0;
        mgcr_detail::ok(mgcr_gcr32_info(op, &i.n, &i.ell_width, &i.tail_rows, &real, &i.stored_bytes), "LowPrecisionGCR::info");
        i.real_slab = real != 0;
        return i;
    }
    // Blocks of k Fields (extension, mgcr_gcr32_apply_multi): Y_j ~ A^-1 F_j, the k fp32 inner solves advancing in lockstep — column
    // j has the bits of operator()(F.column(j)).  active: bit j set, column j takes part; clear, it performs 0 steps and y_j = 0.
    void inner_multi(const MultiField<num_type> &F, MultiField<num_type> &Y, uint32_t active) {
        mgcr_detail::ok(mgcr_gcr32_apply_multi(op, F.device(), Y.device(), active), "LowPrecisionGCR::inner_multi");
        last_k = F.ncols();
    }
    void inner_multi(const MultiField<num_type> &F, MultiField<num_type> &Y) { inner_multi(F, Y, (uint32_t)((1u << F.ncols()) - 1u)); }
    // steps and last fp32 |r| / |f| per column of the last batched inner solve (one synchronisation)
    std::vector<int> last_multi(std::vector<double> *rel_res = nullptr) {
        int32_t it[16] = {};
        double rel[16] = {};
        mgcr_detail::ok(mgcr_gcr32_last_multi(op, it, rel), "LowPrecisionGCR::last_multi");
        if (rel_res) rel_res->assign(rel, rel + last_k);
        return std::vector<int>(it, it + last_k);
    }
    // The batched mixed solve A X = B (extension, mgcr_gcr32_solve_multi): fp64 defect correction, R = B - A X, X += inner_multi(R) on
    // the columns that have not converged; column j has the bits of the same loop on column j alone.  Per column: last_history[j]
    // (|r| / |b| per outer step), last_iterations[j], last_converged[j].
    void solve_multi(Operator<num_type> &A, const MultiField<num_type> &B, MultiField<num_type> &X, double tol = 1e-10, int max_outer = 50,
                     bool use_x0 = false) {
        const int k = B.ncols(), cap = (max_outer >= 0 ? max_outer : 0) + 1;
        std::vector<double> hist((size_t)k * cap, 0.);
        std::vector<int32_t> it((size_t)k, 0), conv((size_t)k, 0);
        mgcr_detail::ok(mgcr_gcr32_solve_multi(A.handle(), op, tol, max_outer, use_x0 ? 1 : 0, B.device(), X.device(), hist.data(), cap, it.data(), conv.data()),
                        "LowPrecisionGCR::solve_multi");
        for (int32_t v : it)
            if (v > 0) last_k = k;   // (a solve in which no column was ever active enqueues no batched apply)
        last_history.assign((size_t)k, std::vector<double>());
        last_iterations.assign(it.begin(), it.end());
        last_converged.assign((size_t)k, false);
        for (int j = 0; j < k; j++) {
            last_history[(size_t)j].assign(hist.begin() + (size_t)j * cap, hist.begin() + (size_t)j * cap + it[(size_t)j] + 1);
            last_converged[(size_t)j] = conv[(size_t)j] != 0;
        }
    }
    std::vector<std::vector<double>> last_history;   // of solve_multi, column j relative to |b_j|
    std::vector<int> last_iterations;
    std::vector<bool> last_converged;

private:
    int last_k = 0;
    static std::complex<double> not_stored() { std::fprintf(stderr, "LowPrecisionGCR stores an fp32 copy on the device only\n"); std::abort(); }

protected:
    static mgcr_gcr_param cparam(const GCR_Param<num_type> *inner) {
        mgcr_gcr_param p;
        std::memset(&p, 0, sizeof(p));
        p.truncation = inner->truncation; p.restart = inner->restart; p.max_iter = inner->max_iter; p.tol = inner->tol;
        p.left_precond = inner->left_precond ? inner->left_precond->handle() : nullptr;
        p.right_precond = inner->right_precond ? inner->right_precond->handle() : nullptr;
        p.use_x0 = inner->use_x0; p.flexible = inner->flexible;
        return p;
    }

private:
    void create(Sparse<num_type> *mat, bool dirac, const GCR_Param<num_type> *inner) {
        mgcr_detail::ensure_init();
        const num_type rows = mat->get_nrow(), nnz = mat->get_nnz();
        std::vector<int64_t> rp((size_t)rows + 1), ci((size_t)nnz);
        std::vector<std::complex<double>> va((size_t)nnz);
        for (num_type i = 0; i <= rows; i++) rp[(size_t)i] = (int64_t)mat->get_ROW(i);
        for (num_type i = 0; i < nnz; i++) { ci[(size_t)i] = (int64_t)mat->get_COL(i); va[(size_t)i] = mat->val_at(i); }
        double v[2] = {k.real(), k.imag()};
        mgcr_gcr_param p = cparam(inner);
        mgcr_detail::ok(mgcr_gcr32_create((int64_t)rows, rp.data(), ci.data(), reinterpret_cast<const double *>(va.data()), dirac ? v : nullptr, &p, &op),
                        "LowPrecisionGCR");
        this->dim = rows;
    }

protected:
    LowPrecisionGCR() {}
    // the Sparse's host arrays as the C interface takes them
    static void host_csr(Sparse<num_type> *mat, std::vector<int64_t> &rp, std::vector<int64_t> &ci, std::vector<std::complex<double>> &va) {
        const num_type rows = mat->get_nrow(), nnz = mat->get_nnz();
        rp.resize((size_t)rows + 1); ci.resize((size_t)nnz); va.resize((size_t)nnz);
        for (num_type i = 0; i <= rows; i++) rp[(size_t)i] = (int64_t)mat->get_ROW(i);
        for (num_type i = 0; i < nnz; i++) { ci[(size_t)i] = (int64_t)mat->get_COL(i); va[(size_t)i] = mat->val_at(i); }
    }
    std::complex<double> k{0., 0.};
    mgcr_op_t op = nullptr;
};

// LowPrecisionEvenOddGCR: mixed precision on the even-odd Schur system (extension, mgcr_gcr32_create_eo) — an fp32 copy of
// S = diag(a_e) - c^2 H_eo diag(1/a_o) H_oe of a Sparse that may store a site diagonal, and LowPrecisionGCR's inner solve on its n_even
// rows.  With k: Dirac form (the operator of EvenOddDiracOp / EvenOddDiagDiracOp); without: matrix form (EvenOddSparse).  Its place
// is GCR_Param::right_precond, flexible = true, of EvenOddDiracOp::solve or of a GCR on such an operator made from the same matrix
// and parity.  set_k, set_param, apply_matrix (Fields of n_even entries) and last are inherited; info() of the base class is
// refused by the library: ask eo_info().
template <typename num_type>
class LowPrecisionEvenOddGCR : public LowPrecisionGCR<num_type> {
public:
    LowPrecisionEvenOddGCR(Sparse<num_type> *mat, std::complex<double> k_factor, const GCR_Param<num_type> *inner, const std::vector<int8_t> *parity = nullptr) {
        this->k = k_factor;
        create_eo(mat, true, inner, parity);
    }
    LowPrecisionEvenOddGCR(Sparse<num_type> *mat, const GCR_Param<num_type> *inner, const std::vector<int8_t> *parity = nullptr) { create_eo(mat, false, inner, parity); }
    struct EoInfo { int64_t n, n_even, n_odd; int32_t width_eo, width_oe; int64_t tail_rows_eo, tail_rows_oe; bool real_slab, has_diag; int64_t stored_bytes; };
    EoInfo eo_info() {
        EoInfo i{};
        int32_t real = 0, diag = 0;
        mgcr_detail::ok(mgcr_gcr32_eo_info(this->op, &i.n, &i.n_even, &i.n_odd, &i.width_eo, &i.width_oe, &i.tail_rows_eo, &i.tail_rows_oe, &real, &diag,
                                           &i.stored_bytes), "LowPrecisionEvenOddGCR::eo_info");
        i.real_slab = real != 0; i.has_diag = diag != 0;
        return i;
    }
    // (n, n_even, n_odd)
    std::vector<num_type> sizes() { const EoInfo i = eo_info(); return {(num_type)i.n, (num_type)i.n_even, (num_type)i.n_odd}; }
    // a_even and 1 / a_odd in single precision, as the device holds them
    void diag(std::vector<std::complex<float>> &a_even, std::vector<std::complex<float>> &inv_a_odd) {
        const EoInfo i = eo_info();
        a_even.resize((size_t)i.n_even); inv_a_odd.resize((size_t)i.n_odd);
        mgcr_detail::ok(mgcr_gcr32_eo_diag(this->op, reinterpret_cast<float *>(a_even.data()), reinterpret_cast<float *>(inv_a_odd.data())),
                        "LowPrecisionEvenOddGCR::diag");
    }

private:
    void create_eo(Sparse<num_type> *mat, bool dirac, const GCR_Param<num_type> *inner, const std::vector<int8_t> *parity) {
        mgcr_detail::ensure_init();
        const num_type rows = mat->get_nrow();
        if (parity && (num_type)parity->size() != rows) { std::fprintf(stderr, "LowPrecisionEvenOddGCR: parity has %zu entries, the matrix has %lld rows\n", parity->size(), (long long)rows); std::abort(); }
        std::vector<int64_t> rp, ci;
        std::vector<std::complex<double>> va;
        this->host_csr(mat, rp, ci, va);
        double v[2] = {this->k.real(), this->k.imag()};
        mgcr_gcr_param p = this->cparam(inner);
        mgcr_detail::ok(mgcr_gcr32_create_eo((int64_t)rows, rp.data(), ci.data(), reinterpret_cast<const double *>(va.data()), parity ? parity->data() : nullptr,
                                             dirac ? v : nullptr, &p, &this->op), "LowPrecisionEvenOddGCR");
        int64_t ne = 0;
        mgcr_detail::ok(mgcr_gcr32_eo_info(this->op, nullptr, &ne, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "LowPrecisionEvenOddGCR");
        this->dim = (num_type)ne;
    }
};

// EvenOddDiracOp: the even-odd (red-black) preconditioned Id - k*D (extension, mgcr_eo_create) — an Operator on the EVEN half of the
// rows, S = Id - k^2 D_eo D_oe.  D is a Sparse holding a pure hopping matrix (square, no diagonal, even rows coupled to odd rows
// only; its arrays are copied, so later changes of the Sparse are not seen).  GCR(&op, &param) solves the Schur system like any other
// operator; solve() runs prepare -> GCR -> reconstruct on full-system Fields and keeps the Schur solve's history (relative to
// |bhat_e|), iteration count and flag.  Fields of a half are plain one-dimensional Fields of n_even / n_odd entries.
template <typename num_type>
class EvenOddDiracOp : public Operator<num_type> {
public:
    EvenOddDiracOp(Sparse<num_type> *mat, std::complex<double> k_factor, const std::vector<int8_t> *parity = nullptr) : k(k_factor) {
        create(mat, parity, 0);
    }

protected:
    // how: 0 mgcr_eo_create; 1 mgcr_eo_create_diag in Dirac form (k); 2 mgcr_eo_create_diag in matrix form (no k);
    // 3 / 4 mgcr_eo_create_block in Dirac / matrix form with sites of bs rows
    EvenOddDiracOp() {}
    void create(Sparse<num_type> *mat, const std::vector<int8_t> *parity, int how, int bs = 1) {
        mgcr_detail::ensure_init();
        const num_type rows = mat->get_nrow(), nnz = mat->get_nnz();
        if (rows != mat->get_dim()) { std::fprintf(stderr, "EvenOddDiracOp: matrix must be square\n"); std::abort(); }
        if (parity && (num_type)parity->size() != rows) { std::fprintf(stderr, "EvenOddDiracOp: parity has %zu entries, the matrix has %lld rows\n", parity->size(), (long long)rows); std::abort(); }
        std::vector<int64_t> rp((size_t)rows + 1), ci((size_t)nnz);
        std::vector<std::complex<double>> va((size_t)nnz);
        for (num_type i = 0; i <= rows; i++) rp[(size_t)i] = (int64_t)mat->get_ROW(i);
        for (num_type i = 0; i < nnz; i++) { ci[(size_t)i] = (int64_t)mat->get_COL(i); va[(size_t)i] = mat->val_at(i); }
        double v[2] = {k.real(), k.imag()};
        const double *vals = reinterpret_cast<const double *>(va.data());
        const int8_t *par = parity ? parity->data() : nullptr;
        if (how == 0) mgcr_detail::ok(mgcr_eo_create((int64_t)rows, rp.data(), ci.data(), vals, par, v, &op), "EvenOddDiracOp");
        else if (how <= 2) mgcr_detail::ok(mgcr_eo_create_diag((int64_t)rows, rp.data(), ci.data(), vals, par, how == 1 ? v : nullptr, &op), "EvenOddDiagDiracOp");
        else mgcr_detail::ok(mgcr_eo_create_block((int64_t)rows, rp.data(), ci.data(), vals, (int32_t)bs, par, how == 3 ? v : nullptr, &op), "EvenOddBlockDiracOp");
        int64_t nn = 0, ne = 0, no = 0;
        mgcr_detail::ok(mgcr_eo_info(op, &nn, &ne, &no), "EvenOddDiracOp");
        n = (num_type)nn; n_even = (num_type)ne; n_odd = (num_type)no;
        this->dim = n_even;
    }

public:
    EvenOddDiracOp(EvenOddDiracOp const &) = delete;
    EvenOddDiracOp &operator=(EvenOddDiracOp const &) = delete;
    ~EvenOddDiracOp() override { if (op) mgcr_op_destroy(op); }
    std::complex<double> val_at(num_type, num_type) const override { return not_stored(); }
    std::complex<double> val_at(num_type) const override { return not_stored(); }
    Field<num_type> operator()(Field<num_type> const &f) override { return this->apply_handle(f, op, n_even); }
    mgcr_op_t handle() override { return op; }
    void set_k(std::complex<double> new_k) { k = new_k; double v[2] = {k.real(), k.imag()}; mgcr_detail::ok(mgcr_eo_set_k(op, v), "EvenOddDiracOp::set_k"); }
    num_type get_n() const { return n; }
    num_type get_n_even() const { return n_even; }
    num_type get_n_odd() const { return n_odd; }
    std::vector<int8_t> parity() const {
        std::vector<int8_t> out((size_t)n);
        mgcr_detail::ok(mgcr_eo_parity(op, out.data()), "EvenOddDiracOp::parity");
        return out;
    }
    void split(const Field<num_type> &full, Field<num_type> &even, Field<num_type> &odd) {
        mgcr_detail::ok(mgcr_eo_split(op, full.device(), even.device(), odd.device()), "EvenOddDiracOp::split");
        even.device_written(); odd.device_written();
    }
    void merge(const Field<num_type> &even, const Field<num_type> &odd, Field<num_type> &full) {
        mgcr_detail::ok(mgcr_eo_merge(op, even.device(), odd.device(), full.device()), "EvenOddDiracOp::merge");
        full.device_written();
    }
    Field<num_type> prepare(const Field<num_type> &rhs_full) {   // bhat_e = b_e + k D_eo b_o
        Field<num_type> out(&n_even, 1);
        mgcr_detail::ok(mgcr_eo_prepare(op, rhs_full.device(), out.device()), "EvenOddDiracOp::prepare");
        out.device_written();
        return out;
    }
    Field<num_type> reconstruct(const Field<num_type> &rhs_full, const Field<num_type> &x_even) {   // x_o = b_o + k D_oe x_e, merged with x_e
        Field<num_type> out(rhs_full.get_mesh());
        mgcr_detail::ok(mgcr_eo_reconstruct(op, rhs_full.device(), x_even.device(), out.device()), "EvenOddDiracOp::reconstruct");
        out.device_written();
        return out;
    }
    // (Id - k D) x_full = rhs_full through the Schur system; x_full's even half is the start vector where param->use_x0 asks for one
    void solve(const Field<num_type> &rhs_full, Field<num_type> &x_full, GCR_Param<num_type> *param) {
        if (param->truncation != 0 && param->restart != 0) { std::fprintf(stderr, "Do not support concurrent restarting and truncation.\n"); std::abort(); }
        mgcr_gcr_param p;
        std::memset(&p, 0, sizeof(p));
        p.truncation = param->truncation; p.restart = param->restart; p.max_iter = param->max_iter; p.tol = param->tol;
        p.verbose = param->verbose ? 1 : 0;
        p.left_precond = param->left_precond ? param->left_precond->handle() : nullptr;
        p.right_precond = param->right_precond ? param->right_precond->handle() : nullptr;
        p.use_x0 = param->use_x0; p.flexible = param->flexible;
        const int cap = (param->max_iter > 0 ? param->max_iter : 1) + 1;
        last_history.assign((size_t)cap, 0.);
        int32_t it = 0, conv = 0;
        mgcr_detail::ok(mgcr_eo_solve(op, &p, rhs_full.device(), x_full.device(), last_history.data(), cap, &it, &conv), "EvenOddDiracOp::solve");
        x_full.device_written();
        last_history.resize((size_t)it + 1);
        last_iterations = it; last_converged = conv != 0;
    }
    std::vector<double> last_history;   // of the Schur solve, relative to |bhat_e|
    int last_iterations = 0;
    bool last_converged = false;
    // (Id - ks[s] D) x_s = rhs_s for any number of systems on full-system Fields, through `width` <= 16 columns of ONE batched solve
    // of the Schur systems (extension, mgcr_eo_solve_queue): a column whose system has stopped is reconstructed into its x Field
    // and takes the next waiting system at the next boundary of the restart cycle.  This operator's own k is neither used nor
    // changed.  rhs may repeat, the x Fields are distinct and updated in place; per SYSTEM: queue_history[s] (relative to
    // |bhat_e,s|), queue_iterations[s], queue_converged[s] — the bits of solve() at ks[s] on that system alone.
    void solve_queue(const std::vector<const Field<num_type> *> &rhs, const std::vector<Field<num_type> *> &x, const std::vector<std::complex<double>> &ks,
                     GCR_Param<num_type> *param, int width = 8) {
        if (rhs.size() != x.size() || ks.size() != rhs.size()) { std::fprintf(stderr, "EvenOddDiracOp::solve_queue: one x and one k per right-hand side\n"); std::abort(); }
        if (param->truncation != 0 && param->restart != 0) { std::fprintf(stderr, "Do not support concurrent restarting and truncation.\n"); std::abort(); }
        mgcr_gcr_param p;
        std::memset(&p, 0, sizeof(p));
        p.truncation = param->truncation; p.restart = param->restart; p.max_iter = param->max_iter; p.tol = param->tol;
        p.verbose = param->verbose ? 1 : 0;
        p.left_precond = param->left_precond ? param->left_precond->handle() : nullptr;
        p.right_precond = param->right_precond ? param->right_precond->handle() : nullptr;
        p.use_x0 = param->use_x0; p.flexible = param->flexible;
        const int nsys = (int)rhs.size(), cap = (param->max_iter > 0 ? param->max_iter : 1) + 1;
        std::vector<mgcr_vec_t> bh, xh;
        for (int s = 0; s < nsys; s++) { bh.push_back(rhs[(size_t)s]->device()); xh.push_back(x[(size_t)s]->device()); }
        std::vector<double> kri, hist((size_t)nsys * cap, 0.);
        for (const std::complex<double> &kk : ks) { kri.push_back(kk.real()); kri.push_back(kk.imag()); }
        std::vector<int32_t> it((size_t)nsys, 0), conv((size_t)nsys, 0);
        mgcr_detail::ok(mgcr_eo_solve_queue(op, &p, width, nsys, bh.data(), xh.data(), kri.data(), hist.data(), cap, it.data(), conv.data()),
                        "EvenOddDiracOp::solve_queue");
        queue_history.assign((size_t)nsys, std::vector<double>());
        queue_iterations.assign(it.begin(), it.end());
        queue_converged.assign((size_t)nsys, false);
        for (int s = 0; s < nsys; s++) {
            x[(size_t)s]->device_written();
            queue_history[(size_t)s].assign(hist.begin() + (size_t)s * cap, hist.begin() + (size_t)s * cap + it[(size_t)s] + 1);
            queue_converged[(size_t)s] = conv[(size_t)s] != 0;
        }
    }
    std::vector<std::vector<double>> queue_history;
    std::vector<int> queue_iterations;
    std::vector<bool> queue_converged;

protected:
    static std::complex<double> not_stored() {
        std::fprintf(stderr, "EvenOddDiracOp::val_at: the Schur complement is applied, never formed\n");
        std::abort();
    }
    std::complex<double> k = 0.;
    num_type n = 0, n_even = 0, n_odd = 0;
    mgcr_op_t op = nullptr;
};

// EvenOddDiagDiracOp: the even-odd preconditioned Id - k D where D may store a SITE diagonal d (extension, mgcr_eo_create_diag in
// Dirac form): with a = 1 - k d the operator on the even half is S = diag(a_e) - k^2 D_eo diag(1/a_o) D_oe, D_eo / D_oe the
// off-diagonal halves.  Everything else is EvenOddDiracOp's; solve_queue and MultiEvenOddDiracOp refuse an operator that carries a
// diagonal.  diag() downloads a_e and 1 / a_o as the device holds them.
template <typename num_type>
class EvenOddDiagDiracOp : public EvenOddDiracOp<num_type> {
public:
    EvenOddDiagDiracOp(Sparse<num_type> *mat, std::complex<double> k_factor, const std::vector<int8_t> *parity = nullptr) {
        this->k = k_factor;
        this->create(mat, parity, 1);
    }
    void diag(std::vector<std::complex<double>> &a_even, std::vector<std::complex<double>> &inv_a_odd) {
        a_even.resize((size_t)this->n_even);
        inv_a_odd.resize((size_t)this->n_odd);
        mgcr_detail::ok(mgcr_eo_diag(this->op, reinterpret_cast<double *>(a_even.data()), reinterpret_cast<double *>(inv_a_odd.data())), "EvenOddDiagDiracOp::diag");
    }

protected:
    EvenOddDiagDiracOp() {}
};

// EvenOddSparse: the even-odd preconditioned form of a matrix M ITSELF (extension, mgcr_eo_create_diag in matrix form): a Poisson
// matrix, a Wilson operator written with its mass term.  S = diag(d_e) - M_eo diag(1/d_o) M_oe on the even half; solve() solves
// M x_full = rhs_full.  There is no hopping parameter: set_k is refused by the library.
template <typename num_type>
class EvenOddSparse : public EvenOddDiagDiracOp<num_type> {
public:
    explicit EvenOddSparse(Sparse<num_type> *mat, const std::vector<int8_t> *parity = nullptr) { this->create(mat, parity, 2); }
};

// EvenOddBlockDiracOp: the even-odd preconditioned Id - k D where D couples the bs consecutive rows of a SITE (extension,
// mgcr_eo_create_block in Dirac form; a clover-type operator): with B_s = I - k D_ss the operator on the even half is
// S = B_e - k^2 D_eo B_o^-1 D_oe, D_eo / D_oe the inter-site halves.  Everything else is EvenOddDiracOp's; solve_queue and
// MultiEvenOddDiracOp refuse an operator with blocks.  block_diag() downloads B_e and B_o^-1 as the device holds them, row-major.
template <typename num_type>
class EvenOddBlockDiracOp : public EvenOddDiracOp<num_type> {
public:
    EvenOddBlockDiracOp(Sparse<num_type> *mat, std::complex<double> k_factor, int bs, const std::vector<int8_t> *parity = nullptr) {
        this->k = k_factor;
        this->create(mat, parity, 3, bs);
    }
    void block_info(int &bs, num_type &sites_even, num_type &sites_odd) {
        int32_t b = 0;
        int64_t se = 0, so = 0;
        mgcr_detail::ok(mgcr_eo_block_info(this->op, &b, &se, &so), "EvenOddBlockDiracOp::block_info");
        bs = (int)b; sites_even = (num_type)se; sites_odd = (num_type)so;
    }
    void block_diag(std::vector<std::complex<double>> &B_even, std::vector<std::complex<double>> &invB_odd) {
        int bs = 0;
        num_type se = 0, so = 0;
        block_info(bs, se, so);
        B_even.resize((size_t)se * bs * bs);
        invB_odd.resize((size_t)so * bs * bs);
        mgcr_detail::ok(mgcr_eo_block_diag(this->op, reinterpret_cast<double *>(B_even.data()), reinterpret_cast<double *>(invB_odd.data())),
                        "EvenOddBlockDiracOp::block_diag");
    }

protected:
    EvenOddBlockDiracOp() {}
};

// EvenOddBlockSparse: the even-odd preconditioned form of a matrix M ITSELF whose diagonal is a dense block per site (extension,
// mgcr_eo_create_block in matrix form): S = M_ee - M_eo M_oo^-1 M_oe on the even half; solve() solves M x_full = rhs_full.
template <typename num_type>
class EvenOddBlockSparse : public EvenOddBlockDiracOp<num_type> {
public:
    EvenOddBlockSparse(Sparse<num_type> *mat, int bs, const std::vector<int8_t> *parity = nullptr) { this->create(mat, parity, 4, bs); }
};

// MultiEvenOddDiracOp: the Schur complements Id - ks[j]^2 D_eo D_oe of ONE hopping matrix on column j of a block of ks.size() Fields
// of the even half — an even-odd hopping-parameter scan as one operator (extension, mgcr_eo_multi_create).  Borrows the halves and
// index lists of `eo`, which must outlive it; eo's own k is not used.  apply_multi, GCR::solve_multi and the methods below take it,
// with MultiFields of exactly ncols() columns; column j has the bits of EvenOddDiracOp(D, ks[j]) on that column alone.  solve() runs
// prepare -> batched GCR -> reconstruct on full-system MultiFields and keeps, per column, the Schur solve's history (relative to
// |bhat_e,j|), iteration count and flag.
template <typename num_type>
class MultiEvenOddDiracOp : public Operator<num_type> {
public:
    MultiEvenOddDiracOp(EvenOddDiracOp<num_type> *eo_op, std::vector<std::complex<double>> k_factors) : ks(std::move(k_factors)), eo(eo_op) {
        mgcr_detail::ok(mgcr_eo_multi_create(eo->handle(), (int32_t)ks.size(), reinterpret_cast<const double *>(ks.data()), &op), "MultiEvenOddDiracOp");
        this->dim = eo->get_n_even();
    }
    MultiEvenOddDiracOp(MultiEvenOddDiracOp const &) = delete;
    MultiEvenOddDiracOp &operator=(MultiEvenOddDiracOp const &) = delete;
    ~MultiEvenOddDiracOp() override { if (op) mgcr_op_destroy(op); }
    int ncols() const { return (int)ks.size(); }
    std::complex<double> val_at(num_type, num_type) const override { return no_single("val_at"); }
    std::complex<double> val_at(num_type) const override { return no_single("val_at"); }
    Field<num_type> operator()(Field<num_type> const &f) override { no_single("operator()"); return f; }
    mgcr_op_t handle() override { return op; }
    void set_k(std::vector<std::complex<double>> new_ks) {   // same count; holds for every later call, never for enqueued work
        if (new_ks.size() != ks.size()) { std::fprintf(stderr, "MultiEvenOddDiracOp::set_k: %zu values for %zu columns\n", new_ks.size(), ks.size()); std::abort(); }
        ks = std::move(new_ks);
        mgcr_detail::ok(mgcr_eo_multi_set_k(op, reinterpret_cast<const double *>(ks.data())), "MultiEvenOddDiracOp::set_k");
    }
    num_type get_n() const { return eo->get_n(); }
    num_type get_n_even() const { return eo->get_n_even(); }
    num_type get_n_odd() const { return eo->get_n_odd(); }
    void split(const MultiField<num_type> &full, MultiField<num_type> &even, MultiField<num_type> &odd) {
        mgcr_detail::ok(mgcr_eo_multi_split(op, full.device(), even.device(), odd.device()), "MultiEvenOddDiracOp::split");
    }
    void merge(const MultiField<num_type> &even, const MultiField<num_type> &odd, MultiField<num_type> &full) {
        mgcr_detail::ok(mgcr_eo_multi_merge(op, even.device(), odd.device(), full.device()), "MultiEvenOddDiracOp::merge");
    }
    MultiField<num_type> prepare(const MultiField<num_type> &rhs_full) {   // bhat_e,j = b_e,j + ks[j] D_eo b_o,j
        num_type ne = eo->get_n_even();
        MultiField<num_type> out(Mesh<num_type>(&ne, 1), ncols());
        mgcr_detail::ok(mgcr_eo_multi_prepare(op, rhs_full.device(), out.device()), "MultiEvenOddDiracOp::prepare");
        return out;
    }
    MultiField<num_type> reconstruct(const MultiField<num_type> &rhs_full, const MultiField<num_type> &x_even) {   // x_o,j = b_o,j + ks[j] D_oe x_e,j, merged
        MultiField<num_type> out(rhs_full.get_mesh(), ncols());
        mgcr_detail::ok(mgcr_eo_multi_reconstruct(op, rhs_full.device(), x_even.device(), out.device()), "MultiEvenOddDiracOp::reconstruct");
        return out;
    }
    // (Id - ks[j] D) x_full,j = rhs_full,j for every column through ONE batched solve of the Schur systems (restart mode, unpreconditioned)
    void solve(const MultiField<num_type> &rhs_full, MultiField<num_type> &x_full, GCR_Param<num_type> *param) {
        if (param->truncation != 0 && param->restart != 0) { std::fprintf(stderr, "Do not support concurrent restarting and truncation.\n"); std::abort(); }
        mgcr_gcr_param p;
        std::memset(&p, 0, sizeof(p));
        p.truncation = param->truncation; p.restart = param->restart; p.max_iter = param->max_iter; p.tol = param->tol;
        p.verbose = param->verbose ? 1 : 0;
        p.left_precond = param->left_precond ? param->left_precond->handle() : nullptr;
        p.right_precond = param->right_precond ? param->right_precond->handle() : nullptr;
        p.use_x0 = param->use_x0; p.flexible = param->flexible;
        const int k = ncols(), cap = (param->max_iter > 0 ? param->max_iter : 1) + 1;
        std::vector<double> hist((size_t)k * cap, 0.);
        std::vector<int32_t> it((size_t)k, 0), conv((size_t)k, 0);
        mgcr_detail::ok(mgcr_eo_multi_solve(op, &p, rhs_full.device(), x_full.device(), hist.data(), cap, it.data(), conv.data()), "MultiEvenOddDiracOp::solve");
        last_history.assign((size_t)k, std::vector<double>());
        last_iterations.assign(it.begin(), it.end());
        last_converged.assign((size_t)k, false);
        for (int j = 0; j < k; j++) {
            last_history[(size_t)j].assign(hist.begin() + (size_t)j * cap, hist.begin() + (size_t)j * cap + it[(size_t)j] + 1);
            last_converged[(size_t)j] = conv[(size_t)j] != 0;
        }
    }
    std::vector<std::vector<double>> last_history;   // of the Schur solves, column j relative to |bhat_e,j|
    std::vector<int> last_iterations;
    std::vector<bool> last_converged;

private:
    static std::complex<double> no_single(const char *what) {
        std::fprintf(stderr, "MultiEvenOddDiracOp::%s: one hopping parameter per column of a block; use apply_multi / GCR::solve_multi / solve\n", what);
        std::abort();
    }
    std::vector<std::complex<double>> ks;
    EvenOddDiracOp<num_type> *eo;
    mgcr_op_t op = nullptr;
};

// ------------------------------------------------------------------------------------------------
// MG — src/MG.h:20-61.  operator() is the corrected V-cycle of DESIGN.md (the reference's returns
// uninitialised memory, src/MG.h:124-129).
// ------------------------------------------------------------------------------------------------
template <typename num_type>
class MG : public Operator<num_type> {
public:
    MG() = default;
    MG(Operator<num_type> *M, MG_Param<num_type> *parameter) : param(parameter) { initialise(M); }
    explicit MG(MG_Param<num_type> *parameter) : param(parameter) {}
    ~MG() override { if (op) mgcr_op_destroy(op); }

    void initialise(Operator<num_type> *M) override {  // :131-285
        m = M;
        this->dim = M->get_dim();
        std::printf("Compute global eigenvectors...\n");
        std::vector<Field<num_type>> vecs = param->null_vectors ? *param->null_vectors : near_null(M);
        const int nd = param->mesh.get_ndim();
        int spinor_index = -1;
        for (int d = 0; d < nd && d < 6; d++) if (param->spinor[d]) spinor_index = d;
        std::vector<std::complex<double>> all;
        auto append = [&](const Field<num_type> &f) { for (num_type i = 0; i < f.field_size(); i++) all.push_back(f.val_at(i)); };
        if (spinor_index >= 0) {  // vec_double :316-345
            for (auto &v : vecs) append((v + v.gamma5(spinor_index)) * 0.5);
            for (auto &v : vecs) append((v - v.gamma5(spinor_index)) * 0.5);
        } else {
            for (auto &v : vecs) append(v);
        }
        mgcr_mg_param p;
        std::memset(&p, 0, sizeof(p));
        p.ndim = nd;
        for (int d = 0; d < nd; d++) { p.dims[d] = (int64_t)param->mesh.get_dims()[d]; p.blocked[d] = (d < 6 ? param->spacetime[d] : true) ? 1 : 0; }
        p.subblock_dim = (int64_t)param->subblock_dim;
        p.n_vec = (int32_t)(all.size() / (size_t)this->dim);
        p.vecs_ri = reinterpret_cast<const double *>(all.data());
        p.n_level = param->n_level;
        p.smoother = solver_param(param->smoother_solver);
        p.coarse = solver_param(param->coarse_solver);
        p.damping = param->damping;
        p.coarse_direct_rows = param->coarse_direct_rows;
        if (op) mgcr_op_destroy(op);
        mgcr_detail::ok(mgcr_mg_create(M->handle(), &p, &op), "MG::initialise");
        std::printf("Adaptive Multigrid precomputation completed.\n");
    }
    Field<num_type> expand(Field<num_type> &x_coarse) {  // :347-364
        Field<num_type> out(param->mesh);
        mgcr_detail::ok(mgcr_mg_expand(op, 0, x_coarse.device(), out.device()), "MG::expand");
        out.device_written();
        return out;
    }
    Field<num_type> restrict(Field<num_type> &x_fine) {  // :366-383
        int64_t dimc = 0;
        mgcr_detail::ok(mgcr_mg_level_info(op, 1, &dimc, nullptr, nullptr), "MG level");
        num_type d1[1] = {(num_type)dimc};
        Field<num_type> out(d1, 1);
        mgcr_detail::ok(mgcr_mg_restrict(op, 0, x_fine.device(), out.device()), "MG::restrict");
        out.device_written();
        return out;
    }
    std::complex<double> val_at(num_type, num_type) const override { std::printf("Warning: Exact value of MG should not be queried!\n"); return 0; }
    std::complex<double> val_at(num_type) const override { std::printf("Warning: Exact value of MG should not be queried!\n"); return 0; }
    Field<num_type> operator()(Field<num_type> const &f) override { return this->apply_handle(f, op, this->dim); }
    mgcr_op_t handle() override { return op; }

private:
    mgcr_gcr_param solver_param(Operator<num_type> *s) const {
        mgcr_gcr_param p;
        std::memset(&p, 0, sizeof(p));
        auto *g = dynamic_cast<GCR<num_type> *>(s);
        if (!g) { std::fprintf(stderr, "MG: smoother / coarse solver must be GCR objects\n"); std::abort(); }
        GCR_Param<num_type> *gp = g->get_param();
        p.truncation = gp->truncation; p.restart = gp->restart; p.max_iter = gp->max_iter; p.tol = gp->tol;
        return p;
    }
    // Arnoldi::solve :90-122 — inverse iteration for the smallest modes, Gram-Schmidt between them.
    // The start vector is init_rand(9) as in the reference, and the first vector follows the reference's literal loop
    // gcr.solve(b, b): rhs and x are one Field, i.e. x0 = b with r0 = b (src/GCR.h:189) — pinned against the real
    // reference in tests/test_gpu_mg.py::test_arnoldi_vs_reference.  The later vectors are solved from x0 = 0: the
    // reference solves them into a malloc'ed, never initialised Field (:110), which has no defined value.
    std::vector<Field<num_type>> near_null(Operator<num_type> *M) {
        GCR_Param<num_type> gp = *param->eigenvector_precomp_param;
        gp.verbose = false;
        GCR<num_type> gcr(M, &gp);
        Field<num_type> b(param->mesh), x(param->mesh);
        b.init_rand(9);
        std::printf("Computing smallest eigenvector 0\n");
        for (int i = 0; i < 10; i++) { x = b; gcr.solve(b, x); b = x; b.normalise(); }
        std::vector<Field<num_type>> v;
        v.push_back(b);
        for (int c = 1; c < param->n_eigen; c++) {
            std::printf("Computing smallest eigenvector %d\n", c);
            x.set_zero();
            gcr.solve(v.back(), x);
            Field<num_type> t(x);
            for (auto &e : v) { std::complex<double> hh = e.dot(t); t -= e * hh; }
            t.normalise();
            v.push_back(t);
        }
        return v;
    }
    MG_Param<num_type> *param = nullptr;
    Operator<num_type> *m = nullptr;
    mgcr_op_t op = nullptr;
};

// ------------------------------------------------------------------------------------------------
// read_data — src/Parse.cpp:64-90; text-CSR format of SURVEY.md Appendix B.  Opens
// "../../data/sample_matrix/" + filename like the reference ($MGCR_SAMPLE_DIR overrides the prefix).
// ------------------------------------------------------------------------------------------------
inline Sparse<long> read_data(const std::string &filename) {
    const char *pre = std::getenv("MGCR_SAMPLE_DIR");
    std::string prefix = pre ? std::string(pre) + "/" : "../../data/sample_matrix/";
    std::ifstream file(prefix + filename);
    if (file) std::printf("File read is successful.\n");
    else std::printf("File read is unsuccessful!\n");
    long row = 0, col = 0, nnz = 0;
    file >> row >> col >> nnz;
    Sparse<long> output(row, col, nnz);
    for (long i = 0; i < row; i++) { long v; file >> v; output.mod_ROW_at(i, v); }
    for (long i = 0; i < nnz; i++) { long c; std::complex<double> v; file >> c >> v; output.mod_COL_at(i, c); output.mod_VAL_at(i, v); }
    return output;
}

// parse_data — src/Parse.cpp:9-61: MatrixMarket `complex coordinate` -> text CSR ("parsed.txt" next to the
// sample data; $MGCR_SAMPLE_DIR overrides the directory).  Duplicates are summed by the triplet constructor.
inline void parse_data(const std::string &file_loc) {
    std::ifstream file(file_loc);
    if (file) std::printf("File read is successful.\n");
    else { std::printf("File read is unsuccessful!\n"); return; }
    while (file.peek() == '%') file.ignore(1 << 20, '\n');
    long rows = 0, cols = 0, elements = 0;
    file >> rows >> cols >> elements;
    std::vector<std::pair<std::complex<double>, std::pair<long, long>>> trip((size_t)elements);
    for (long l = 0; l < elements; l++) {
        long r, c;
        double re, im;
        file >> r >> c >> re >> im;
        trip[(size_t)l] = {std::complex<double>(re, im), {r - 1, c - 1}};
    }
    Sparse<long> sparse(rows, cols, trip.data(), elements);
    const char *pre = std::getenv("MGCR_SAMPLE_DIR");
    std::ofstream out((pre ? std::string(pre) + "/" : std::string("../../data/sample_matrix/")) + "parsed.txt");
    out << sparse.get_nrow() << " " << sparse.get_dim() << " " << sparse.get_nnz() << "\n";
    for (long i = 0; i < sparse.get_nrow(); i++) out << sparse.get_ROW(i) << " ";
    for (long j = 0; j < sparse.get_nnz(); j++) out << "\n" << sparse.get_COL(j) << " " << sparse.val_at(j);
}

#endif  // MGCR_DROPIN_HPP
