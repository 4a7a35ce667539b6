"""Host-side mirror of the reference's Operator / Field / SolverParam interface over the C ABI.

Same names, argument meaning and error behaviour as the reference's C++ classes (paths relative
to the reference root); the data lives in HBM and every operation is a HIP kernel of
libmgcr_hip.so.  This Python layer is what tests/ and bench.py drive; the C++ twin of the same
interface is include/mgcr/*.h.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import GcrParamC, MgParamC, MgcrError, check

c128 = np.complex128


def _ri(z):
    z = complex(z)
    return (C.c_double * 2)(z.real, z.imag)


def set_option(name, value):
    """mgcr_set_option: switch between equivalent code paths ("pattern_storage", "lean_cycles"); returns the old value."""
    prev = C.c_int()
    check(_lib.lib().mgcr_set_option(name.encode(), int(value), C.byref(prev)))
    return prev.value


def stat(name):
    """mgcr_stat: a counter of the library ("resident_solves")."""
    v = C.c_int64()
    check(_lib.lib().mgcr_stat(name.encode(), C.byref(v)))
    return v.value


class Field:
    """Field<num_type> (src/Fields.h:29-71): complex-fp64 vector tagged with mesh dimensions."""

    def __init__(self, dims, data=None):
        _lib.init()
        if isinstance(dims, (int, np.integer)):
            dims = (int(dims),)
        self.dims = tuple(int(d) for d in dims)
        n = int(np.prod(self.dims, dtype=np.int64))
        h = C.c_void_p()
        check(_lib.lib().mgcr_vec_create(n, C.byref(h)))
        self.h = h
        self._n = n
        if data is not None:
            self.upload(data)

    # -- construction / queries
    @classmethod
    def like(cls, other):
        return cls(other.dims)

    def field_size(self):  # src/Fields.h:120-123
        return self._n

    def get_ndim(self):
        return len(self.dims)

    def upload(self, data):
        a = np.ascontiguousarray(data, dtype=c128).reshape(-1)
        if a.size != self._n:
            raise MgcrError(1, "Dimension mismatch.")
        check(_lib.lib().mgcr_vec_upload(self.h, a.ctypes.data))
        return self

    def to_numpy(self):
        out = np.empty(self._n, c128)
        check(_lib.lib().mgcr_vec_download(self.h, out.ctypes.data))
        return out

    def val_at(self, location):  # src/Fields.h:163-168 (host convenience, one element)
        if not 0 <= location < self._n:
            raise MgcrError(1, "Field memory access out of bound!")
        return self.to_numpy()[location]

    def set_zero(self):  # src/Fields.h:137-145
        check(_lib.lib().mgcr_vec_zero(self.h))
        return self

    def set_constant(self, c):  # src/Fields.h:146-151
        check(_lib.lib().mgcr_vec_set_constant(self.h, _ri(c)))
        return self

    def fill_rhs(self, seed=0, global_offset=0):
        """Deterministic repo-owned stand-in for init_rand (src/Fields.h:125-135)."""
        check(_lib.lib().mgcr_vec_fill_rhs(self.h, seed, global_offset))
        return self

    def assign(self, other):  # operator= src/Fields.h:256-286
        check(_lib.lib().mgcr_vec_copy(self.h, other.h))
        return self

    def copy(self):
        return Field(self.dims).assign(self)

    # -- algebra (value semantics like the reference; the fused solver kernels do not use these)
    def dot(self, other):  # src/Fields.h:216-226
        out = (C.c_double * 2)()
        check(_lib.lib().mgcr_dot(self.h, other.h, out))
        return complex(out[0], out[1])

    def squarednorm(self):  # src/Fields.h:228-235
        out = C.c_double()
        check(_lib.lib().mgcr_norm2(self.h, C.byref(out)))
        return out.value

    def norm(self):
        return float(np.sqrt(self.squarednorm()))

    def add_scaled(self, alpha, other):
        """self + other*alpha as a new Field (operator+ with operator*, src/Fields.h:192-253)."""
        out = Field(self.dims)
        check(_lib.lib().mgcr_add_scaled(out.h, self.h, _ri(alpha), other.h))
        return out

    def __add__(self, other):
        return self.add_scaled(1.0, other)

    def __sub__(self, other):
        return self.add_scaled(-1.0, other)

    def __mul__(self, a):  # src/Fields.h:245-253
        out = self.copy()
        check(_lib.lib().mgcr_scale(out.h, _ri(a)))
        return out

    def __iadd__(self, other):  # src/Fields.h:288-297
        check(_lib.lib().mgcr_axpy(_ri(1.0), other.h, self.h))
        return self

    def __isub__(self, other):
        check(_lib.lib().mgcr_axpy(_ri(-1.0), other.h, self.h))
        return self

    def normalise(self):  # src/Fields.h:237-243
        check(_lib.lib().mgcr_normalise(self.h))
        return self

    def gamma5(self, spinor_index=4):  # src/Fields.h:310-339
        """New Field with the spinor components swapped 0<->2, 1<->3 (on the device)."""
        if self.dims[spinor_index] != 4:
            raise ValueError("gamma5: dimension %d of the mesh has %d entries, not 4" % (spinor_index, self.dims[spinor_index]))
        inner = int(np.prod(self.dims[spinor_index + 1:], dtype=np.int64))
        out = Field(self.dims)
        check(_lib.lib().mgcr_vec_gamma5(self.h, out.h, inner))
        return out

    def __del__(self):
        try:
            if getattr(self, "h", None):
                _lib.lib().mgcr_vec_destroy(self.h)
                self.h = None
        except Exception:
            pass


class MultiField:
    """Block of k Fields on one mesh (multi-RHS; the reference has no counterpart).  On the device the columns are interleaved
    (element (row i, column j) at i * k + j, include/mgcr.h); on the host a block is a (k, n) complex128 array."""

    def __init__(self, dims, k, data=None):
        _lib.init()
        if isinstance(dims, (int, np.integer)):
            dims = (int(dims),)
        self.dims = tuple(int(d) for d in dims)
        self.k = int(k)
        n = int(np.prod(self.dims, dtype=np.int64))
        h = C.c_void_p()
        check(_lib.lib().mgcr_mvec_create(n, self.k, C.byref(h)))
        self.h = h
        self._n = n
        if data is not None:
            self.upload(data)

    @classmethod
    def from_fields(cls, fields):
        """Packs Fields of one size into a block, on the device."""
        fields = list(fields)
        if not fields:
            raise MgcrError(1, "MultiField.from_fields: no Fields")
        out = cls(fields[0].dims, len(fields))
        for j, f in enumerate(fields):
            check(_lib.lib().mgcr_mvec_set_column(out.h, j, f.h))
        return out

    @classmethod
    def like(cls, other):
        return cls(other.dims, other.k)

    def field_size(self):
        return self._n

    def ncols(self):
        return self.k

    def upload(self, data):
        a = np.ascontiguousarray(data, dtype=c128)
        if a.size != self._n * self.k:
            raise MgcrError(1, "Dimension mismatch.")
        check(_lib.lib().mgcr_mvec_upload(self.h, a.ctypes.data))
        return self

    def to_numpy(self):
        out = np.empty((self.k, self._n), c128)
        check(_lib.lib().mgcr_mvec_download(self.h, out.ctypes.data))
        return out

    def column(self, j):
        """Column j as a new Field (device-side unpack)."""
        out = Field(self.dims)
        check(_lib.lib().mgcr_mvec_get_column(self.h, int(j), out.h))
        return out

    def set_column(self, j, field):
        check(_lib.lib().mgcr_mvec_set_column(self.h, int(j), field.h))
        return self

    def set_zero(self):
        check(_lib.lib().mgcr_mvec_zero(self.h))
        return self

    def dot(self, other):
        """k dot products <self_j, other_j> (conj on self) in one pass; column j has the bits of Field.dot on that column."""
        out = (C.c_double * (2 * self.k))()
        check(_lib.lib().mgcr_mvec_dot(self.h, other.h, out))
        return np.array([complex(out[2 * j], out[2 * j + 1]) for j in range(self.k)], c128)

    def squarednorm(self):
        out = (C.c_double * self.k)()
        check(_lib.lib().mgcr_mvec_norm2(self.h, out))
        return np.array(out[:], np.float64)

    def axpy(self, alpha, x):
        """self_j += alpha_j * x_j (alpha: one value, or k of them)."""
        al = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, c128), (self.k,)))
        check(_lib.lib().mgcr_mvec_axpy(al.ctypes.data_as(C.POINTER(C.c_double)), x.h, self.h))
        return self

    def __del__(self):
        try:
            if getattr(self, "h", None):
                _lib.lib().mgcr_mvec_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Operator:
    """Operator<num_type> (src/Operator.h:16-29)."""

    def __init__(self):
        self.h = None
        self._keep = []

    def get_dim(self):
        return int(_lib.lib().mgcr_op_dim(self.h))

    def get_nrow(self):
        return int(_lib.lib().mgcr_op_nrow(self.h))

    def __call__(self, f, out=None):
        """Field operator()(const Field&): applies the operator, returns a new Field."""
        if out is None:
            nrow = self.get_nrow()
            out = Field(f.dims if nrow == f.field_size() else (nrow,))
        check(_lib.lib().mgcr_op_apply(self.h, f.h, out.h))
        return out

    def apply_multi(self, X, out=None):
        """Y = op(X) for a MultiField: the matrix is streamed once for all k columns; column j has the bits of op(X.column(j))."""
        if out is None:
            nrow = self.get_nrow()
            out = MultiField(X.dims if nrow == X.field_size() else (nrow,), X.k)
        check(_lib.lib().mgcr_op_apply_multi(self.h, X.h, out.h))
        return out

    def bench_apply_multi(self, X, Y, reps=20):
        ms = C.c_double()
        check(_lib.lib().mgcr_bench_op_apply_multi(self.h, X.h, Y.h, reps, C.byref(ms)))
        return ms.value

    def stored_bytes(self):
        b, w, t = C.c_int64(), C.c_int32(), C.c_int64()
        check(_lib.lib().mgcr_op_stored_bytes(self.h, C.byref(b), C.byref(w), C.byref(t)))
        return dict(matrix_bytes=b.value, ell_width=w.value, tail_nnz=t.value)

    def ell_layout(self):
        """dict(ell_width, lanes, tail_rows, reach, tail_chunk_cap): how a Sparse's rows are dealt to threads (include/mgcr.h)."""
        w, l, t, r, cap, win = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        check(_lib.lib().mgcr_op_ell_layout(self.h, C.byref(w), C.byref(l), C.byref(t), C.byref(r), C.byref(cap), C.byref(win)))
        return dict(ell_width=w.value, lanes=l.value, tail_rows=t.value, reach=r.value, tail_chunk_cap=cap.value, x_window=win.value)

    def xr_fuse_kind(self):
        """0 / 1 / 2: where a lean GCR on this operator runs its residual update (include/mgcr.h mgcr_op_xr_fuse_kind)."""
        k = C.c_int32()
        check(_lib.lib().mgcr_op_xr_fuse_kind(self.h, C.byref(k)))
        return k.value

    def storage_format(self):
        """(format, n_patterns): 0 ELL slab, 1 row-pattern dictionary (columns + values), 2 (columns only)."""
        f, n = C.c_int32(), C.c_int32()
        check(_lib.lib().mgcr_op_storage_format(self.h, C.byref(f), C.byref(n)))
        return f.value, n.value

    def bench_apply(self, x, y, reps=20):
        ms = C.c_double()
        check(_lib.lib().mgcr_bench_op_apply(self.h, x.h, y.h, reps, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            if getattr(self, "h", None):
                _lib.lib().mgcr_op_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Sparse(Operator):
    """Sparse<long> (src/Operator.h:56-101): CSR with int64 indices on the host side.  The host arrays are kept (the
    reference's get_ROW / get_COL / val_at accessors and its set-up-time algebra work on them); the device copy is what
    operator() uses."""

    def __init__(self, rows, cols, rowptr, col, val):
        super().__init__()
        _lib.init()
        rowptr = np.ascontiguousarray(rowptr, np.int64)
        col = np.ascontiguousarray(col, np.int64)
        val = np.ascontiguousarray(val, c128)
        if rowptr.size != rows + 1 or col.size != rowptr[-1] or val.size != col.size:
            raise MgcrError(1, "CSR arrays have inconsistent sizes")
        h = C.c_void_p()
        check(_lib.lib().mgcr_csr_create(rows, cols, rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, C.byref(h)))
        self.h = h
        self._nnz = int(rowptr[-1])
        self._shape = (int(rows), int(cols))
        self.ROW, self.COL, self.VAL = rowptr, col, val

    @classmethod
    def from_triplets(cls, rows, cols, trip_rows, trip_cols, trip_vals):
        """Sparse(rows, cols, triplets, n) (src/Operator.h:250-294): unordered triplets, duplicates summed."""
        from . import hostalg
        return cls(rows, cols, *hostalg.csr_from_triplets(rows, cols, trip_rows, trip_cols, trip_vals))

    def get_nnz(self):  # src/Operator.h:73
        return self._nnz

    def get_ROW(self, l):  # src/Operator.h:78-79
        return int(self.ROW[l])

    def get_COL(self, l):
        return int(self.COL[l])

    def val_at(self, row, col=None):  # src/Operator.h:392-402
        if col is None:
            return complex(self.VAL[row])
        for l in range(self.ROW[row], self.ROW[row + 1]):
            if self.COL[l] == col:
                return complex(self.VAL[l])
        return 0j

    def dagger(self):
        """void Sparse::dagger() (src/Operator.h:296-328): conjugate transpose IN PLACE (rows and columns swap)."""
        from . import hostalg
        nr, nc, rp, ci, va = hostalg.csr_dagger(self._shape[0], self._shape[1], self.ROW, self.COL, self.VAL)
        rp, ci, va = np.ascontiguousarray(rp, np.int64), np.ascontiguousarray(ci, np.int64), np.ascontiguousarray(va, c128)
        # the matrix changes BEHIND the handle (mgcr_csr_replace): a DiracOp / GCR that borrowed this Sparse — the
        # reference's DiracOp keeps a Sparse* (src/Operator.h:117) — applies the daggered matrix from now on
        check(_lib.lib().mgcr_csr_replace(self.h, nr, nc, rp.ctypes.data, ci.ctypes.data, va.ctypes.data))
        self._shape, self.ROW, self.COL, self.VAL = (int(nr), int(nc)), rp, ci, va
        self._nnz = int(rp[-1])
        return self

    def __mul__(self, a):
        """Sparse operator*(complex) (src/Operator.h:535-544): a new Sparse with every value scaled."""
        from . import hostalg
        return Sparse(self._shape[0], self._shape[1], self.ROW, self.COL, hostalg.csr_scale(self.VAL, a))


class DiracOp(Operator):
    """DiracOp = Id - k*D (src/Operator.h:104-122,555-575); borrows the Sparse."""

    def __init__(self, mat, k_factor):
        super().__init__()
        h = C.c_void_p()
        check(_lib.lib().mgcr_dirac_create(mat.h, _ri(k_factor), C.byref(h)))
        self.h = h
        self._keep.append(mat)
        self.comm, self.row0 = getattr(mat, "comm", None), getattr(mat, "row0", 0)

    def set_k(self, new_k):  # src/Operator.h:116
        check(_lib.lib().mgcr_dirac_set_k(self.h, _ri(new_k)))


class MultiDiracOp(Operator):
    """Id - ks[j]*D on column j of a block of len(ks) Fields: a hopping-parameter scan as ONE operator (mgcr_dirac_multi_create;
    no reference counterpart).  Borrows the Sparse.  Only apply_multi and GCR(...).solve_multi take it, with blocks of exactly
    ncols columns; column j has the bits of DiracOp(mat, ks[j]) on that column alone."""

    def __init__(self, mat, ks):
        super().__init__()
        kv = self._values(ks)
        h = C.c_void_p()
        check(_lib.lib().mgcr_dirac_multi_create(mat.h, kv.shape[0], kv.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h)))
        self.h = h
        self.ncols = int(kv.shape[0])
        self._keep.append(mat)

    @staticmethod
    def _values(ks):
        kv = np.atleast_1d(np.asarray(ks, c128)).reshape(-1)
        return np.ascontiguousarray(kv.view(np.float64).reshape(-1, 2))

    def set_k(self, ks):
        """Replace all ncols values; takes effect for every later apply / solve, never for work already enqueued."""
        kv = self._values(ks)
        if kv.shape[0] != self.ncols:
            raise MgcrError(1, "MultiDiracOp.set_k: %d values for %d columns" % (kv.shape[0], self.ncols))
        check(_lib.lib().mgcr_dirac_multi_set_k(self.h, kv.ctypes.data_as(C.POINTER(C.c_double))))


class EvenOddDiracOp(Operator):
    """The even-odd (red-black) preconditioned Id - k*D (mgcr_eo_create; no reference counterpart): an Operator on the EVEN half,
    S = Id - k^2 D_eo D_oe.  `mat` is a Sparse holding a pure hopping matrix (square, no diagonal, even rows coupled to odd rows
    only); its host arrays are copied.  parity: 0 even / 1 odd per row, or None — the rows are then two-coloured.  GCR(op, ...)
    solves the Schur system like any other; solve() runs prepare -> GCR -> reconstruct on full-system Fields."""

    def __init__(self, mat, k, parity=None):
        super().__init__()
        _lib.init()
        n = int(mat._shape[0])
        if mat._shape[0] != mat._shape[1]:
            raise MgcrError(1, "EvenOddDiracOp: matrix must be square")
        par = None if parity is None else np.ascontiguousarray(parity, np.int8)
        if par is not None and par.size != n:
            raise MgcrError(1, "EvenOddDiracOp: parity has %d entries, the matrix has %d rows" % (par.size, n))
        h = C.c_void_p()
        check(_lib.lib().mgcr_eo_create(n, mat.ROW.ctypes.data, mat.COL.ctypes.data, mat.VAL.ctypes.data,
                                        par.ctypes.data if par is not None else None, _ri(k), C.byref(h)))
        self.h = h
        self.last_history = None
        self.last_iterations = None
        self.last_converged = None

    def set_k(self, new_k):
        check(_lib.lib().mgcr_eo_set_k(self.h, _ri(new_k)))

    def sizes(self):
        """(n, n_even, n_odd)"""
        n, ne, no = C.c_int64(), C.c_int64(), C.c_int64()
        check(_lib.lib().mgcr_eo_info(self.h, C.byref(n), C.byref(ne), C.byref(no)))
        return n.value, ne.value, no.value

    def parity(self):
        par = np.empty(self.sizes()[0], np.int8)
        check(_lib.lib().mgcr_eo_parity(self.h, par.ctypes.data))
        return par

    def halves(self):
        """(D_eo, D_oe): borrowed views of the two half matrices, Sparse operators owned by this one."""
        out = []
        for which in (0, 1):
            h = C.c_void_p()
            check(_lib.lib().mgcr_eo_half_op(self.h, which, C.byref(h)))
            op = Operator()
            op.h = h
            op._keep.append(self)
            op.__class__ = _BorrowedOperator
            out.append(op)
        return tuple(out)

    def split(self, full, even=None, odd=None):
        _, ne, no = self.sizes()
        even = Field((ne,)) if even is None else even
        odd = Field((no,)) if odd is None else odd
        check(_lib.lib().mgcr_eo_split(self.h, full.h, even.h, odd.h))
        return even, odd

    def merge(self, even, odd, full=None):
        full = Field((self.sizes()[0],)) if full is None else full
        check(_lib.lib().mgcr_eo_merge(self.h, even.h, odd.h, full.h))
        return full

    def prepare(self, rhs_full, bhat_even=None):
        """bhat_e = b_e + k D_eo b_o"""
        bhat_even = Field((self.sizes()[1],)) if bhat_even is None else bhat_even
        check(_lib.lib().mgcr_eo_prepare(self.h, rhs_full.h, bhat_even.h))
        return bhat_even

    def reconstruct(self, rhs_full, x_even, x_full=None):
        """x_o = b_o + k D_oe x_e, merged with x_e"""
        x_full = Field(rhs_full.dims) if x_full is None else x_full
        check(_lib.lib().mgcr_eo_reconstruct(self.h, rhs_full.h, x_even.h, x_full.h))
        return x_full

    def solve(self, rhs_full, x_full, gcr_param):
        """(Id - k D) x_full = rhs_full through the Schur system; history, iteration count and flag are the Schur solve's
        (relative to |bhat_e|) and are kept in last_history / last_iterations / last_converged."""
        cap = max(gcr_param.max_iter, 1) + 1
        hist = np.zeros(cap, np.float64)
        it, conv = C.c_int32(), C.c_int32()
        pc = gcr_param._c()
        check(_lib.lib().mgcr_eo_solve(self.h, C.byref(pc), rhs_full.h, x_full.h, hist.ctypes.data, cap, C.byref(it), C.byref(conv)))
        self.last_iterations = it.value
        self.last_converged = bool(conv.value)
        self.last_history = hist[: it.value + 1].copy()
        return x_full

    def solve_queue(self, rhs_list, x_list, ks, gcr_param, width=8):
        """(Id - ks[s] D) x_s = rhs_s for any number of systems on full-system Fields, through `width` <= 16 columns of ONE batched
        solve of the Schur systems (mgcr_eo_solve_queue): a column whose system has stopped is reconstructed into its x Field and
        refilled with the next system at the next boundary of the restart cycle.  This operator's own k is neither used nor
        changed.  rhs Fields may repeat, the x Fields are distinct and updated in place; last_history (relative to |bhat_e,s|),
        last_iterations and last_converged are kept per system, each with the bits of solve() at ks[s] on that system alone."""
        nsys = len(rhs_list)
        if len(x_list) != nsys:
            raise MgcrError(1, "solve_queue: %d right-hand sides, %d x Fields" % (nsys, len(x_list)))
        kv = None
        if ks is not None:
            kv = MultiDiracOp._values(ks)
            if kv.shape[0] != nsys:
                raise MgcrError(1, "solve_queue: %d hopping parameters for %d systems" % (kv.shape[0], nsys))
        cap = max(gcr_param.max_iter, 1) + 1
        hist = np.zeros((max(nsys, 1), cap), np.float64)
        it, conv = (C.c_int32 * max(nsys, 1))(), (C.c_int32 * max(nsys, 1))()
        bh = (C.c_void_p * max(nsys, 1))(*[f.h if f is not None else None for f in rhs_list])
        xh = (C.c_void_p * max(nsys, 1))(*[f.h if f is not None else None for f in x_list])
        pc = gcr_param._c()
        check(_lib.lib().mgcr_eo_solve_queue(self.h, C.byref(pc), int(width), nsys, bh, xh,
                                             kv.ctypes.data_as(C.POINTER(C.c_double)) if kv is not None else None,
                                             hist.ctypes.data, cap, it, conv))
        self.last_iterations = [int(v) for v in it][:nsys]
        self.last_converged = [bool(v) for v in conv][:nsys]
        self.last_history = [hist[j, : it[j] + 1].copy() for j in range(nsys)]
        return x_list


class EvenOddDiagDiracOp(EvenOddDiracOp):
    """The even-odd preconditioned Id - k*D where D may store a SITE diagonal d (mgcr_eo_create_diag, Dirac form): with
    a = 1 - k d the operator on the even half is S = diag(a_e) - k^2 D_eo diag(1/a_o) D_oe, D_eo / D_oe the off-diagonal halves.
    Everything else is EvenOddDiracOp's: split / merge / prepare / reconstruct / solve / halves are inherited.  The scans
    (MultiEvenOddDiracOp, solve_queue) refuse an operator that carries a diagonal.  A matrix without any diagonal entry gives
    exactly EvenOddDiracOp(mat, k)."""

    _who = "EvenOddDiagDiracOp"

    def __init__(self, mat, k, parity=None):
        Operator.__init__(self)
        self._create(mat, _ri(k), parity)

    def _create(self, mat, k_ri, parity):
        _lib.init()
        n = int(mat._shape[0])
        if mat._shape[0] != mat._shape[1]:
            raise MgcrError(1, "%s: matrix must be square" % self._who)
        par = None if parity is None else np.ascontiguousarray(parity, np.int8)
        if par is not None and par.size != n:
            raise MgcrError(1, "%s: parity has %d entries, the matrix has %d rows" % (self._who, par.size, n))
        h = C.c_void_p()
        check(_lib.lib().mgcr_eo_create_diag(n, mat.ROW.ctypes.data, mat.COL.ctypes.data, mat.VAL.ctypes.data,
                                             par.ctypes.data if par is not None else None, k_ri, C.byref(h)))
        self.h = h
        self.last_history = None
        self.last_iterations = None
        self.last_converged = None

    def diag(self):
        """(a_even, 1 / a_odd): the two element-wise factors of the Schur apply as the device holds them"""
        _, ne, no = self.sizes()
        a, inv = np.empty(ne, c128), np.empty(no, c128)
        check(_lib.lib().mgcr_eo_diag(self.h, a.ctypes.data, inv.ctypes.data))
        return a, inv


class EvenOddSparse(EvenOddDiagDiracOp):
    """The even-odd preconditioned form of a matrix M ITSELF (mgcr_eo_create_diag, matrix form): M = diag(d) + offdiag, a Poisson
    matrix or a Wilson operator written with its mass term; S = diag(d_e) - M_eo diag(1/d_o) M_oe on the even half, and solve()
    solves M x_full = rhs_full.  There is no hopping parameter: set_k raises."""

    _who = "EvenOddSparse"

    def __init__(self, mat, parity=None):
        Operator.__init__(self)
        self._create(mat, None, parity)


class EvenOddBlockDiracOp(EvenOddDiracOp):
    """The even-odd preconditioned Id - k*D where D couples the bs consecutive rows of a SITE (mgcr_eo_create_block, Dirac form; a
    clover-type operator): with B_s = I - k D_ss the operator on the even half is S = B_e - k^2 D_eo B_o^-1 D_oe, D_eo / D_oe the
    inter-site halves.  Everything else is EvenOddDiracOp's: split / merge / prepare / reconstruct / solve / halves are inherited.
    The scans (MultiEvenOddDiracOp, solve_queue) refuse an operator with blocks.  bs = 1 gives exactly EvenOddDiagDiracOp(mat, k)."""

    _who = "EvenOddBlockDiracOp"

    def __init__(self, mat, k, bs, parity=None):
        Operator.__init__(self)
        self._create(mat, _ri(k), bs, parity)

    def _create(self, mat, k_ri, bs, parity):
        _lib.init()
        n = int(mat._shape[0])
        if mat._shape[0] != mat._shape[1]:
            raise MgcrError(1, "%s: matrix must be square" % self._who)
        par = None if parity is None else np.ascontiguousarray(parity, np.int8)
        if par is not None and par.size != n:
            raise MgcrError(1, "%s: parity has %d entries, the matrix has %d rows" % (self._who, par.size, n))
        h = C.c_void_p()
        check(_lib.lib().mgcr_eo_create_block(n, mat.ROW.ctypes.data, mat.COL.ctypes.data, mat.VAL.ctypes.data, int(bs),
                                              par.ctypes.data if par is not None else None, k_ri, C.byref(h)))
        self.h = h
        self.last_history = None
        self.last_iterations = None
        self.last_converged = None

    def block_info(self):
        """(bs, number of even sites, number of odd sites)"""
        bs, se, so = C.c_int32(), C.c_int64(), C.c_int64()
        check(_lib.lib().mgcr_eo_block_info(self.h, C.byref(bs), C.byref(se), C.byref(so)))
        return bs.value, se.value, so.value

    def block_diag(self):
        """(B_even[sites_e, bs, bs], invB_odd[sites_o, bs, bs]): the two block factors of the Schur apply as the device holds them"""
        bs, se, so = self.block_info()
        B, inv = np.empty((se, bs, bs), c128), np.empty((so, bs, bs), c128)
        check(_lib.lib().mgcr_eo_block_diag(self.h, B.ctypes.data, inv.ctypes.data))
        return B, inv


class EvenOddBlockSparse(EvenOddBlockDiracOp):
    """The even-odd preconditioned form of a matrix M ITSELF whose diagonal is a dense block per site of bs consecutive rows
    (mgcr_eo_create_block, matrix form): S = M_ee - M_eo M_oo^-1 M_oe on the even half, and solve() solves M x_full = rhs_full.
    There is no hopping parameter: set_k raises."""

    _who = "EvenOddBlockSparse"

    def __init__(self, mat, bs, parity=None):
        Operator.__init__(self)
        self._create(mat, None, bs, parity)


class MultiEvenOddDiracOp(Operator):
    """The Schur complements Id - ks[j]^2 D_eo D_oe of ONE hopping matrix on column j of a block of len(ks) Fields of the even
    half: an even-odd hopping-parameter scan as one operator (mgcr_eo_multi_create; no reference counterpart).  Borrows the halves
    and index lists of `eo`, an EvenOddDiracOp, and keeps it alive; eo's own k is not used.  apply_multi, GCR(...).solve_multi and
    the methods below take it, with MultiFields of exactly ncols columns; column j has the bits of EvenOddDiracOp(D, ks[j]) on
    that column alone."""

    def __init__(self, eo, ks):
        super().__init__()
        kv = MultiDiracOp._values(ks)
        h = C.c_void_p()
        check(_lib.lib().mgcr_eo_multi_create(eo.h, kv.shape[0], kv.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h)))
        self.h = h
        self.ncols = int(kv.shape[0])
        self.eo = eo
        self._keep.append(eo)
        self.last_history = None
        self.last_iterations = None
        self.last_converged = None

    def set_k(self, ks):
        """Replace all ncols values; takes effect for every later call, never for work already enqueued."""
        kv = MultiDiracOp._values(ks)
        if kv.shape[0] != self.ncols:
            raise MgcrError(1, "MultiEvenOddDiracOp.set_k: %d values for %d columns" % (kv.shape[0], self.ncols))
        check(_lib.lib().mgcr_eo_multi_set_k(self.h, kv.ctypes.data_as(C.POINTER(C.c_double))))

    def sizes(self):
        """(n, n_even, n_odd)"""
        return self.eo.sizes()

    def split(self, full, even=None, odd=None):
        _, ne, no = self.sizes()
        even = MultiField((ne,), self.ncols) if even is None else even
        odd = MultiField((no,), self.ncols) if odd is None else odd
        check(_lib.lib().mgcr_eo_multi_split(self.h, full.h, even.h, odd.h))
        return even, odd

    def merge(self, even, odd, full=None):
        full = MultiField((self.sizes()[0],), self.ncols) if full is None else full
        check(_lib.lib().mgcr_eo_multi_merge(self.h, even.h, odd.h, full.h))
        return full

    def prepare(self, rhs_full, bhat_even=None):
        """bhat_e,j = b_e,j + ks[j] D_eo b_o,j"""
        bhat_even = MultiField((self.sizes()[1],), self.ncols) if bhat_even is None else bhat_even
        check(_lib.lib().mgcr_eo_multi_prepare(self.h, rhs_full.h, bhat_even.h))
        return bhat_even

    def reconstruct(self, rhs_full, x_even, x_full=None):
        """x_o,j = b_o,j + ks[j] D_oe x_e,j, merged with x_e,j"""
        x_full = MultiField(rhs_full.dims, self.ncols) if x_full is None else x_full
        check(_lib.lib().mgcr_eo_multi_reconstruct(self.h, rhs_full.h, x_even.h, x_full.h))
        return x_full

    def solve(self, RHS_full, X_full, gcr_param):
        """(Id - ks[j] D) x_full,j = rhs_full,j for every column through ONE batched solve of the Schur systems; histories (relative
        to |bhat_e,j|), iteration counts and flags are kept per column in last_history / last_iterations / last_converged."""
        k = self.ncols
        cap = max(gcr_param.max_iter, 1) + 1
        hist = np.zeros((k, cap), np.float64)
        it, conv = (C.c_int32 * k)(), (C.c_int32 * k)()
        pc = gcr_param._c()
        check(_lib.lib().mgcr_eo_multi_solve(self.h, C.byref(pc), RHS_full.h, X_full.h, hist.ctypes.data, cap, it, conv))
        self.last_iterations = [int(v) for v in it]
        self.last_converged = [bool(v) for v in conv]
        self.last_history = [hist[j, : it[j] + 1].copy() for j in range(k)]
        return X_full


class HierarchicalSparse(Operator):
    """HierarchicalSparse<long,int> (src/HierarchicalSparse.h:22-48) from unsorted
    (block_row, block_col, dense block) triplets, duplicates kept (ctor :58-98)."""

    def __init__(self, block_rows, block_cols, rows, cols, blocks):
        super().__init__()
        _lib.init()
        rows = np.ascontiguousarray(rows, np.int32)
        cols = np.ascontiguousarray(cols, np.int32)
        blocks = np.ascontiguousarray(blocks, c128)
        nt = rows.size
        bs = int(round(np.sqrt(blocks.size // max(nt, 1))))
        if nt == 0 or bs * bs * nt != blocks.size:
            raise MgcrError(1, "blocks must hold ntriplets square blocks")
        h = C.c_void_p()
        check(_lib.lib().mgcr_bcsr_create_from_triplets(block_rows, block_cols, bs, nt, rows.ctypes.data,
                                                        cols.ctypes.data, blocks.ctypes.data, C.byref(h)))
        self.h = h
        self.bs = bs


class Dense(HierarchicalSparse):
    """Dense<num_type>(matrix, dim) (src/Operator.h:125-129,159-173): row-major dim x dim complex matrix; its
    operator() accumulates each row in column order.  Stored as a block-CSR operator of one block."""

    def __init__(self, matrix, dim=None):
        m = np.ascontiguousarray(matrix, c128)
        dim = int(dim) if dim is not None else int(round(np.sqrt(m.size)))
        if dim * dim != m.size:
            raise MgcrError(1, "Dense: matrix must hold dim*dim entries")
        super().__init__(1, 1, [0], [0], m.reshape(1, dim, dim))
        self.mat = m.reshape(dim, dim).copy()

    def val_at(self, row, col=None):  # src/Operator.h:45-46
        return complex(self.mat.reshape(-1)[row] if col is None else self.mat[row, col])

    # set-up-time algebra (src/Operator.h:139-190), on the host like the reference's
    def __add__(self, other):
        from . import hostalg
        return Dense(hostalg.dense_add(self.mat, other.mat))

    def __mul__(self, other):
        from . import hostalg
        return Dense(hostalg.dense_mul(self.mat, other.mat))

    def dagger(self):
        from . import hostalg
        return Dense(hostalg.dense_dagger(self.mat))


_BLOCK_ONLY = (MultiDiracOp, MultiEvenOddDiracOp)   # operators of the block entry points only


class GCR_Param:
    """GCR_Param(trunc, re, max_it, tau, verb, solver_l, solver_r) (src/SolverParam.h:21-35,85-99)."""

    def __init__(self, trunc=0, re=0, max_it=100, tau=1e-16, verb=True, solver_l=None, solver_r=None,
                 use_x0=False, flexible=False, check_every=0, profile_spmv=False):
        self.truncation, self.restart, self.max_iter, self.tol = int(trunc), int(re), int(max_it), float(tau)
        self.verbose = bool(verb)
        self.left_precond, self.right_precond = solver_l, solver_r
        self.use_x0, self.flexible, self.check_every = bool(use_x0), bool(flexible), int(check_every)
        self.profile_spmv = bool(profile_spmv)

    def _c(self):
        return GcrParamC(self.truncation, self.restart, self.max_iter, self.tol, int(self.verbose),
                         self.left_precond.h if self.left_precond is not None else None,
                         self.right_precond.h if self.right_precond is not None else None,
                         int(self.use_x0), int(self.flexible), self.check_every, int(self.profile_spmv))


class GCR(Operator):
    """GCR<num_type> (src/GCR.h:18-50): `GCR(M, param)` or `GCR(param)` + `initialise(M)`."""

    def __init__(self, M=None, gcr_param=None, x0_mode=1):
        super().__init__()
        if isinstance(M, GCR_Param) and gcr_param is None:  # GCR(GCR_Param*) src/GCR.h:30
            M, gcr_param = None, M
        _lib.init()
        self.param = gcr_param
        self.A = M
        h = C.c_void_p()
        pc = gcr_param._c()
        # (a MultiDiracOp or MultiEvenOddDiracOp serves solve_multi only, which takes the operator from self.A: the single-Field
        # solver object is made without one, and solve / operator() answer as the C entry points do)
        single = M is not None and not isinstance(M, _BLOCK_ONLY)
        check(_lib.lib().mgcr_gcr_create(M.h if single else None, C.byref(pc), x0_mode, C.byref(h)))
        self.h = h
        self._keep += [M, gcr_param, gcr_param.left_precond, gcr_param.right_precond]
        self.last_history = None
        self.last_iterations = None
        self.last_converged = None

    def initialise(self, M):  # src/GCR.h:31
        self.A = M
        self._keep.append(M)
        if not isinstance(M, _BLOCK_ONLY):
            check(_lib.lib().mgcr_gcr_set_operator(self.h, M.h))

    def _single_field_only(self, who):
        if isinstance(self.A, _BLOCK_ONLY):
            raise MgcrError(7, "%s: a %s has one hopping parameter per column of a block; use solve_multi" % (who, type(self.A).__name__))

    def __call__(self, f, out=None):
        self._single_field_only("GCR as an operator")
        return super().__call__(f, out)

    def set_x0(self, x0):
        check(_lib.lib().mgcr_gcr_set_x0(self.h, x0.h if x0 is not None else None))

    def solve(self, rhs, x):
        """void solve(const Field& rhs, Field& x) (src/GCR.h:158-302). x is updated in place;
        the residual history / iteration count are kept in last_history / last_iterations."""
        self._single_field_only("GCR.solve")
        cap = max(self.param.max_iter, 1) + 1
        hist = np.zeros(cap, np.float64)
        it, conv = C.c_int32(), C.c_int32()
        pc = self.param._c()  # the reference reads its GCR_Param* at solve time: refresh, keep the work vectors
        check(_lib.lib().mgcr_gcr_set_param(self.h, C.byref(pc)))
        check(_lib.lib().mgcr_gcr_solve_op(self.h, rhs.h, x.h, hist.ctypes.data, cap, C.byref(it), C.byref(conv)))
        self.last_iterations = it.value
        self.last_converged = bool(conv.value)
        self.last_history = hist[: it.value + 1].copy()
        return x

    def solve_multi(self, RHS, X):
        """k independent solves A x_j = rhs_j in lockstep (mgcr_gcr_solve_multi; restart mode).  Unpreconditioned, or — the flexible
        batched GCR — with GCR_Param(..., solver_r=M, flexible=True): M a LowPrecisionGCR of the square form, which runs as the k-wide
        lockstep inner solve, or an operator that apply_multi takes (Sparse, DiracOp, HierarchicalSparse), applied k-wide to the
        residual block.  Column j has the bits of solve() on column j alone with the same M in the slot (Rule F of include/mgcr.h).
        X is updated in place; last_history (k arrays), last_iterations and last_converged (lists) are kept per column."""
        if self.A is None:
            raise MgcrError(1, "GCR has no operator (call initialise first)")
        k = RHS.k
        if self.param.right_precond is not None and not any(o is self.param.right_precond for o in self._keep):
            self._keep.append(self.param.right_precond)   # (a preconditioner set on the param after construction lives as long as the solver)
        cap = max(self.param.max_iter, 1) + 1
        hist = np.zeros((k, cap), np.float64)
        it, conv = (C.c_int32 * k)(), (C.c_int32 * k)()
        pc = self.param._c()
        check(_lib.lib().mgcr_gcr_solve_multi(self.A.h, C.byref(pc), RHS.h, X.h, hist.ctypes.data, cap, it, conv))
        if isinstance(self.param.right_precond, LowPrecisionGCR):
            self.param.right_precond._last_k = k   # last_multi() of the preconditioner: the k-wide inner solve this solve enqueued last
        self.last_iterations = [int(v) for v in it]
        self.last_converged = [bool(v) for v in conv]
        self.last_history = [hist[j, : it[j] + 1].copy() for j in range(k)]
        return X

    def solve_queue(self, rhs_list, x_list, width=8, ks=None):
        """len(rhs_list) independent systems (any number) through `width` <= 16 slots of one batched solve (mgcr_gcr_solve_queue):
        a slot whose system has stopped is refilled with the next one at the next boundary of the restart cycle.  System s is
        A x_s = rhs_s with A the operator of this GCR, or — ks given, A the Sparse D — (1 - ks[s] D) x_s = rhs_s.  rhs Fields may
        repeat, the x Fields are distinct and updated in place; last_history, last_iterations and last_converged are kept per
        system, each with the bits of solve() on that system alone."""
        if self.A is None:
            raise MgcrError(1, "GCR has no operator (call initialise first)")
        nsys = len(rhs_list)
        if len(x_list) != nsys:
            raise MgcrError(1, "solve_queue: %d right-hand sides, %d x Fields" % (nsys, len(x_list)))
        kv = None
        if ks is not None:
            kv = MultiDiracOp._values(ks)
            if kv.shape[0] != nsys:
                raise MgcrError(1, "solve_queue: %d hopping parameters for %d systems" % (kv.shape[0], nsys))
        cap = max(self.param.max_iter, 1) + 1
        hist = np.zeros((max(nsys, 1), cap), np.float64)
        it, conv = (C.c_int32 * max(nsys, 1))(), (C.c_int32 * max(nsys, 1))()
        bh = (C.c_void_p * max(nsys, 1))(*[f.h for f in rhs_list])
        xh = (C.c_void_p * max(nsys, 1))(*[f.h for f in x_list])
        pc = self.param._c()
        check(_lib.lib().mgcr_gcr_solve_queue(self.A.h, C.byref(pc), int(width), nsys, bh, xh,
                                              kv.ctypes.data_as(C.POINTER(C.c_double)) if kv is not None else None,
                                              hist.ctypes.data, cap, it, conv))
        self.last_iterations = [int(v) for v in it][:nsys]
        self.last_converged = [bool(v) for v in conv][:nsys]
        self.last_history = [hist[j, : it[j] + 1].copy() for j in range(nsys)]
        return x_list


class LowPrecisionGCR(Operator):
    """Mixed precision: an fp32 copy of `mat` (a Sparse; its host arrays ROW, COL, VAL are used) and a restarted GCR that runs in
    fp32 on the device, from x0 = 0, without host round trips (mgcr_gcr32_create).  k given: A = 1 - k D (Dirac form); k None: A = the
    matrix.  gcr_param: restart (1 .. 16), max_it (steps enqueued per apply), tau (relative tolerance).  operator()(f) returns
    y ~ A^-1 f; its place is GCR_Param(solver_r=..., flexible=True) of an fp64 solve."""

    def __init__(self, mat, k=None, gcr_param=None):
        super().__init__()
        _lib.init()
        if gcr_param is None:
            gcr_param = GCR_Param(0, 8, 8, 0.1, False)
        self.param = gcr_param
        self.k = None if k is None else complex(k)
        h = C.c_void_p()
        pc = gcr_param._c()
        n = int(mat.ROW.size - 1)
        check(_lib.lib().mgcr_gcr32_create(n, mat.ROW.ctypes.data, mat.COL.ctypes.data, mat.VAL.ctypes.data,
                                           _ri(k) if k is not None else None, C.byref(pc), C.byref(h)))
        self.h = h

    def set_k(self, k):
        check(_lib.lib().mgcr_gcr32_set_k(self.h, _ri(k)))
        self.k = complex(k)

    def set_param(self, gcr_param):
        pc = gcr_param._c()
        check(_lib.lib().mgcr_gcr32_set_param(self.h, C.byref(pc)))
        self.param = gcr_param

    def apply_matrix(self, x, out=None):
        """y = fp64(A32 fp32(x)): one matrix apply in fp32 (the test hook of the arithmetic)."""
        if out is None:
            out = Field(x.dims)
        check(_lib.lib().mgcr_gcr32_apply_matrix(self.h, x.h, out.h))
        return out

    def last(self):
        """(steps the last apply performed, its last fp32 |r| / |f|): one synchronisation."""
        it, rel = C.c_int32(), C.c_double()
        check(_lib.lib().mgcr_gcr32_last(self.h, C.byref(it), C.byref(rel)))
        return it.value, rel.value

    def info(self):
        n, w, t, real, b = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_int64()
        check(_lib.lib().mgcr_gcr32_info(self.h, C.byref(n), C.byref(w), C.byref(t), C.byref(real), C.byref(b)))
        return dict(n=n.value, ell_width=w.value, tail_rows=t.value, real_slab=bool(real.value), stored_bytes=b.value)

    # ---- blocks of k Fields: the k inner solves in lockstep, and fp64 defect correction around them (mgcr_gcr32_apply_multi) ----
    def inner_multi(self, F, Y=None, active=None):
        """Y_j ~ A^-1 F_j for the k columns of the MultiField F, the k fp32 inner solves advancing in lockstep; column j has the bits
        of self(F.column(j)) (Rule M1).  active: an iterable of k truth values, or a bit mask — a column that is not active performs 0
        steps and gets y = 0; None: every column."""
        if Y is None:
            Y = MultiField.like(F)
        if active is None:
            mask = (1 << F.k) - 1
        elif isinstance(active, (int, np.integer)):
            mask = int(active)
        else:
            mask = sum(1 << j for j, a in enumerate(active) if a)
        if mask < 0 or mask >> 32:
            raise MgcrError(1, "LowPrecisionGCR.inner_multi: active = %r is not a mask of at most 16 columns" % (active,))
        check(_lib.lib().mgcr_gcr32_apply_multi(self.h, F.h, Y.h, mask))
        self._last_k = F.k
        return Y

    def last_multi(self):
        """[(steps, last fp32 |r| / |f|)] per column of the last batched inner solve that was enqueued, by inner_multi or by
        solve_multi (a solve in which no column was ever active enqueues none): one synchronisation."""
        it, rel = (C.c_int32 * 16)(), (C.c_double * 16)()
        check(_lib.lib().mgcr_gcr32_last_multi(self.h, it, rel))
        return [(int(it[j]), float(rel[j])) for j in range(getattr(self, "_last_k", 0))]

    def solve_multi(self, A, B, X, tol=1e-10, max_outer=50, use_x0=False):
        """The batched mixed solve A X = B: fp64 defect correction, R = B - A X, X += inner_multi(R), on the columns that have not
        converged (mgcr_gcr32_solve_multi; column j has the bits of the same loop on column j alone, Rule M2).  Sets last_history
        (one array of |r| / |b| per column), last_iterations and last_converged (lists)."""
        k = B.k
        cap = int(max_outer) + 1 if max_outer >= 0 else 1
        hist = np.zeros((k, cap), np.float64)
        it, conv = (C.c_int32 * k)(), (C.c_int32 * k)()
        check(_lib.lib().mgcr_gcr32_solve_multi(A.h, self.h, float(tol), int(max_outer), 1 if use_x0 else 0, B.h, X.h,
                                                hist.ctypes.data_as(C.POINTER(C.c_double)), cap, it, conv))
        self.last_iterations = [int(v) for v in it]
        if max(self.last_iterations) > 0:
            self._last_k = k
        self.last_converged = [bool(v) for v in conv]
        self.last_history = [hist[j, : it[j] + 1].copy() for j in range(k)]
        return X


class LowPrecisionEvenOddGCR(LowPrecisionGCR):
    """Mixed precision on the even-odd Schur system: an fp32 copy of S = diag(a_e) - c^2 H_eo diag(1/a_o) H_oe of `mat` (a Sparse that
    may store a site diagonal) and LowPrecisionGCR's inner solve on its n_e rows (mgcr_gcr32_create_eo).  k given: Dirac form, the
    operator of EvenOddDiracOp / EvenOddDiagDiracOp; k None: matrix form, EvenOddSparse.  parity as theirs.  Its place is
    GCR_Param(solver_r=..., flexible=True) of EvenOddDiracOp.solve or of a GCR on such an operator made from the same matrix and
    parity.  set_k, set_param, apply_matrix and last are inherited."""

    def __init__(self, mat, k=None, gcr_param=None, parity=None):
        Operator.__init__(self)
        _lib.init()
        if gcr_param is None:
            gcr_param = GCR_Param(0, 8, 8, 0.1, False)
        self.param = gcr_param
        self.k = None if k is None else complex(k)
        n = int(mat.ROW.size - 1)
        par = None if parity is None else np.ascontiguousarray(parity, np.int8)
        if par is not None and par.size != n:
            raise MgcrError(1, "LowPrecisionEvenOddGCR: parity has %d entries, the matrix has %d rows" % (par.size, n))
        h = C.c_void_p()
        pc = gcr_param._c()
        check(_lib.lib().mgcr_gcr32_create_eo(n, mat.ROW.ctypes.data, mat.COL.ctypes.data, mat.VAL.ctypes.data,
                                              par.ctypes.data if par is not None else None, _ri(k) if k is not None else None,
                                              C.byref(pc), C.byref(h)))
        self.h = h

    def info(self):
        n, ne, no, b, t0, t1 = (C.c_int64() for _ in range(6))
        w0, w1, real, diag = (C.c_int32() for _ in range(4))
        check(_lib.lib().mgcr_gcr32_eo_info(self.h, C.byref(n), C.byref(ne), C.byref(no), C.byref(w0), C.byref(w1), C.byref(t0), C.byref(t1),
                                            C.byref(real), C.byref(diag), C.byref(b)))
        return dict(n=n.value, n_even=ne.value, n_odd=no.value, width_eo=w0.value, width_oe=w1.value, tail_rows_eo=t0.value,
                    tail_rows_oe=t1.value, real_slab=bool(real.value), has_diag=bool(diag.value), stored_bytes=b.value)

    def sizes(self):
        """(n, n_even, n_odd)"""
        i = self.info()
        return i["n"], i["n_even"], i["n_odd"]

    def diag(self):
        """(a_even, 1 / a_odd) in complex64, as the device holds them"""
        _, ne, no = self.sizes()
        a, inv = np.empty(ne, np.complex64), np.empty(no, np.complex64)
        check(_lib.lib().mgcr_gcr32_eo_diag(self.h, a.ctypes.data, inv.ctypes.data))
        return a, inv


def legacy_dense_gcr(matrix, rhs, x, tol, max_iter, truncation, verbose=True):
    """GCR(matrix, dimension).solve(rhs, x, tol, max_iter, truncation) — the reference's legacy raw-pointer dense solve
    (src/GCR.h:70-156): r0 = rhs - A x (x0 honoured), directions truncated to the last `truncation`, stops when
    |r|^2 <= tol — absolute, tested BEFORE every step, so possibly after none — or after max_iter steps.  On the device:
    the Dense operator, GCR in truncation mode with use_x0; sqrt(tol) / |rhs| as relative tolerance is the same test.
    Returns (x, absolute residual norms per step) and prints the reference's lines when verbose."""
    A = Dense(matrix)
    d = A.mat.shape[0]
    b = Field((d,), rhs)
    xf = Field((d,), x)
    r0 = b - A(xf)
    bn2, rr = b.squarednorm(), r0.squarednorm()
    norms = np.zeros(0)
    if rr > tol and max_iter > 0 and bn2 > 0.:
        g = GCR(A, GCR_Param(int(truncation), 0, int(max_iter), float(np.sqrt(tol) / np.sqrt(bn2)), False, use_x0=True))
        g.solve(b, xf)
        norms = g.last_history[1:] * np.sqrt(bn2)
        rr = float(norms[-1] ** 2)
    elif rr > tol and max_iter > 0:
        # rhs = 0 with x0 != 0: the reference iterates on r0 = -A x0 and drives x towards 0 (its test is absolute).  The Field
        # solve's test is relative to its right-hand side, so hand it r0 AS the right-hand side (r = rhs there whatever x is,
        # src/GCR.h:189) and let it update x0 in place: the same recurrence, tolerance sqrt(tol) / |r0|
        g = GCR(A, GCR_Param(int(truncation), 0, int(max_iter), float(np.sqrt(tol) / np.sqrt(rr)), False))
        rn = np.sqrt(rr)
        g.solve(r0, xf)
        norms = g.last_history[1:] * rn
        rr = float(norms[-1] ** 2)
    if verbose:
        for k, v in enumerate(norms):
            print("Step %d residual norm = %.10e" % (k + 1, v))
        if norms.size == max_iter:
            print("GCR did not converge after %d steps! Residual norm = %.10e" % (max_iter, rr))
    return xf.to_numpy(), norms


class Mesh:
    """Mesh<num_type> (src/Mesh.h:13-64): row-major N-D index algebra (host side)."""

    def __init__(self, index_dims, num_dims=None):
        self.dims = tuple(int(d) for d in (index_dims[:num_dims] if num_dims else index_dims))

    def get_ndim(self):
        return len(self.dims)

    def get_size(self):
        return int(np.prod(self.dims, dtype=np.int64))

    def ind_loc(self, index):  # src/Mesh.h:156-165
        loc = int(index[0])
        for i in range(1, len(self.dims)):
            loc = loc * self.dims[i] + int(index[i])
        return loc

    def loc_ind(self, loc):  # alloc_loc_ind src/Mesh.h:368-398
        return tuple(int(v) for v in np.unravel_index(loc, self.dims))

    # ---- aggregates (src/Mesh.h:236-324): the reference's 4 blocked ("spacetime") dimensions --------------
    def blocking(self, subblock_dim, blocked_dimensions):
        """Mesh::blocking (src/Mesh.h:236-298): block_map[block][offset] = location of a site in the row-major
        spacetime lattice (the blocked dimensions only), blocks and in-block offsets row-major as well.  Integer
        index algebra on the host, as in the reference; the device set-up (csrc/mg_setup.hip:agg_kernel) forms
        the same aggregates directly from the row index (tests/test_gpu_mg.py::test_mesh_blocking_matches_device_aggregates)."""
        blocked = [bool(b) for b in blocked_dimensions][:len(self.dims)]
        idx = [d for d, b in enumerate(blocked) if b]
        if len(idx) != 4:
            raise ValueError("Mesh::blocking blocks exactly 4 dimensions (got %d)" % len(idx))
        sub = int(subblock_dim)
        st_dims = [self.dims[d] for d in idx]
        if any(v % sub for v in st_dims):
            raise ValueError("Dimension not exactly divisible by block size!")
        self.sub_dim = sub
        self.blocked_ind = idx
        self.block_dim = [v // sub for v in st_dims]
        coords = np.indices(st_dims).reshape(4, -1)                      # x, y, z, w of every site, row-major
        loc = np.ravel_multi_index(tuple(coords), st_dims)
        block = np.ravel_multi_index(tuple(coords // sub), self.block_dim)
        off = np.ravel_multi_index(tuple(coords % sub), [sub] * 4)
        self.block_map = np.empty((self.get_nblocks(), self.get_block_size()), np.int64)
        self.block_map[block, off] = loc
        return self

    def get_nblocks(self):
        return int(np.prod(self.block_dim))

    def get_block_dim(self):
        return list(self.block_dim)

    def get_block_size(self):
        return self.sub_dim ** 4

    def get_block_map(self, block_idx):
        return self.block_map[int(block_idx)]

    def alloc_full_index(self, spacetime_loc, spinor, colour, spacetime_dimensions, spinor_dimension):
        """Mesh::alloc_full_index (src/Mesh.h:300-324): spacetime location + spinor + colour -> N-D index."""
        st_dims = [self.dims[d] for d in range(len(self.dims)) if spacetime_dimensions[d]]
        st = np.unravel_index(int(spacetime_loc), st_dims)
        out, c = [], 0
        for d in range(len(self.dims)):
            if spacetime_dimensions[d]:
                out.append(int(st[c]))
                c += 1
            elif spinor_dimension[d]:
                out.append(int(spinor))
            else:
                out.append(int(colour))
        return tuple(out)


def gamma5(field_values, dims, spinor_index=4):
    """Field::gamma5 (src/Fields.h:310-339) of host values: output[index with spinor 0<->2, 1<->3] = field[i]
    (computed on the device: Field.gamma5)."""
    return Field(tuple(dims), np.asarray(field_values, c128).reshape(-1)).gamma5(spinor_index).to_numpy()


def _vec_double_fields(fields, spinor_index):
    plus, minus = [], []
    for v in fields:
        g = v.gamma5(spinor_index)
        plus.append((v + g) * 0.5)
        minus.append((v - g) * 0.5)
    return plus + minus


def vec_double(vecs, dims, spinor_index=4):
    """MG::vec_double (src/MG.h:316-345): [v+ ..., v- ...] with v+- = (v +- gamma5 v) * 0.5, on the device."""
    fields = [Field(tuple(dims), np.asarray(v, c128).reshape(-1)) for v in vecs]
    return np.array([f.to_numpy() for f in _vec_double_fields(fields, spinor_index)])


class MG_Param:
    """MG_Param(mesh, subblock, eigenvecs, eigen_param, solver_coarse, solver_smooth, levels,
    solver_l, solver_r) (src/SolverParam.h:38-59,142-158).

    solver_coarse / solver_smooth are GCR objects created with `GCR(GCR_Param)` exactly as in the
    reference (src/main.cpp:851-853); MG takes their GCR_Param.  Extras the reference lacks:
    `null_vectors` (use these near-null vectors instead of computing n_eigen of them),
    `spacetime` mask for meshes that are not 6-D, `damping` (reference literal: 0.1), `coarse_direct` (solve a
    coarsest level of at most that many unknowns directly instead of by solver_coarse; 0 = never, like the reference)."""

    def __init__(self, m, subblock, eigenvecs, eigen_param, solver_coarse, solver_smooth, levels=1,
                 solver_l=None, solver_r=None, spacetime=None, spinor=None, null_vectors=None, damping=1.0, coarse_direct=0):
        self.mesh = m if isinstance(m, Mesh) else Mesh(m)
        self.subblock_dim = int(subblock)
        self.n_eigen = int(eigenvecs)
        self.eigenvector_precomp_param = eigen_param
        self.coarse_solver, self.smoother_solver = solver_coarse, solver_smooth
        nd = self.mesh.get_ndim()
        default_st = [True, True, True, True, False, False]
        self.spacetime = list(spacetime) if spacetime is not None else (default_st[:nd] if nd == 6 else [True] * nd)
        self.spinor = list(spinor) if spinor is not None else ([False] * 4 + [True, False] if nd == 6 else [False] * nd)
        self.n_level = int(levels)
        self.left_precond, self.right_precond = solver_l, solver_r
        self.null_vectors = null_vectors
        self.damping = float(damping)
        self.coarse_direct = int(coarse_direct)   # > 0: a coarsest level of at most this many unknowns (<= 2048) is inverted at set-up


class MG(Operator):
    """MG<num_type> (src/MG.h:20-61): `MG(M, param)` or `MG(param)` + `initialise(M)`.

    apply = corrected V-cycle; restrict / expand as in src/MG.h:347-383."""

    def __init__(self, M=None, parameter=None):
        super().__init__()
        if isinstance(M, MG_Param) and parameter is None:
            M, parameter = None, M
        self.param = parameter
        self.m = None
        if M is not None:
            self.initialise(M)

    def near_null_vectors(self, M, start=None, alias_rhs_x=True, double=True):
        """Arnoldi::solve (src/MG.h:90-122): inverse iteration with GCR for the smallest modes,
        Gram-Schmidt between them, then chirality doubling when the mesh has a spinor dimension.
        The start vector is the repo's deterministic RHS (seed 9) instead of libc rand() unless `start` is given (the
        reference's is init_rand(9)).  `alias_rhs_x` (default, the reference's literal first loop): gcr.solve(b, b) —
        rhs and x are ONE Field, i.e. x0 = b while r0 = b (src/GCR.h:189), so each of the ten steps is
        b <- normalise(b + GCR(b)); False: each solve starts from x0 = 0, b <- normalise(GCR(b)).
        The later vectors are solved from x0 = 0 either way: the reference solves
        them into a malloc'ed, never initialised Field (src/MG.h:110, src/Fields.h:97-101), which has no defined value
        (tests/test_gpu_mg.py::test_arnoldi_vs_reference)."""
        prm = self.param
        dims = prm.mesh.dims
        gp = prm.eigenvector_precomp_param
        gcr = GCR(M, GCR_Param(gp.truncation, gp.restart, gp.max_iter, gp.tol, False))
        comm = getattr(M, "comm", None)   # distributed operator: dot products and norms are global

        def gdot(a, b_):
            return comm.dot(a, b_) if comm is not None else a.dot(b_)

        def gnormalise(f):
            return f * (1.0 / np.sqrt(gdot(f, f).real)) if comm is not None else f.normalise()

        b = Field(dims).fill_rhs(9, global_offset=getattr(M, "row0", 0)) if start is None else Field(dims, start)
        x = Field(dims)
        for _ in range(10):
            if alias_rhs_x:
                x.assign(b)
            else:
                x.set_zero()
            gcr.solve(b, x)
            b = gnormalise(b.assign(x))
        vecs = [b.copy()]
        for count in range(1, prm.n_eigen):
            x.set_zero()
            gcr.solve(vecs[-1], x)
            t = x.copy()
            for v in vecs:       # Gram-Schmidt against the vectors found so far (src/MG.h:112-118), Field algebra on the device
                t = t - v * gdot(v, t)
            vecs.append(gnormalise(t))
        if double and any(prm.spinor):
            vecs = _vec_double_fields(vecs, prm.spinor.index(True))
        return np.array([v.to_numpy() for v in vecs])

    def initialise(self, M):  # src/MG.h:131-285
        _lib.init()
        prm = self.param
        self.m = M
        vecs = prm.null_vectors if prm.null_vectors is not None else self.near_null_vectors(M)
        vecs = np.ascontiguousarray(vecs, c128)
        if vecs.ndim == 1:
            vecs = vecs[None, :]
        nd = prm.mesh.get_ndim()
        pc = MgParamC()
        pc.ndim = nd
        for d in range(nd):
            pc.dims[d] = prm.mesh.dims[d]
            pc.blocked[d] = int(bool(prm.spacetime[d]))
        pc.subblock_dim = prm.subblock_dim
        pc.n_vec = vecs.shape[0]
        pc.vecs_ri = vecs.ctypes.data
        pc.n_level = prm.n_level
        pc.smoother = prm.smoother_solver.param._c()
        pc.coarse = prm.coarse_solver.param._c()
        pc.damping = prm.damping
        pc.coarse_direct_rows = prm.coarse_direct
        h = C.c_void_p()
        check(_lib.lib().mgcr_mg_create(M.h, C.byref(pc), C.byref(h)))
        if self.h:
            _lib.lib().mgcr_op_destroy(self.h)
        self.h = h
        self._keep += [M, prm]
        self.n_levels = prm.n_level + 1

    def level_info(self, level):
        dim, ne, nagg = C.c_int64(), C.c_int32(), C.c_int64()
        check(_lib.lib().mgcr_mg_level_info(self.h, level, C.byref(dim), C.byref(ne), C.byref(nagg)))
        return dict(dim=dim.value, ne=ne.value, nagg=nagg.value)

    def restrict(self, x_fine, level=0):  # src/MG.h:366-383
        out = Field((self.level_info(level + 1)["dim"],))
        check(_lib.lib().mgcr_mg_restrict(self.h, level, x_fine.h, out.h))
        return out

    def expand(self, x_coarse, level=0):  # src/MG.h:347-364
        info = self.level_info(level)
        out = Field(self.param.mesh.dims if level == 0 else (info["dim"],))
        check(_lib.lib().mgcr_mg_expand(self.h, level, x_coarse.h, out.h))
        return out

    def level_operator(self, level):
        """Borrowed view of the level's operator (level >= 1: the Galerkin m_coarse, src/MG.h:281)."""
        h = C.c_void_p()
        check(_lib.lib().mgcr_mg_level_op(self.h, level, C.byref(h)))
        op = Operator()
        op.h = h
        op._keep.append(self)
        op.__class__ = _BorrowedOperator
        return op

    def prolongator(self, level=0):
        info = self.level_info(level)
        pv = np.empty((info["dim"], info["ne"]), c128)
        agg = np.empty(info["dim"], np.int32)
        check(_lib.lib().mgcr_mg_download_prolongator(self.h, level, pv.ctypes.data, agg.ctypes.data))
        return pv, agg


class _BorrowedOperator(Operator):
    def __del__(self):  # owned by the MG object
        self.h = None


def read_data(filename, directory=None):
    """Sparse<long> read_data(const std::string&) (src/Parse.cpp:64-90).

    The reference opens "../../data/sample_matrix/" + filename relative to the cwd; `directory`
    (or $MGCR_SAMPLE_DIR) overrides that prefix.  Format: SURVEY.md Appendix B."""
    prefix = directory if directory is not None else os.environ.get("MGCR_SAMPLE_DIR", "../../data/sample_matrix/")
    path = os.path.join(prefix, filename)
    try:
        f = open(path, "r")
    except OSError:
        print("File read is unsuccessful!")  # src/Parse.cpp:67-68 (the reference then reads garbage)
        raise
    print("File read is successful.")
    with f:
        row, col, nnz = (int(t) for t in f.readline().split())
        rowptr = np.empty(row + 1, np.int64)
        rowptr[:row] = np.array(f.readline().split(), dtype=np.int64)
        rowptr[row] = nnz  # ROW[rows] = nnz, src/Operator.h:61
        cols = np.empty(nnz, np.int64)
        vals = np.empty(nnz, c128)
        for i, line in enumerate(f):
            if i >= nnz:
                break
            a, b = line.split()
            cols[i] = int(a)
            re, im = b[1:-1].split(",")
            vals[i] = complex(float(re), float(im))
    return Sparse(row, col, rowptr, cols, vals)
