"""Case table of the even-odd Schur solve for operators with a dense block per site (a plain module, like
tests/evenodd_diag_cases.py — not a test file): matrices whose sites of bs consecutive rows are coupled inside, built on the hopping
cases of tests/evenodd_cases.py, and a numpy model of the plan (csrc/evenodd_plan.h, evenodd_plan_build_block), of the blocks, of
their elimination and of the Schur apply, prepare and reconstruct of csrc/evenodd_block.hip.

The full operator is A = B - c H: H the stored entries between different sites, B one bs x bs block per site.  Dirac form:
A = 1 - k D, B_s = I - k D_ss, c = k; matrix form: A = M, B_s = D_ss, c = -1.  Entry (i, j) of D_ss = the stored entries at that
position added in stored order.  Every product is formed from real and imaginary parts with separate real operations (emul / einv
of tests/evenodd_diag_cases.py), a block-vector product accumulates j = 0 .. bs - 1 ascending, real and imaginary parts apart, and
the inverse of an odd block is Gauss-Jordan with partial pivoting on [B | I] in the fixed order of Rule 1b of include/mgcr.h — the
bits the device must show.

kron_case(hop_case, bs, seed) replaces every hop of a hopping case by a seeded dense bs x bs complex link and adds a seeded block
per site.  `open4d_b5` stands on the OPEN4D_DIMS lattice with ONE unknown per site (315 sites, 158 + 157 of them per colour) — not
on the 3780-row case `open4d`, whose every row would become a site with rows of up to 480 entries and 7.5 million entries in all:
what the case is for (n_e != n_o, more than 12 sites per half, sites that straddle lanes 63 | 64) holds on the small lattice.

tests/test_evenodd_block_cases.py (CPU) checks the premises on the model alone; tests/test_evenodd_block_plan.py runs the C++ plan
against the model; tests/test_gpu_evenodd_block.py runs the device against both.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import evenodd_cases as ec
from tests.evenodd_diag_cases import cplx, einv, emul

c128 = np.complex128

# form: "dirac" (k is the hopping parameter) or "matrix" (k is None); n, rowptr, col, val: the matrix WITH its in-site entries
BCase = namedtuple("BCase", "name form k bs n rowptr col val")

SOLVABLE = ("chain_b2", "open4d_b5", "sample_h05", "sample_h10", "w7_b16", "bpoisson_box", "no_insite", "dup_insite", "pivot_swap")
APPLY_ONLY = ("grid2d_varied_b3", "cond1e8", "singular_even")
ALL = SOLVABLE + APPLY_ONLY
LONG_ROWS = "w7_b16"             # rows of up to 7 x 16 entries: the halves get several lanes per row or a CSR tail
# H_eo stored one thread per row.  (The sample's halves are NOT: rows of 39 entries are stored with 8 lanes per row, as for the plain
# even-odd operator; the fused step of this operator does not depend on the storage of the halves and must run on every case.)
ONE_THREAD_PER_ROW = ("chain_b2", "bpoisson_box", "no_insite", "dup_insite", "pivot_swap", "cond1e8", "singular_even")
POISSON_DIMS = (6, 5, 4)
TOL = 1e-8
STEP_CAP = 400


def small_chain(nsites, seed):
    return ec.Case("chain%d" % nsites, *ec.chain_links([(i, i + 1) for i in range(nsites - 1)], nsites, seed))


def open4d_scalar():
    return ec.Case("open4d_scalar", *ec.hopping_lattice(ec.OPEN4D_DIMS, 1, False, 11, False))


def random_blocks(ns, bs, seed, scale=1.0, hermitian=False):
    rng = np.random.default_rng(seed)
    g = rng.uniform(-1, 1, (ns, bs, bs)) + 1j * rng.uniform(-1, 1, (ns, bs, bs))
    if hermitian:
        g = (g + np.conj(np.swapaxes(g, 1, 2))) / 2
    return (scale * g).astype(c128)


def coo_blocks(sites, blocks):
    """(rows, cols, vals) of dense bs x bs blocks placed on the diagonal at `sites`"""
    blocks = np.asarray(blocks, c128)
    bs = blocks.shape[-1]
    sites = np.asarray(sites, np.int64)
    a, b = np.meshgrid(np.arange(bs, dtype=np.int64), np.arange(bs, dtype=np.int64), indexing="ij")
    return ((sites[:, None, None] * bs + a[None]).ravel(), (sites[:, None, None] * bs + b[None]).ravel(), blocks.ravel())


def kron_hops(hop, bs, seed, identity=None):
    """every hop (r, c, v) of `hop` -> a dense bs x bs link at site pair (r, c): seeded random complex, or identity * I"""
    rows = ec.entry_rows(hop.n, hop.rowptr)
    if identity is not None:
        a = np.arange(bs, dtype=np.int64)
        return ((rows[:, None] * bs + a[None]).ravel(), (hop.col[:, None] * bs + a[None]).ravel(),
                np.full(rows.size * bs, identity, c128))
    rng = np.random.default_rng(seed)
    links = rng.uniform(-1, 1, (rows.size, bs, bs)) + 1j * rng.uniform(-1, 1, (rows.size, bs, bs))
    a, b = np.meshgrid(np.arange(bs, dtype=np.int64), np.arange(bs, dtype=np.int64), indexing="ij")
    return ((rows[:, None, None] * bs + a[None]).ravel(), (hop.col[:, None, None] * bs + b[None]).ravel(), links.astype(c128).ravel())


def assemble(n, parts):
    """CSR with every row's entries in ascending column order; entries at one position keep the order given"""
    return ec._csr_from_coo(n, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                            np.concatenate([np.asarray(p[2], c128) for p in parts]))


def kron_case(hop, bs, seed, blocks=None, sites=None, extra=()):
    """n, rowptr, col, val of hop (x) dense links + a block per site (`blocks` at `sites`; default: seeded, every site)"""
    if blocks is None:
        blocks = random_blocks(hop.n, bs, seed + 1)
    if sites is None:
        sites = np.arange(hop.n)
    return (hop.n * bs,) + assemble(hop.n * bs, [kron_hops(hop, bs, seed), coo_blocks(sites, blocks)] + list(extra))


def rough_k(n, rowptr, col, val):
    """0.7 over a rough estimate of the spectral radius, as ec.case_k"""
    return float(0.7 / (np.sqrt(col.size / n) * np.sqrt(np.mean(np.abs(val) ** 2))))


def dominant_blocks(ns, bs, seed, shift):
    return random_blocks(ns, bs, seed) + shift * np.eye(bs)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "chain_b2":                # 6 sites, 12 rows: halves far shorter than a wave
        mat = kron_case(small_chain(6, 31), 2, 131)
        return BCase(name, "dirac", rough_k(*mat), 2, *mat)
    if name == "grid2d_varied_b3":        # halves of 98304 rows: many workgroups, sites (3 rows) straddle every wave and workgroup edge
        mat = kron_case(ec.case("grid2d_varied"), 3, 132)
        return BCase(name, "dirac", rough_k(*mat), 3, *mat)
    if name == "open4d_b5":               # 158 even and 157 odd sites of 5 rows: n_e != n_o, a site straddles lanes 63 | 64
        mat = kron_case(open4d_scalar(), 5, 133)
        return BCase(name, "dirac", rough_k(*mat), 5, *mat)
    if name in ("sample_h05", "sample_h10"):   # the sample itself + Hermitian 12 x 12 blocks: 1536 half rows, sites straddle 256-row edges
        c = ec.case("sample")
        scale = 0.5 if name == "sample_h05" else 1.0
        blocks = random_blocks(c.n // 12, 12, 134, scale, hermitian=True)
        mat = assemble(c.n, [(ec.entry_rows(c.n, c.rowptr), c.col, c.val), coo_blocks(np.arange(c.n // 12), blocks)])
        return BCase(name, "dirac", 0.15, 12, c.n, *mat)
    if name == "w7_b16":                  # the widest block; rows of up to 112 entries
        mat = kron_case(ec.case("w7_slab"), 16, 135)
        return BCase(name, "dirac", rough_k(*mat), 16, *mat)
    if name == "bpoisson_box":            # block Poisson on the 6 x 5 x 4 box in matrix form: [[6, -0.5], [-0.5, 6]] on the diagonal, -I hops
        n, rowptr, col, val = ec.hopping_lattice(POISSON_DIMS, 1, False, 0, True, axis_real=True)
        hop = ec.Case("box", n, rowptr, col, val)
        blocks = np.broadcast_to(np.array([[6.0, -0.5], [-0.5, 6.0]], c128), (n, 2, 2))
        return BCase(name, "matrix", None, 2, 2 * n, *assemble(2 * n, [kron_hops(hop, 2, 0, identity=-1.0), coo_blocks(np.arange(n), blocks)]))
    if name == "no_insite":               # sites 2 (even) and 3 (odd) store no in-site entry: B = I there
        hop = small_chain(6, 36)
        keep = np.array([0, 1, 4, 5])
        mat = kron_case(hop, 2, 136, random_blocks(4, 2, 137), keep)
        return BCase(name, "dirac", rough_k(*mat), 2, *mat)
    if name == "dup_insite":              # positions (0, 1) of site 1 (odd) and (1, 1) of site 2 (even) are stored three times / twice
        hop = small_chain(6, 38)
        extra = [(np.array([2, 2, 5]), np.array([3, 3, 5]), np.array([0.25 - 0.5j, 1e-3 + 2.0j, -0.75 + 0.125j]))]
        mat = kron_case(hop, 2, 138, extra=extra)
        return BCase(name, "dirac", rough_k(*mat), 2, *mat)
    if name == "pivot_swap":              # matrix form; the odd site 1 has B_00 = 0 exactly (not stored): the elimination must swap
        hop = small_chain(6, 39)
        blocks = dominant_blocks(6, 3, 139, 6.0)
        blocks[1] = np.array([[0.0, 2.0, 1.0], [3.0, 0.5j, 1.0], [1.0, 1.0, 4.0]])
        r, c, v = coo_blocks(np.arange(6), blocks)
        stored = ~((r == 3) & (c == 3))
        return BCase(name, "matrix", None, 3, 18, *assemble(18, [kron_hops(hop, 3, 140), (r[stored], c[stored], v[stored])]))
    if name == "cond1e8":                 # matrix form; the odd site 3 has a block of condition ~ 1e8
        hop = small_chain(6, 41)
        blocks = dominant_blocks(6, 4, 141, 6.0)
        rng = np.random.default_rng(142)
        u, _ = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))
        w, _ = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))
        blocks[3] = (u * np.array([1.0, 1e-2, 1e-5, 1e-8])) @ w
        return BCase(name, "matrix", None, 4, 24, *kron_case(hop, 4, 143, blocks)[1:])
    if name == "singular_even":           # matrix form; the even site 2 has a block of rank 1
        hop = small_chain(6, 44)
        blocks = dominant_blocks(6, 2, 144, 6.0)
        blocks[2] = np.array([[1.0, 2.0], [2.0, 4.0]])
        return BCase(name, "matrix", None, 2, 12, *kron_case(hop, 2, 145, blocks)[1:])
    raise ValueError(name)


def with_k(bc, k):
    return bc._replace(k=k) if bc.form == "dirac" else bc


@functools.lru_cache(maxsize=None)
def rejected(name):
    """not_whole: (BCase whose n is no multiple of bs); bs0 / bs17: a BCase with that bs; triangle: (BCase, (row, column) named);
    split_parity: (BCase, parity, the row named, its site); flipped: (BCase, parity, (row, column) named);
    singular_odd: (BCase refused at creation, site, row named); set_k_singular: (BCase accepted, the k its set_k must refuse, site, row)"""
    good = case("chain_b2")
    if name == "not_whole":
        mat = kron_case(small_chain(5, 51), 3, 151)
        return BCase(name, "dirac", 0.1, 2, *mat)                       # 15 rows, bs = 2
    if name in ("bs0", "bs17"):
        return good._replace(name=name, bs=0 if name == "bs0" else 17)
    if name == "triangle":            # sites 0, 1, 2 in a ring: 0 even, 1 and 2 odd; the first inter-site entry with equal colours joins 1 and 2
        hop, _, _ = ec.rejected("triangle")
        mat = kron_case(hop, 2, 152)
        bc = BCase(name, "dirac", 0.1, 2, *mat)
        inter, _, _ = strip_case(bc)
        par = np.repeat(ec.colour(*site_graph(inter, 2)), 2)
        return bc, ec.first_conflict(inter.n, inter.rowptr, inter.col, par)
    if name == "split_parity":        # row 7 (site 3) gets the other colour than row 6
        par = np.repeat(np.arange(6) % 2, 2).astype(np.int8)
        par[7] ^= 1
        return good, par, 7, 3
    if name == "flipped":             # site 4 as a whole gets the colour of its neighbours
        par = np.repeat(np.arange(6) % 2, 2).astype(np.int8)
        par[8:10] ^= 1
        inter, _, _ = strip_case(good)
        return good, par, ec.first_conflict(inter.n, inter.rowptr, inter.col, par)
    if name == "singular_odd":        # Dirac form, k = 0.5: the odd site 1 stores d = [[2, 0], [0, 1]], so I - k d = [[0, 0], [0, 0.5]]
        hop = small_chain(6, 53)
        blocks = random_blocks(6, 2, 153)
        blocks[1] = np.array([[2.0, 0.0], [0.0, 1.0]])
        return BCase(name, "dirac", 0.5, 2, *kron_case(hop, 2, 154, blocks)), 1, 2
    if name == "set_k_singular":      # d = 2 E_00 on the odd site 3: fine at k = 0.25, I - k d has a zero first column at k = 0.5
        hop = small_chain(6, 55)
        blocks = random_blocks(6, 2, 155)
        blocks[3] = np.array([[2.0, 0.0], [0.0, 0.0]])
        return BCase(name, "dirac", 0.25, 2, *kron_case(hop, 2, 156, blocks)), 0.5, 3, 6
    raise ValueError(name)


# ---- the model --------------------------------------------------------------------------------------------------------------------
def strip_case(bc):
    """(the inter-site part as an ec.Case, D_ss[sites, bs, bs], the number of stored in-site entries)"""
    bs = bc.bs
    rows = ec.entry_rows(bc.n, bc.rowptr)
    on = rows // bs == bc.col // bs
    blocks = np.zeros((bc.n // bs, bs, bs), c128)
    np.add.at(blocks, (rows[on] // bs, rows[on] % bs, bc.col[on] % bs), bc.val[on])         # in stored order
    rowptr = np.zeros(bc.n + 1, np.int64)
    np.cumsum(np.bincount(rows[~on], minlength=bc.n), out=rowptr[1:])
    return ec.Case(bc.name, bc.n, rowptr, bc.col[~on], bc.val[~on]), blocks, int(on.sum())


def site_graph(inter, bs):
    """(number of sites, rowptr, col) of the site graph of the inter-site entries, duplicates kept"""
    ns = inter.n // bs
    rows = ec.entry_rows(inter.n, inter.rowptr) // bs
    sptr = np.zeros(ns + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=ns), out=sptr[1:])
    return ns, sptr, inter.col // bs


@functools.lru_cache(maxsize=None)
def strip(name):
    return strip_case(case(name))


def plan_of(bc, parity=None):
    inter, _, _ = strip_case(bc)
    if parity is None:
        parity = np.repeat(ec.colour(*site_graph(inter, bc.bs)), bc.bs)
    return ec.plan(inter, parity)


@functools.lru_cache(maxsize=None)
def case_plan(name):
    inter = strip(name)[0]
    return ec.plan(inter, np.repeat(ec.colour(*site_graph(inter, case(name).bs)), case(name).bs))


Coef = namedtuple("Coef", "B c c2 cn")     # B[sites, bs, bs] of every site, in full-system site order


def coefficients(bc, d):
    if bc.form == "matrix":
        c = c128(-1.0)
        return Coef(d.copy(), c, c128(emul(c, c)), c128(cplx(-c.real, -c.imag)))
    k = c128(bc.k)
    kd = emul(np.full(d.shape, k), d)
    eye = np.broadcast_to(np.eye(bc.bs), d.shape)
    return Coef(cplx(eye - kd.real, 0.0 - kd.imag), k, c128(emul(k, k)), c128(cplx(-k.real, -k.imag)))


def site_lists(p, bs):
    """(even sites, odd sites) in list order"""
    return p.even[::bs] // bs, p.odd[::bs] // bs


def bmul(M, x):
    """(M (.) x): M[sites, bs, bs], x[sites * bs]; acc = M_i0 x_0, then + M_ij x_j ascending, real and imaginary parts apart"""
    s, bs, _ = M.shape
    if s == 0:
        return np.zeros(0, c128)
    X = np.asarray(x, c128).reshape(s, bs)
    acc = emul(M[:, :, 0], X[:, None, 0])
    re, im = acc.real.copy(), acc.imag.copy()
    for j in range(1, bs):
        t = emul(M[:, :, j], X[:, None, j])
        re = re + t.real
        im = im + t.imag
    return cplx(re, im).reshape(s * bs)


def invert(B):
    """Gauss-Jordan with partial pivoting on [B | I], every site at once: (inverse[sites, bs, bs], first failing pivot per site or
    -1, number of row swaps per site).  A failed site's inverse is meaningless."""
    s, bs, _ = B.shape
    aug = np.zeros((s, bs, 2 * bs), c128)
    aug[:, :, :bs] = B
    aug[:, np.arange(bs), bs + np.arange(bs)] = 1.0
    failed = np.full(s, -1, np.int64)
    swaps = np.zeros(s, np.int64)
    idx = np.arange(s)
    with np.errstate(all="ignore"):
        for p in range(bs):
            col = aug[:, :, p]
            mag = col.real * col.real + col.imag * col.imag
            best, q = mag[:, p].copy(), np.full(s, p, np.int64)
            for i in range(p + 1, bs):
                upd = mag[:, i] > best                    # the first maximum wins
                best = np.where(upd, mag[:, i], best)
                q = np.where(upd, i, q)
            live = failed < 0
            sw = live & (q != p)
            swaps += sw
            rp, rq = aug[idx[sw], p].copy(), aug[idx[sw], q[sw]].copy()
            aug[idx[sw], p], aug[idx[sw], q[sw]] = rq, rp
            app = aug[:, p, p]
            den = app.real * app.real + app.imag * app.imag
            bad = live & (~(den > 0.0) | ~np.isfinite(den))
            failed[bad] = p
            go = live & ~bad
            piv = cplx(app.real / den, -app.imag / den)
            rowp = emul(aug[:, p, :], piv[:, None])
            f = aug[:, :, p].copy()
            new = aug - emul(f[:, :, None], rowp[:, None, :])
            new[:, p, :] = rowp
            aug[go] = new[go]
    return aug[:, :, bs:].copy(), failed, swaps


def first_failure(failed):
    """(site, pivot) the device's status word names: the smallest site that failed, its first failing pivot; None"""
    bad = np.nonzero(failed >= 0)[0]
    return None if bad.size == 0 else (int(bad[0]), int(failed[bad[0]]))


def full_apply(bc, x):
    """A x with the matrix as stored (numpy arithmetic: a reference to rounding, not to the bit)"""
    y = ec.csr_apply(ec.Case(bc.name, bc.n, bc.rowptr, bc.col, bc.val), x)
    return y if bc.form == "matrix" else x - bc.k * y


def dense(bc):
    A = np.zeros((bc.n, bc.n), c128)
    np.add.at(A, (ec.entry_rows(bc.n, bc.rowptr), bc.col), bc.val)
    return A if bc.form == "matrix" else np.eye(bc.n) - bc.k * A


Model = namedtuple("Model", "bc plan co Be invBo failed swaps")


def scalar_times(s, v):
    return emul(np.full(v.size, c128(s)), v)


def schur_apply(m, x):
    t = bmul(m.invBo, ec.csr_apply(m.plan.oe, x))
    return bmul(m.Be, x) - scalar_times(m.co.c2, ec.csr_apply(m.plan.eo, t))


def prepare(m, b):
    return b[m.plan.even] - scalar_times(m.co.cn, ec.csr_apply(m.plan.eo, bmul(m.invBo, b[m.plan.odd])))


def reconstruct(m, b, xe):
    x = np.empty(m.plan.n, c128)
    x[m.plan.even] = xe
    x[m.plan.odd] = bmul(m.invBo, b[m.plan.odd] - scalar_times(m.co.cn, ec.csr_apply(m.plan.oe, xe)))
    return x


def model_of(bc, plan):
    _, d, _ = strip_case(bc)
    co = coefficients(bc, d)
    se, so = site_lists(plan, bc.bs)
    inv, failed, swaps = invert(co.B[so])
    return Model(bc, plan, co, co.B[se], inv, failed, swaps)


@functools.lru_cache(maxsize=None)
def _model(name, k):
    bc = case(name) if k is None else with_k(case(name), k)
    return model_of(bc, case_plan(name))


def model(name, k=None):
    return _model(name, None if k is None else complex(k))
