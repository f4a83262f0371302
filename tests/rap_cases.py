"""Host emulation of the Galerkin product through the MIS blocks, in the order of sums that DESIGN.md section 4 specifies
(shared by test_rap_cases.py, which checks the emulation itself without a GPU, and test_gpu_rap.py).

For a MIS m1 with dofs d[0..r1) in mis_to_dof order, the columns of its k1 rows of Ac are the blocks of the neighbour MISes
with k > 0 in ascending id (stored zeros of A count as adjacency).  T[il][c] starts at 0.0 and takes
fma(a_q, P[col_q, c], T[il][c]) over the stored entries q of row d[il] of A in storage order, for the c of the block of the
MIS of col_q only (and only if that MIS has k > 0).  Ac[(m1, v1), c] starts at 0.0 and takes
fma(P[d[il], coloff[m1] + v1], T[il][c], .) for il = 0 .. r1-1.

The fma is exactly rounded.  fma_exact is the plain definition with rationals (12 us per operation); fma is the same on
numpy arrays from error-free transformations: a b = uh + ul (Dekker), c + uh = th + tl (Knuth), and
RN(th + RO(tl + ul)) with RO rounding to odd (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums: proved
algorithms using rounding to odd", IEEE TC 57(4), 2008): correct whenever nothing over- or underflows, which holds for
operators and bases whose entries are within a few hundred binades of 1."""
from fractions import Fraction

import numpy as np
import scipy.sparse as sp


def fma_exact(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """Exactly rounded a * b + c, elementwise on float64 arrays (broadcast)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64),
                                  np.asarray(c, dtype=np.float64))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    vh, vl = _two_sum(tl, ul)
    bits = np.ascontiguousarray(vh).view(np.int64)
    need = (vl != 0.0) & ((bits & 1) == 0)            # inexact and even: the odd neighbour on the side of the remainder
    away = (vl > 0.0) == (vh > 0.0)
    v = np.where(need, np.where(away, bits + 1, bits - 1), bits).view(np.float64)
    return th + v


def coloff_of(k):
    return np.concatenate(([0], np.cumsum(np.asarray(k, dtype=np.int64))))


def neighbours(A, mises, k, dofs):
    """Neighbour MISes with k > 0 of the MIS whose dofs are `dofs`, ascending."""
    cols = np.concatenate([A.indices[A.indptr[g]:A.indptr[g + 1]] for g in dofs] + [np.zeros(0, dtype=A.indices.dtype)])
    ms = np.unique(mises[cols])
    return ms[k[ms] > 0]


def mis_adjacency(A, mises, k):
    """nm x nm 0/1 matrix: MIS m2 with k > 0 holds the column of a stored entry (zeros included) of a row of MIS m1."""
    k = np.asarray(k)
    n, nm = A.shape[0], len(k)
    M = sp.csr_matrix((np.ones(n), (mises, np.arange(n))), shape=(nm, n))
    pat = sp.csr_matrix((np.ones(len(A.indices)), A.indices, A.indptr), shape=A.shape)
    adj = sp.csr_matrix(M @ pat @ M.T)
    adj.data[:] = 1.0
    return sp.csr_matrix(adj @ sp.diags((k > 0).astype(np.float64)))


LDS_BUDGET = 160 * 1024 // 8      # doubles of LDS a workgroup of the product may take (rap_mis, csrc/mis.hip)


def lds_need(adj, k):
    """Per MIS (one_pass, floor), as rap_size_kernel counts them (0 where k = 0): the doubles of LDS with which the block is
    done in one pass -- the tables of its nn neighbours, its k accumulator rows and one row of T, each of ncol doubles -- and
    the least the kernel can work with, tables and two rows.  one_pass > LDS_BUDGET: the block takes the multi-pass path
    (KC < k1); floor > LDS_BUDGET: the library refuses.  `adj`: mis_adjacency(A, mises, k) with its zeros eliminated."""
    k = np.asarray(k, dtype=np.int64)
    nn = np.diff(adj.indptr).astype(np.int64)
    ncol = np.asarray(adj @ k.astype(np.float64)).astype(np.int64)
    on = k > 0
    return np.where(on, 3 * nn + 2 + (k + 1) * ncol, 0), np.where(on, 3 * nn + 2 + 2 * ncol, 0)


def emulate_mis_rows(A, P, mises, k, m2d_I, m2d_J, m1, scalar=False):
    """Rows of Ac of MIS m1: (cols, vals) with cols the ncol column indices (shared by its k[m1] rows) and vals of shape
    (k[m1], ncol).  A and P are scipy CSR matrices in the library's storage order; P holds k entries per dof, the block of
    the dof's MIS.  scalar: the slow definition with fma_exact instead of the vectorised walk."""
    k = np.asarray(k)
    coloff = coloff_of(k)
    d = np.asarray(m2d_J[m2d_I[m1]:m2d_I[m1 + 1]], dtype=np.int64)
    k1, r1 = int(k[m1]), len(d)
    nb = neighbours(A, mises, k, d)
    cols = np.concatenate([np.arange(coloff[m], coloff[m] + k[m]) for m in nb] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    ncol = len(cols)
    cpos = {int(c): i for i, c in enumerate(cols)}
    pos_of = np.full(int(coloff[-1]) + 1, -1, dtype=np.int64)
    pos_of[cols] = np.arange(ncol)
    Pp, Pi, Px = P.indptr.astype(np.int64), P.indices, P.data
    T = np.zeros((r1, ncol))
    if scalar:
        for il, g in enumerate(d):
            for q in range(A.indptr[g], A.indptr[g + 1]):
                col, a = int(A.indices[q]), A.data[q]
                m2 = int(mises[col])
                for v in range(int(k[m2])):
                    assert Pi[Pp[col] + v] == coloff[m2] + v
                    c = cpos[int(coloff[m2]) + v]
                    T[il, c] = fma_exact(a, Px[Pp[col] + v], T[il, c])
        vals = np.zeros((k1, ncol))
        for v1 in range(k1):
            for c in range(ncol):
                s = 0.0
                for il, g in enumerate(d):
                    assert Pi[Pp[g] + v1] == coloff[m1] + v1
                    s = fma_exact(Px[Pp[g] + v1], T[il, c], s)
                vals[v1, c] = s
        return cols, vals
    # entry t of every row at once: the rows are independent, and the k products of an entry go to k different columns
    start = A.indptr[d].astype(np.int64)
    length = A.indptr[d + 1].astype(np.int64) - start
    Tf = T.reshape(-1)
    for t in range(int(length.max()) if r1 else 0):
        act = np.nonzero(length > t)[0]
        q = start[act] + t
        col = A.indices[q].astype(np.int64)
        m2 = mises[col].astype(np.int64)
        k2 = k[m2].astype(np.int64)
        on = k2 > 0
        act, q, col, m2, k2 = act[on], q[on], col[on], m2[on], k2[on]
        if not len(act):
            continue
        first = np.cumsum(k2) - k2
        v = np.arange(int(k2.sum())) - np.repeat(first, k2)
        pq = np.repeat(Pp[col], k2) + v
        c = np.repeat(coloff[m2], k2) + v
        assert np.array_equal(Pi[pq], c)
        idx = np.repeat(act, k2) * ncol + pos_of[c]
        assert (pos_of[c] >= 0).all()
        Tf[idx] = fma(np.repeat(A.data[q], k2), Px[pq], Tf[idx])
    vals = np.zeros((k1, ncol))
    for il, g in enumerate(d):
        assert np.array_equal(Pi[Pp[g]:Pp[g] + k1], coloff[m1] + np.arange(k1))
        vals = fma(Px[Pp[g]:Pp[g] + k1][:, None], T[il][None, :], vals)
    return cols, vals


def ac_rows(Ac, k, m1):
    """The stored rows of MIS m1 in Ac: (list of column arrays, list of value arrays), one per basis vector."""
    coloff = coloff_of(k)
    rows = range(int(coloff[m1]), int(coloff[m1 + 1]))
    return ([Ac.indices[Ac.indptr[r]:Ac.indptr[r + 1]] for r in rows], [Ac.data[Ac.indptr[r]:Ac.indptr[r + 1]] for r in rows])


def check_mis_exact(Ac, A, P, mises, k, m2d_I, m2d_J, m1):
    """Rows of MIS m1 of Ac == the emulation: column indices and values (with ==)."""
    if k[m1] == 0:
        return 0
    cols, vals = emulate_mis_rows(A, P, mises, k, m2d_I, m2d_J, m1)
    got_c, got_v = ac_rows(Ac, k, m1)
    for v1 in range(int(k[m1])):
        assert np.array_equal(got_c[v1], cols), (m1, v1)
        bad = np.nonzero(got_v[v1] != vals[v1])[0]
        assert not len(bad), (m1, v1, bad[:4], got_v[v1][bad[:4]], vals[v1][bad[:4]])
    return int(k[m1]) * len(cols)
