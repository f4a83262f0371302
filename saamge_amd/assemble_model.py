"""CPU model of the device operator assembly (csrc/operator.hip) -- numpy only, test infrastructure like capi.py.

This file is the DEFINITION of the result: the device code restates it and must give the same bits.

  pattern      row i holds every dof j that shares an element with i, once, ascending; the structural union is stored (an
               entry whose value is zero stays).
  value        a_ij = sum of elmat_e[loc_e(i), loc_e(j)] over the elements e that hold both dofs, in ascending element id,
               starting from the first term (problems._assemble's documented order, MFEM's Assemble).
  elimination  dof i is essential when bdr[i] & ON_ESS_DOMAIN_BORDER.  An off-diagonal entry with an essential row or column
               becomes 0.0 and stays stored; the diagonal is kept.  bdr None: no essential dof.
  rhs          EliminateEssentialBCFromDofs(ess, x, b) with the diagonal kept: a non-essential row i gets
               b_i <- b_i - a_ij x_j over its essential columns j, ascending, one rounded product and one rounded
               difference per column, with the un-eliminated a_ij; an essential row gets b_i = a_ii x_i.
  refused      elem_ptr[0] != 0, an empty element or decreasing offsets, a dof outside [0, n), an element that lists a dof
               twice, a dof that lies in no element (the first one is named).

elem_ptr None: elem_to_dof is (NE, nde) and elmat (NE, nde, nde); otherwise flat elem_to_dof and elmat packed in element order
(element e: nd_e x nd_e row-major at sum_{f<e} nd_f^2), as saamge_amd_ml_produce_data_mixed takes them.
"""
import numpy as np

ON_ESS_DOMAIN_BORDER = 0x02


def _mesh(n, elem_ptr, elem_to_dof):
    e2d = np.asarray(elem_to_dof)
    if elem_ptr is None:
        if e2d.ndim != 2 or e2d.shape[1] < 1:
            raise ValueError("elem_to_dof: (NE, nde) with nde >= 1 is needed without elem_ptr")
        ep = np.arange(e2d.shape[0] + 1, dtype=np.int64) * e2d.shape[1]
    else:
        ep = np.asarray(elem_ptr, np.int64)
        if ep.ndim != 1 or len(ep) < 1 or ep[0] != 0:
            raise ValueError("elem_ptr: must start at 0")
        if (np.diff(ep) <= 0).any():
            raise ValueError("elem_ptr: every element needs a dof")
    e2d = e2d.astype(np.int64).ravel()
    if len(e2d) != ep[-1]:
        raise ValueError("elem_to_dof: elem_ptr[NE] entries are needed")
    if len(e2d) and (e2d.min() < 0 or e2d.max() >= n):
        raise ValueError("elem_to_dof entry out of range")
    nd = np.diff(ep)
    elem = np.repeat(np.arange(len(nd), dtype=np.int64), nd)
    if len(np.unique(elem * max(int(n), 1) + e2d)) != len(e2d):
        raise ValueError("an element lists a dof twice")
    free = np.flatnonzero(np.bincount(e2d, minlength=n) == 0)
    if len(free):
        raise ValueError("dof %d lies in no element" % free[0])
    return ep, e2d, nd


def _terms(n, elem_ptr, elem_to_dof, elmat):
    """Every (row, column, term) sorted by (row, column, element), the start of each (row, column) group and its size."""
    ep, e2d, nd = _mesh(n, elem_ptr, elem_to_dof)
    term = np.asarray(elmat, np.float64).ravel()
    if len(term) != int((nd * nd).sum()):
        raise ValueError("elmat: sum of nd_e^2 entries are needed")
    moff = np.concatenate([[0], np.cumsum(nd * nd)])
    rows = np.zeros(len(term), np.int64)
    cols = np.zeros(len(term), np.int64)
    for c in np.unique(nd):
        ids = np.flatnonzero(nd == c)
        d = e2d[ep[ids][:, None] + np.arange(c)]
        at = moff[ids][:, None] + np.arange(c * c)
        rows[at] = np.repeat(d, c, axis=1)
        cols[at] = np.tile(d, (1, c))
    order = np.argsort(rows * n + cols, kind="stable")           # packed order is element order: stable keeps it
    key = (rows * n + cols)[order]
    start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, np.int64)
    size = np.diff(np.concatenate([start, [len(key)]]))
    return key[start] // n, key[start] % n, term[order], start, size


def _sum_in_order(term, start, size):
    val = term[start].copy()
    for r in range(1, int(size.max()) if len(size) else 0):
        m = size > r
        val[m] = val[m] + term[start[m] + r]
    return val


def essential(n, bdr):
    if bdr is None:
        return np.zeros(n, bool)
    return (np.asarray(bdr).astype(np.int64) & ON_ESS_DOMAIN_BORDER) != 0


def assemble(n, elem_ptr, elem_to_dof, elmat, bdr=None, eliminate=True):
    """(rowptr int64 (n + 1), col int32, val float64)"""
    i, j, term, start, size = _terms(n, elem_ptr, elem_to_dof, elmat)
    val = _sum_in_order(term, start, size)
    if eliminate:
        ess = essential(n, bdr)
        val[(ess[i] | ess[j]) & (i != j)] = 0.0
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))]).astype(np.int64)
    return rowptr, j.astype(np.int32), val


def eliminate_rhs(n, elem_ptr, elem_to_dof, elmat, bdr, x_ess, b):
    """The new b (a copy)."""
    rowptr, col, val = assemble(n, elem_ptr, elem_to_dof, elmat, eliminate=False)
    ess = essential(n, bdr)
    x = np.asarray(x_ess, np.float64)
    out = np.array(b, np.float64)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    hit = np.flatnonzero(ess[col] & ~ess[row])                     # ascending (row, column)
    rank = np.arange(len(hit)) - np.searchsorted(row[hit], row[hit], side="left")
    for r in range(int(rank.max()) + 1 if len(hit) else 0):
        k = hit[rank == r]
        out[row[k]] = out[row[k]] - val[k] * x[col[k]]
    diag = np.flatnonzero((row == col) & ess[row])
    out[row[diag]] = val[diag] * x[row[diag]]
    return out


def assemble_rhs(n, elem_ptr, elem_to_dof, elvec):
    """b (n,): b_i the sum of the element terms of dof i in ascending element id, the first term taken as it is
    (_sum_in_order's rule).  elvec packed in element order (element e at sum_{f<e} nd_f), or (NE, nde) without elem_ptr.
    Essential dofs are assembled like any other; eliminate_rhs overwrites them afterwards."""
    ep, e2d, nd = _mesh(n, elem_ptr, elem_to_dof)
    term = np.asarray(elvec, np.float64).ravel()
    if len(term) != len(e2d):
        raise ValueError("elvec: sum of nd_e entries are needed")
    order = np.argsort(e2d, kind="stable")                           # packed order is element order: stable keeps it
    key = e2d[order]
    start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, np.int64)
    size = np.diff(np.concatenate([start, [len(key)]]))
    return _sum_in_order(term[order], start, size)                   # (_mesh refuses a dof in no element: n groups)
