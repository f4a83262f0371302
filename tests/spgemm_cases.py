"""Inputs, a host model of the route selection and plain references for the tests of the general sparse products, the transpose
and the threshold of csrc/spgemm.hip (not a test module).

A product case is  C = beta E + alpha diag(d) A B  with the operands as scipy CSR matrices whose rows are passed to the kernels
AS STORED: every input row has distinct columns (the kernels rely on it), and the cases marked `shuffled` store their rows in a
random order of columns.  The thresholds the cases sit on are those of spgemm.hip:

    hash-table product   three tiers of 256, 2048 and 8192 slots; the tier that holds the row with the most distinct columns
                         serves the whole product, a row beyond 8192 is refused
    dense-B product      only for E = d = none, alpha = 1, beta = 0, and B.ncols <= 2048, A.nnz >= 256 A.nrows,
                         B.nrows B.ncols <= 2^27

Two families of values.  `exact`: integers with 1 <= |v| <= 8, d powers of two, alpha and beta dyadic -- every partial sum is a
dyadic number of a few bits far below 2^53, the reference is exact and the comparison bitwise.  `general`: seeded normal values and
alpha = 1 / sin^2(pi / 5) (interp_smooth's weight), the reference in long double and an entrywise bound from the kernel's
arithmetic (reference_product).
"""
import numpy as np
import scipy.sparse as sp

TIERS = (256, 2048, 8192)          # slots of the three hash tables (launch_spgemm<T, WPB>)
WAVES_PER_WORKGROUP = (4, 2, 1)
DENSE_MAX_COLS = 2048              # SPD_MAXC
DENSE_MAX_CELLS = 1 << 27
DENSE_MIN_ROW = 256                # A.nnz >= 256 A.nrows
ROUTE_DENSE, ROUTE_REFUSED = 3, "refused"
SORT_LDS = 2048                    # row_order_kernel<2048>: longer rows are sorted by rank counting
CHUNK = 64                         # threshold_kernel: entries per ballot

ALPHA_SMOOTH = float(1.0 / np.sin(np.pi / 5.0) ** 2)
FAMILIES = ("exact", "general")
HAVE_LONGDOUBLE = bool(np.finfo(np.longdouble).eps < 1e-18)


# ---------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------
def csr_from_rows(rows, ncols, vals=None):
    """rows: one integer array of (distinct) columns per row, kept in the order given"""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    indices = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    data = np.ones(len(indices)) if vals is None else np.asarray(vals, dtype=np.float64)
    M = sp.csr_matrix((data, indices, indptr), shape=(len(rows), ncols))
    assert rows_have_distinct_columns(M)
    return M


def rows_of(M):
    return [M.indices[M.indptr[i]:M.indptr[i + 1]] for i in range(M.shape[0])]


def rows_have_distinct_columns(M):
    return all(len(np.unique(r)) == len(r) for r in rows_of(M))


def rows_are_sorted(M):
    return all(np.all(np.diff(r) > 0) for r in rows_of(M))


def shuffled_rows(M, rng):
    """the same matrix with every row stored in a random order of its columns"""
    indices, data = M.indices.copy(), M.data.copy()
    for i in range(M.shape[0]):
        b, e = M.indptr[i], M.indptr[i + 1]
        p = rng.permutation(e - b)
        indices[b:e], data[b:e] = M.indices[b:e][p], M.data[b:e][p]
    return sp.csr_matrix((data, indices, M.indptr.copy()), shape=M.shape)


def with_values(M, family, rng):
    """M's pattern with values of the family (never zero)"""
    n = len(M.indices)
    if family == "exact":
        v = rng.integers(1, 9, size=n).astype(np.float64) * rng.choice([-1.0, 1.0], size=n)
    else:
        v = rng.standard_normal(n)
        v[v == 0.0] = 1.0
    return sp.csr_matrix((v, M.indices.copy(), M.indptr.copy()), shape=M.shape)


def pattern(M):
    return sp.csr_matrix((np.ones(len(M.indices)), M.indices, M.indptr), shape=M.shape)


def product_row_counts(A, B, E=None):
    """distinct columns per row of the STRUCTURAL product (and of E)"""
    S = pattern(A) @ pattern(B)
    if E is not None:
        S = S + pattern(E)
    return np.diff(sp.csr_matrix(S).indptr)


def model_route(A, B, E=None, d=None, alpha=1.0, beta=0.0):
    """the route spgemm takes, from its documented predicates: ROUTE_DENSE, the final hash tier, or ROUTE_REFUSED"""
    n = A.shape[0]
    if n == 0:
        return -1
    plain = E is None and d is None and alpha == 1.0 and beta == 0.0
    if (plain and B.shape[1] <= DENSE_MAX_COLS and B.shape[0] * B.shape[1] <= DENSE_MAX_CELLS
            and len(A.indices) >= DENSE_MIN_ROW * n):
        return ROUTE_DENSE
    most = int(product_row_counts(A, B, E).max())
    for tier, slots in enumerate(TIERS):
        if most <= slots:
            return tier
    return ROUTE_REFUSED


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def reference_product(A, B, E=None, d=None, alpha=1.0, beta=0.0, extended=False):
    """(C, bound): the product row by row in the kernel's order of operations, accumulated in fp64 (exact for the exact family)
    or in long double.  C has the structural pattern (cancelled entries stay as zeros), rows sorted.  bound[k] belongs to
    C.data[k]:  (len(A row i) + 3) 2^-53 (|beta| |E| + |alpha| |d| |A| |B|)_ij  -- the kernel rounds alpha d once, its product
    with A_ik once, every fma once and beta E_ij once, so an entry of row i passes through at most len(A row i) + 2 roundings;
    the last unit covers the second-order terms and the long double reference."""
    ft = np.longdouble if extended else np.float64
    n, nc = A.shape[0], B.shape[1]
    acc, mag, hit = np.zeros(nc, dtype=ft), np.zeros(nc, dtype=ft), np.zeros(nc, dtype=bool)
    indptr, cols, vals, bounds = [0], [], [], []
    for i in range(n):
        touched = []
        if E is not None:
            ec = E.indices[E.indptr[i]:E.indptr[i + 1]]
            ev = ft(beta) * E.data[E.indptr[i]:E.indptr[i + 1]].astype(ft)
            acc[ec] += ev
            mag[ec] += np.abs(ev)
            hit[ec] = True
            touched.append(ec)
        sc = ft(alpha) * (ft(d[i]) if d is not None else ft(1.0))
        for p in range(A.indptr[i], A.indptr[i + 1]):
            k = A.indices[p]
            a = sc * ft(A.data[p])
            bc = B.indices[B.indptr[k]:B.indptr[k + 1]]
            t = a * B.data[B.indptr[k]:B.indptr[k + 1]].astype(ft)
            acc[bc] += t                      # (a row of B has distinct columns)
            mag[bc] += np.abs(t)
            hit[bc] = True
            touched.append(bc)
        c = np.nonzero(hit)[0]
        cols.append(c.astype(np.int32))
        vals.append(acc[c].astype(np.float64))
        bounds.append(((A.indptr[i + 1] - A.indptr[i] + 3) * 2.0 ** -53 * mag[c]).astype(np.float64))
        indptr.append(indptr[-1] + len(c))
        for t in touched:
            acc[t], mag[t], hit[t] = 0.0, 0.0, False
    cat = lambda parts, dt: np.concatenate(parts + [np.zeros(0, dt)]).astype(dt)      # noqa: E731
    C = sp.csr_matrix((cat(vals, np.float64), cat(cols, np.int32), np.asarray(indptr, dtype=np.int32)), shape=(n, nc))
    return C, cat(bounds, np.float64)


def reference_transpose(P):
    """P^T with sorted rows; the values are copied, never added"""
    r, c = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr)), P.indices
    order = np.lexsort((r, c))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=P.shape[1]))]).astype(np.int32)
    return sp.csr_matrix((P.data[order], r[order].astype(np.int32), indptr), shape=(P.shape[1], P.shape[0]))


def sorted_rows(M):
    """M with every row ordered by column (values carried along bit for bit)"""
    r = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    order = np.lexsort((M.indices, r))
    return sp.csr_matrix((M.data[order], M.indices[order], M.indptr.copy()), shape=M.shape)


def reference_threshold(A, tol):
    keep = np.abs(A.data) > tol
    r = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r[keep], minlength=A.shape[0]))]).astype(np.int32)
    return sp.csr_matrix((A.data[keep], A.indices[keep], indptr), shape=A.shape)


# ---------------------------------------------------------------------------------------------------------------------
# product cases on the hash path
# ---------------------------------------------------------------------------------------------------------------------
def _long_row_pattern(target, nrows, seed, bump=False, e_new=None):
    """(A, B, E, info): row `info["row"]` of A B has exactly `target` distinct columns (+ 1 with bump: one more column in one
    row of B, nothing else changed), every other row far fewer.  The long row has `m` entries, each on a row of B with about 100
    to 300 entries; 32 columns are in EVERY one of these rows (hit by every entry of the long row of A) and the others overlap
    at random.  Row 0 of B and its last row are empty and referenced; one row of A is empty where nrows allows it.
    e_new: an E whose long row has 40 columns of the product and e_new columns outside it (None: no E)."""
    rng = np.random.default_rng(seed)
    m = max(24, -(-target // 140))
    ncols = target + 300 + target // 8
    U = np.sort(rng.choice(ncols, size=target, replace=False))
    outside = np.setdiff1d(np.arange(ncols), U)
    hot = U[rng.choice(target, size=min(32, target), replace=False)]
    owner = rng.integers(0, m, size=target)
    nsmall = 6
    nB = 1 + m + nsmall + 1                       # empty | long rows | small rows | empty
    brows = [np.zeros(0, np.int64)]
    for j in range(m):
        extra = U[rng.choice(target, size=min(target, int(rng.integers(90, 200))), replace=False)]
        brows.append(np.unique(np.concatenate([U[owner == j], hot, extra])))
    if bump:
        brows[m] = np.concatenate([brows[m], outside[:1]])          # (stored last: this row is not sorted)
    for j in range(nsmall):
        brows.append(np.sort(rng.choice(ncols, size=int(rng.integers(1, 20)), replace=False)))
    brows.append(np.zeros(0, np.int64))
    long_row = 0 if nrows == 1 else nrows - 2
    arows = []
    for i in range(nrows):
        if i == long_row:
            arows.append(np.concatenate([[0], np.arange(1, m + 1), [nB - 1]]))
        elif i == 1:
            arows.append(np.zeros(0, np.int64))                       # an empty row of A
        elif i == 2 and target > TIERS[0]:
            arows.append(np.array([0, 1, 2, 3, m + 1]))               # a second row beyond the first table
        else:
            arows.append(np.concatenate([[0], np.sort(rng.choice(np.arange(m + 1, m + 1 + nsmall), size=3, replace=False))]))
    A, B = csr_from_rows(arows, nB), csr_from_rows(brows, ncols)
    E = None
    if e_new is not None:
        erows = []
        for i in range(nrows):
            if i == long_row:
                erows.append(np.sort(np.concatenate([U[rng.choice(target, size=40, replace=False)], outside[1:1 + e_new]])))
            elif i == 0:
                erows.append(np.zeros(0, np.int64))
            else:
                erows.append(np.sort(rng.choice(ncols, size=5, replace=False)))
        E = csr_from_rows(erows, ncols)
    return A, B, E, {"row": long_row, "hot": hot, "m": m}


def hash_home(key, slots):
    """home slot of a column in a table of `slots` (a power of two): the high bits of the multiplicative hash (common.h)"""
    return ((int(key) * 2654435761) & 0xFFFFFFFF) >> (32 - (slots.bit_length() - 1))


def probes_needed(before, key, slots):
    """slots the open-addressing table looks at until `key` has a place, after the distinct keys `before` went in (linear
    probing: which slots they occupy does not depend on their order); None when the table is full"""
    used = np.zeros(slots, dtype=bool)
    for k in before:
        h = hash_home(k, slots)
        while used[h]:
            h = (h + 1) % slots
        used[h] = True
    h = hash_home(key, slots)
    for probe in range(slots):
        if not used[h]:
            return probe + 1
        h = (h + 1) % slots
    return None


def _last_probe_pattern(slots, seed):
    """A row that fills a table to its last slot, and whose last column finds that slot with the very last probe: the row of A
    has the entries 1 .. m and then m + 1; rows 1 .. m of B hold slots - 1 columns between them, row m + 1 the single column
    whose home is the slot right AFTER the one left free."""
    rng = np.random.default_rng(seed)
    ncols = 4 * slots
    first = rng.choice(ncols, size=slots - 1, replace=False)
    used = np.zeros(slots, dtype=bool)
    for k in first:
        h = hash_home(k, slots)
        while used[h]:
            h = (h + 1) % slots
        used[h] = True
    free = int(np.nonzero(~used)[0][0])
    taken = set(first.tolist())
    last = next(c for c in range(ncols) if c not in taken and hash_home(c, slots) == (free + 1) % slots)
    m = -(-(slots - 1) // 200)
    brows = [np.zeros(0, np.int64)] + [np.sort(part) for part in np.array_split(first, m)] + [np.array([last])]
    arows = [np.array([0, 1]), np.zeros(0, np.int64), np.arange(0, m + 2)]
    return csr_from_rows(arows, m + 2), csr_from_rows(brows, ncols), {"row": 2, "first": first, "last": last}


def _product_case(expect, A, B, E=None, d=False, alpha=1.0, beta=0.0, shuffled=False, seed=0, **info):
    return dict(kind="pattern", expect=expect, A=A, B=B, E=E, d=d, alpha=alpha, beta=beta, shuffled=shuffled, seed=seed, **info)


def _square_alias_pattern(n, width, per_row, seed):
    """A square (n x n) and B (n x width) for E = B: row n - 2 of A has every column, the rows of B have per_row entries"""
    rng = np.random.default_rng(seed)
    brows = [np.sort(rng.choice(width, size=per_row, replace=False)) for _ in range(n)]
    brows[0] = np.zeros(0, np.int64)
    arows = [np.sort(rng.choice(n, size=2, replace=False)) for _ in range(n)]
    arows[1] = np.zeros(0, np.int64)
    arows[n - 2] = np.arange(n)
    return csr_from_rows(arows, n), csr_from_rows(brows, width), {"row": n - 2}


def _dense_pattern(ncols, seed, lengths=(600, 590, 0, 610, 3, 640, 0, 600, 620, 0, 580, 615, 0), nB=3000):
    """A: rows of `lengths` entries over nB columns; B: nB x ncols with up to 6 entries per row, every 7th column and the
    last one structurally empty (none where ncols == 1), every 11th row empty"""
    rng = np.random.default_rng(seed)
    arows = [np.sort(rng.choice(nB, size=l, replace=False)) for l in lengths]
    live = np.array([c for c in range(ncols) if ncols == 1 or (c % 7 != 3 and c != ncols - 1)])
    brows = []
    for k in range(nB):
        cnt = 0 if k % 11 == 5 else min(len(live), int(rng.integers(1, 7)))
        brows.append(np.sort(rng.choice(live, size=cnt, replace=False)))
    return csr_from_rows(arows, nB), csr_from_rows(brows, ncols), {"live": live}


def product_patterns():
    """name -> pattern case (no values yet).  expect: the route the case is written for."""
    c = {}
    # ---- the table tiers: the row with the most distinct columns on either side of every limit
    for name, target, nrows, bump, expect, shuf in [
            ("tier0_row_256", 256, 5, False, 0, False), ("tier1_row_257", 256, 5, True, 1, False),
            ("tier0_one_row_256", 256, 1, False, 0, True),
            ("tier1_row_2048", 2048, 7, False, 1, True), ("tier2_row_2049", 2048, 7, True, 2, True),
            ("tier1_one_row_2048", 2048, 1, False, 1, False),
            ("tier2_row_8192", 8192, 5, False, 2, False), ("refused_row_8193", 8192, 5, True, ROUTE_REFUSED, False),
            ("tier2_one_row_8192", 8192, 1, False, 2, True)]:
        A, B, _, info = _long_row_pattern(target, nrows, seed=target + nrows, bump=bump)   # (bump draws nothing: same case)
        c[name] = _product_case(expect, A, B, shuffled=shuf, seed=len(c), named_row=info["row"], named_count=target + int(bump),
                                hot=info["hot"], m=info["m"])
    # ---- a full table whose last column needs every probe the table has
    for tier, slots in enumerate(TIERS):
        A, B, info = _last_probe_pattern(slots, seed=50 + tier)
        c["tier%d_last_probe" % tier] = _product_case(tier, A, B, seed=len(c), named_row=info["row"], named_count=slots,
                                                      first=info["first"], last=info["last"])
    # ---- E, d, alpha, beta away from interp_smooth's combination, with E's own columns filling the table to its last slot
    for tier, target in ((0, 250), (1, 2040)):
        new = TIERS[tier] - target
        A, B, E, info = _long_row_pattern(target, 5 + 2 * tier, seed=77 + tier, e_new=new)
        common = dict(named_row=info["row"], hot=info["hot"], m=info["m"])
        c["tier%d_E_only" % tier] = _product_case(tier, A, B, E=E, alpha=1.0, beta=-2.0, shuffled=bool(tier), seed=len(c),
                                                  named_count=TIERS[tier], **common)
        c["tier%d_d_only" % tier] = _product_case(tier, A, B, d=True, alpha=0.5, seed=len(c), named_count=target, **common)
        c["tier%d_E_and_d" % tier] = _product_case(tier, A, B, E=E, d=True, alpha=0.5, beta=-2.0, shuffled=not tier, seed=len(c),
                                                   named_count=TIERS[tier], **common)
        # one more column of E: the next tier
        _, _, E1, _ = _long_row_pattern(target, 5 + 2 * tier, seed=77 + tier, e_new=new + 1)
        c["tier%d_E_one_more" % (tier + 1)] = _product_case(tier + 1, A, B, E=E1, alpha=0.5, beta=0.25, seed=len(c),
                                                            named_count=TIERS[tier] + 1, **common)
    # ---- E = B as the smoother calls it (A square)
    A, B, info = _square_alias_pattern(7, 250, 60, seed=5)
    c["tier0_E_is_B"] = _product_case(0, A, B, E="B", d=True, alpha=-0.5, beta=1.0, seed=len(c), named_row=info["row"])
    A, B, info = _square_alias_pattern(7, 1500, 290, seed=6)
    c["tier1_E_is_B"] = _product_case(1, A, B, E="B", d=True, alpha=-0.5, beta=1.0, shuffled=True, seed=len(c),
                                      named_row=info["row"])
    # ---- the dense-B product and its ineligible twins
    for ncols in (1, 255, 256, 257, 300, 2048):
        A, B, info = _dense_pattern(ncols, seed=ncols)
        c["dense_cols_%d" % ncols] = _product_case(ROUTE_DENSE, A, B, shuffled=ncols in (257, 300), seed=len(c), live=info["live"])
    lengths = (600, 0, 400, 280, 0)                        # 1280 = 256 * 5 entries
    A, B, info = _dense_pattern(300, seed=9, lengths=lengths)
    c["dense_nnz_256n"] = _product_case(ROUTE_DENSE, A, B, seed=len(c), live=info["live"])
    # the twins are made from the eligible case WITH its values (product_case): B with a 2049th column in every fifth row;
    # A without the last entry of its row 3.  Everything the change does not reach must come out as in the eligible case.
    c["hash_cols_2049"] = dict(kind="twin", expect=1, twin_of="dense_cols_2048", change="one_more_column")
    c["hash_nnz_256n_minus_1"] = dict(kind="twin", expect=0, twin_of="dense_nnz_256n", change="one_entry_less")
    # ---- no rows at all
    c["no_rows"] = _product_case(-1, csr_from_rows([], 4), csr_from_rows([np.array([0, 2])] * 4, 3), seed=len(c))
    return c


PATTERNS = product_patterns()


def product_case(name, family):
    """the operands of a pattern case with the family's values: dict(A, B, E, d, alpha, beta, expect, ...)"""
    pat = PATTERNS[name]
    if pat["kind"] == "twin":
        return _twin_case(pat, family)
    rng = np.random.default_rng(1000 * pat["seed"] + FAMILIES.index(family))
    A, B = with_values(pat["A"], family, rng), with_values(pat["B"], family, rng)
    E = pat["E"]
    if E is not None and not isinstance(E, str):
        E = with_values(E, family, rng)
    if pat["shuffled"]:
        A, B = shuffled_rows(A, rng), shuffled_rows(B, rng)
        if E is not None and not isinstance(E, str):
            E = shuffled_rows(E, rng)
    if isinstance(E, str):
        E = B                                     # the SAME object: capi.spgemm passes B's arrays twice
    d = None
    if pat["d"]:
        d = (2.0 ** rng.integers(-3, 4, size=A.shape[0])) if family == "exact" else rng.standard_normal(A.shape[0])
    alpha, beta = pat["alpha"], pat["beta"]
    if family == "general" and alpha != 1.0:
        alpha = ALPHA_SMOOTH * np.sign(alpha)
    if family == "general" and beta != 0.0:
        beta = beta * 0.3
    out = dict(pat)
    out.update(A=A, B=B, E=E, d=d, alpha=float(alpha), beta=float(beta), family=family)
    return out


def _twin_case(pat, family):
    out = dict(product_case(pat["twin_of"], family))
    A, B = out["A"], out["B"]
    if pat["change"] == "one_more_column":
        rng = np.random.default_rng(31 + FAMILIES.index(family))
        rows, vals = rows_of(B), [B.data[B.indptr[k]:B.indptr[k + 1]] for k in range(B.shape[0])]
        extra = with_values(csr_from_rows([np.array([0])] * B.shape[0], 1), family, rng).data
        for k in range(0, B.shape[0], 5):
            rows[k], vals[k] = np.concatenate([rows[k], [B.shape[1]]]), np.concatenate([vals[k], extra[k:k + 1]])
        out["B"] = csr_from_rows(rows, B.shape[1] + 1, np.concatenate(vals))
        out["same_rows"], out["same_cols"] = np.arange(A.shape[0]), B.shape[1]
    else:
        keep = np.ones(len(A.indices), dtype=bool)
        keep[A.indptr[4] - 1] = False
        indptr = A.indptr.copy()
        indptr[4:] -= 1
        out["A"] = sp.csr_matrix((A.data[keep], A.indices[keep], indptr), shape=A.shape)
        out["same_rows"], out["same_cols"] = np.array([0, 1, 2, 4]), B.shape[1]
    out.update(expect=pat["expect"], twin_of=pat["twin_of"])
    return out


def operands(case):
    return dict(E=case["E"], d=case["d"], alpha=case["alpha"], beta=case["beta"])


# ---------------------------------------------------------------------------------------------------------------------
# transpose cases
# ---------------------------------------------------------------------------------------------------------------------
def _special_values(v):
    """values whose bits a copy must not touch: negative zero, a denormal, huge and tiny magnitudes"""
    v = v.copy()
    if len(v) >= 5:
        v[:5] = [-0.0, 5e-324, -1.7e308, 2.2250738585072014e-308, 0.0]
    return v


def _column_length_matrix(nrows, lengths, seed, shuffled):
    """P (nrows x len(lengths)) whose column c has lengths[c] entries, on random rows"""
    rng = np.random.default_rng(seed)
    r = np.concatenate([rng.choice(nrows, size=l, replace=False) for l in lengths] + [np.zeros(0, np.int64)]).astype(np.int64)
    c = np.repeat(np.arange(len(lengths)), lengths)
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=nrows))]).astype(np.int32)
    P = sp.csr_matrix((_special_values(rng.standard_normal(len(r))), c.astype(np.int32), indptr), shape=(nrows, len(lengths)))
    return shuffled_rows(P, rng) if shuffled else P


TRANSPOSE_LENGTHS = (0, 0, 1, 2, 64, 0, 2047, 2048, 2049, 5000, 3, 0, 0)     # empty columns: start, middle, end


def transpose_cases():
    c = {}
    c["column_lengths"] = _column_length_matrix(5003, TRANSPOSE_LENGTHS, seed=1, shuffled=False)
    c["column_lengths_unsorted"] = _column_length_matrix(5003, TRANSPOSE_LENGTHS, seed=2, shuffled=True)
    c["small_unsorted"] = _column_length_matrix(37, (5, 0, 37, 1, 20, 36, 2), seed=3, shuffled=True)
    c["no_entries"] = csr_from_rows([np.zeros(0, np.int64)] * 5, 3)
    c["no_columns"] = csr_from_rows([np.zeros(0, np.int64)] * 4, 0)
    c["no_rows"] = csr_from_rows([], 3)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# threshold cases
# ---------------------------------------------------------------------------------------------------------------------
THRESHOLD_LENGTHS = (0, 1, 63, 64, 65, 128, 200)
TOL = 0.25


def _threshold_matrix(seed):
    """rows of THRESHOLD_LENGTHS entries with normal values (some exactly +tol or -tol), then a row of 70 entries all at or
    below tol in magnitude, a row of 130 all above, and a row of 66 alternating +tol, -tol and 1: 10 rows, unsorted"""
    rng = np.random.default_rng(seed)
    ncols = 260
    rows, vals = [], []
    for l in THRESHOLD_LENGTHS:
        rows.append(rng.choice(ncols, size=l, replace=False))
        v = rng.standard_normal(l) * 0.4
        v[rng.random(l) < 0.15] = TOL
        v[rng.random(l) < 0.15] = -TOL
        vals.append(v)
    rows.append(rng.choice(ncols, size=70, replace=False))
    v = rng.uniform(-TOL, TOL, size=70)
    v[::7], v[3::7] = TOL, -TOL
    vals.append(v)
    rows.append(rng.choice(ncols, size=130, replace=False))
    vals.append((TOL + rng.uniform(1e-3, 2.0, size=130)) * rng.choice([-1.0, 1.0], size=130))
    vals[-1][64] = np.nextafter(TOL, 1.0)          # the smallest value that is kept, in the second chunk
    rows.append(rng.choice(ncols, size=66, replace=False))
    vals.append(np.tile([TOL, -TOL, 1.0], 22))
    return csr_from_rows(rows, ncols, np.concatenate(vals))


def threshold_cases():
    """name -> (A, tol)"""
    c = {}
    A = _threshold_matrix(4)
    c["chunks"] = (A, TOL)
    Z = A.copy()
    Z.data[::3], Z.data[1::5] = 0.0, -0.0
    Z.data[2] = 5e-324
    c["tol_zero_explicit_zeros"] = (Z, 0.0)
    c["everything_dropped"] = (A, 1e300)
    c["nothing_dropped_negative_tol"] = (Z, -1.0)
    c["one_row_of_129"] = (csr_from_rows([np.arange(129)[::-1]], 129, np.where(np.arange(129) % 2 == 0, 1.0, TOL)), TOL)
    c["no_rows"] = (csr_from_rows([], 7), TOL)
    return c
