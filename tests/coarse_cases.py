"""Operators, a host model of the block structure and a high-precision reference for the tests of the coarsest-level
direct solvers (not a test module).

Every case is a fine matrix for the element-free mode (`Hierarchy.from_matrix`, params.algebraic = 1) together with a map
dof -> agglomerate.  The fine graph is the wanted AGGLOMERATE graph blown up: agglomerate a owns a short chain of 2 or 3 dofs,
and an edge (a, b) of the agglomerate graph joins the first dofs of the two chains.  The local matrix of an agglomerate is the
Laplacian of its chain (connected: one zero eigenvalue, the next one >= 1/2 in the diagonal scaling), so a tiny theta keeps
exactly one vector per agglomerate, P is piecewise constant with orthonormal columns, and the graph of Ac = P^T A P is the
agglomerate graph.  This is what the cases EXPECT; the GPU tests assert it on the operator the library returns.

    A = L + shift * diag(L),      L the weighted graph Laplacian of the fine graph

`shift` = 0.1 gives cond(Ac) of about 20 ("well": the one refinement step of the direct solvers squares the relative error of
a factor, and the couplings must not be so weak that a wrong factor disappears in that square), 1e-6 a stiff operator, 0 a
singular one.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.sparse.csgraph import connected_components

BT_MAX_BLOCK = 12288      # blocktri.hip
BT_MIN_BLOCK = 256
DNB = 64                  # dense.hip: columns per step of the block Gauss-Jordan elimination
DENSE_MAX = 16384         # cycle.hip: the largest operator that gets one explicit dense inverse


# ---------------------------------------------------------------------------------------------------------------------
# agglomerate graphs: (n, edges) with edges an (m, 2) array, each undirected edge once
# ---------------------------------------------------------------------------------------------------------------------
def grid_graph(nx, ny=1, nz=1, king=False):
    """7-point grid; king: 27-point (every neighbour of the surrounding 3 x 3 x 3 box, the graph of a coarse operator whose
    agglomerates share faces, edges and corners: breadth-first levels are then shells and planes, not diagonal slices)"""
    idx = np.arange(nx * ny * nz).reshape(nx, ny, nz)
    if not king:
        e = [np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1), np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1),
             np.stack([idx[:, :, :-1].ravel(), idx[:, :, 1:].ravel()], 1)]
        return idx.size, np.concatenate(e).astype(np.int64)
    e = []
    for dx, dy, dz in [(a, b, c) for a in (0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) > (0, 0, 0)]:
        def sl(d, n):
            return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
        (ax, bx), (ay, by), (az, bz) = sl(dx, nx), sl(dy, ny), sl(dz, nz)
        e.append(np.stack([idx[ax, ay, az].ravel(), idx[bx, by, bz].ravel()], 1))
    return idx.size, np.concatenate(e).astype(np.int64)


def star_graph(n):
    """vertex 0 adjacent to every other one"""
    return n, np.stack([np.zeros(n - 1, np.int64), np.arange(1, n, dtype=np.int64)], 1)


def tree_graph(branching, depth):
    """the complete tree: vertex v > 0 hangs off (v - 1) // branching; branching ** depth leaves"""
    n = (branching ** (depth + 1) - 1) // (branching - 1)
    v = np.arange(1, n, dtype=np.int64)
    return n, np.stack([(v - 1) // branching, v], 1)


def with_pendant(g):
    """one more vertex, hanging off the last one (a vertex count no grid gives)"""
    n, e = g
    return n + 1, np.concatenate([e, [[n - 1, n]]]).astype(np.int64)


def disjoint_union(*graphs):
    off, es = 0, []
    for n, e in graphs:
        es.append(e + off)
        off += n
    return off, np.concatenate(es).astype(np.int64).reshape(-1, 2)


def renumbered(g, seed):
    n, e = g
    p = np.random.default_rng(seed).permutation(n)
    return n, p[e]


def graph_laplacian(n, edges, shift, weights=None):
    """L + shift diag(L) as CSR with sorted columns; an isolated vertex gets the diagonal 1 + shift"""
    w = np.ones(len(edges)) if weights is None else np.asarray(weights, dtype=np.float64)
    i, j = edges[:, 0], edges[:, 1]
    W = sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n)).tocsr()
    d = np.asarray(W.sum(axis=1)).ravel()
    d[d == 0.0] = 1.0
    A = (sp.diags(d * (1.0 + shift)) - W).tocsr()
    A.sort_indices()
    return A


def blow_up(g, shift, seed=None):
    """(A, dof_partition): the fine operator whose agglomerate graph is g.  Agglomerate a = a chain of 2 + a % 2 dofs, the
    edge (a, b) joins their first dofs with weight 1 + 0.5 cos(a + b) (no two rows of Ac alike).  seed: the dofs are
    renumbered at random as well."""
    n, edges = g
    size = 2 + np.arange(n) % 2
    first = np.concatenate([[0], np.cumsum(size)])
    nf = int(first[-1])
    part = np.repeat(np.arange(n), size)
    chain = np.setdiff1d(np.arange(nf - 1), first[1:-1] - 1)              # (d, d + 1) inside one agglomerate
    fe = np.concatenate([np.stack([chain, chain + 1], 1), first[edges]]) if len(edges) else np.stack([chain, chain + 1], 1)
    fw = np.concatenate([np.ones(len(chain)), 1.0 + 0.5 * np.cos(edges.sum(axis=1))]) if len(edges) else np.ones(len(chain))
    if seed is not None:
        p = np.random.default_rng(seed).permutation(nf)                   # old dof d becomes p[d]
        fe = p[fe]
        newpart = np.empty(nf, dtype=np.int64)
        newpart[p] = part
        part = newpart
    return graph_laplacian(nf, fe, shift, fw), part.astype(np.int32)


def expected_coarse_operator(g, shift):
    """What Ac should be up to the signs of P's columns (which change no magnitude and no pattern): P^T A P for the
    piecewise constant orthonormal P.  The CPU checks of the cases run on this."""
    A, part = blow_up(g, shift)
    n = g[0]
    cnt = np.bincount(part, minlength=n)
    P = sp.csr_matrix((1.0 / np.sqrt(cnt[part]), (np.arange(A.shape[0]), part)), shape=(A.shape[0], n))
    Ac = (P.T @ A @ P).tocsr()
    Ac.sort_indices()
    return Ac


# ---------------------------------------------------------------------------------------------------------------------
# the case catalogue
# ---------------------------------------------------------------------------------------------------------------------
WELL, STIFF = 0.1, 1e-6


def _case(graph, shift=WELL, seed=None, components=1, kinds=(1, 3), expect=None):
    return {"graph": graph, "shift": shift, "seed": seed, "components": components, "kinds": kinds, "expect": expect or {}}


def _dense_edge_graph(nc):
    """a 3-D grid where nc factors, a 2-D grid or a path otherwise"""
    shapes = {DNB - 1: (3, 3, 7), DNB: (4, 4, 4), DNB + 1: (5, 13), 2 * DNB - 1: (127,), 2 * DNB + 1: (3, 43),
              3 * DNB + 5: (197,), 1000: (10, 10, 10), 4097: (17, 241)}
    g = grid_graph(*shapes[nc])
    assert g[0] == nc
    return g


def catalogue():
    """name -> case.  `expect` holds what the case is meant to reach, in terms of the model: nblk, max_block, refused,
    far_wins, min_levels."""
    c = {}
    c["one_row"] = _case(grid_graph(1), expect={"nblk": 1, "max_block": 1})
    c["two_rows"] = _case(grid_graph(2), expect={"nblk": 1, "max_block": 2})
    c["small_grid_255"] = _case(grid_graph(15, 17), expect={"nblk": 1, "max_block": 255})
    # 16 x 16: the anti-diagonals of a corner search reach 256 rows only with the last one: one block of exactly BT_MIN_BLOCK
    c["small_grid_256"] = _case(grid_graph(16, 16), expect={"nblk": 1, "max_block": 256})
    # 257 is prime: the 16 x 16 grid and one pendant vertex.  The search starts AT the pendant vertex (smallest degree), the
    # far corner's one-row level is the merged tail
    c["small_grid_257"] = _case(with_pendant(grid_graph(16, 16)), expect={"nblk": 1, "max_block": 257})
    # (the first split needs two runs of levels of 256 rows each; the anti-diagonals of 16 x 40 give blocks of 264 and 376)
    c["small_grid_640"] = _case(grid_graph(16, 40), expect={"nblk": 2, "max_block": 376})
    for nc in (DNB - 1, DNB, DNB + 1, 2 * DNB - 1, 2 * DNB + 1, 3 * DNB + 5, 1000, 4097):
        c["dense_edges_%d" % nc] = _case(_dense_edge_graph(nc))
    # 3000 one-row levels in blocks of 256 and a tail of 184 merged into the last one: 11 blocks, the last of 440
    c["path"] = _case(grid_graph(3000), expect={"nblk": 11, "max_block": 440, "min_levels": 3000})
    c["rod"] = _case(grid_graph(4, 4, 600), expect={"min_levels": 600})
    c["rod_stiff"] = _case(grid_graph(4, 4, 600), shift=STIFF, expect={"min_levels": 600})
    # 80 x 60 x 3 with 27-point coupling, 14 400 rows (80 x 80 x 3 = 19 200 would be beyond one dense inverse, and every case
    # but too_wide is to run both kinds; on a SQUARE slab, and on any 7-point grid, the far end of a corner search is no
    # better a start than the corner, the model shows equal costs): the far end is the whole 60 x 3 face, planes of 180 rows
    # (merged in pairs) beat the L-shaped shells around a corner
    c["slab"] = _case(grid_graph(80, 60, 3, king=True), expect={"far_wins": True, "nblk": 40, "max_block": 360})
    # 24 x 24 x 26 with 27-point coupling: a true cube has the three far faces as its far end, i.e. shells again and never
    # planes; two more layers make the far end one 24 x 24 face and the levels 26 planes of 576 rows
    c["cube"] = _case(grid_graph(24, 24, 26, king=True), expect={"far_wins": True, "nblk": 26, "max_block": 576})
    c["cube_stiff"] = _case(grid_graph(24, 24, 26, king=True), shift=STIFF, expect={"far_wins": True, "nblk": 26})
    c["two_components"] = _case(disjoint_union(grid_graph(30, 50), grid_graph(700)), components=2)
    # 1500 + 700 + 5 agglomerates: the five-row component is smaller than a block and shares one with rows of another
    c["three_components_uneven"] = _case(disjoint_union(grid_graph(30, 50), grid_graph(700), grid_graph(5)), components=3)
    # 1500 and not 5000 agglomerates: the Galerkin product keeps the neighbours of an agglomerate in a table of 2048 slots and
    # refuses a coarse row beyond that ("RAP: MIS neighbour table overflow"), so no hub can have more neighbours
    c["star"] = _case(star_graph(1500), expect={"nblk": 1, "max_block": 1500})
    c["permuted_cube"] = _case(renumbered(grid_graph(24, 24, 26, king=True), 7), seed=11, expect={"far_wins": True, "nblk": 26})
    # No hub graph: a coarse row cannot have n_c > 3 * 12288 entries (see `star`).  The complete 7-ary tree of depth 5 instead
    # (19 608 rows, degree <= 8): seen from a leaf the 6 * 7^4 = 14 406 leaves under the other children of the root are ONE
    # level, and they are the far end too, so both candidate structures hold a block above BT_MAX_BLOCK
    c["too_wide"] = _case(tree_graph(7, 5), kinds=(3,), expect={"refused": True})
    c["semidefinite"] = _case(grid_graph(20, 30), shift=0.0)
    c["updated"] = _case(grid_graph(24, 24, 26, king=True), expect={"nblk": 26, "max_block": 576})
    return c


def build(case):
    """(A, dof_partition) of a catalogue entry"""
    return blow_up(case["graph"], case["shift"], case["seed"])


# ---------------------------------------------------------------------------------------------------------------------
# host model of the integer part of blocktri_factor (from the header comment of blocktri.hip and its three rules: levels
# of a breadth-first search, unreached vertices continue the numbering from the smallest unreached index; small neighbouring
# levels are merged until a block has BT_MIN_BLOCK rows, a short tail joins the last block; no block above BT_MAX_BLOCK)
# ---------------------------------------------------------------------------------------------------------------------
def _bfs_levels(indptr, indices, start):
    n = len(indptr) - 1
    lev = [-1] * n
    order = []
    for v in start:
        if lev[v] < 0:
            lev[v] = 0
            order.append(v)
    top, head, seed = -1, 0, 0
    while True:
        while head < len(order):
            u = order[head]
            head += 1
            lu = lev[u]
            if lu > top:
                top = lu
            for v in indices[indptr[u]:indptr[u + 1]]:
                if lev[v] < 0:
                    lev[v] = lu + 1
                    order.append(v)
        while seed < n and lev[seed] >= 0:
            seed += 1
        if seed >= n:
            break
        lev[seed] = top + 1           # another connected component: nothing couples it to the levels so far
        order.append(seed)
    return top + 1, np.asarray(lev), order


def _cost(nlev, lev):
    sizes = np.bincount(lev, minlength=nlev)
    return float(np.sum(sizes.astype(np.float64) ** 3)), sizes


def level_blocks(Ac):
    """The block-tridiagonal structure blocktri_factor chooses for the operator Ac (pattern only):
    {refused, nblk, max_block, off, block (per row), perm, nlev, cost_vertex, cost_far, far_wins}."""
    Ac = sp.csr_matrix(Ac)
    n = Ac.shape[0]
    indptr, indices = Ac.indptr.tolist(), Ac.indices.tolist()
    deg = np.diff(Ac.indptr)
    nlev, lev, order = _bfs_levels(indptr, indices, [0])
    best = order[-1]                  # smallest degree in the last level; among equals the one reached last
    for v in reversed(order):
        if lev[v] != nlev - 1:
            break
        if deg[v] < deg[best]:
            best = v
    nlev, lev, order = _bfs_levels(indptr, indices, [best])
    cost, sizes = _cost(nlev, lev)
    far = np.nonzero(lev == nlev - 1)[0].tolist()
    nlev2, lev2, _ = _bfs_levels(indptr, indices, far)
    cost2, sizes2 = _cost(nlev2, lev2)
    far_wins = cost2 < cost
    if far_wins:
        nlev, lev, sizes = nlev2, lev2, sizes2
    blk_of_lev = np.zeros(nlev, dtype=np.int64)
    nblk = acc = 0
    for l in range(nlev):
        blk_of_lev[l] = nblk
        acc += int(sizes[l])
        if acc >= BT_MIN_BLOCK:
            nblk += 1
            acc = 0
    if acc > 0:
        if nblk > 0:
            blk_of_lev[blk_of_lev == nblk] = nblk - 1
        else:
            nblk = 1
    block = blk_of_lev[lev]
    bsz = np.bincount(block, minlength=nblk)
    off = np.concatenate([[0], np.cumsum(bsz)])
    perm = np.argsort(block, kind="stable")            # ascending original index inside a block
    out = {"refused": bool(bsz.max() > BT_MAX_BLOCK), "nblk": int(nblk), "max_block": int(bsz.max()), "off": off,
           "block": block, "perm": perm, "nlev": int(nlev), "level_sizes": sizes, "cost_vertex": cost, "cost_far": cost2,
           "far_wins": bool(far_wins)}
    return out


def check_block_tridiagonal(Ac, lb):
    """no entry couples blocks more than one apart; sizes within the limits; every block but a lone one has BT_MIN_BLOCK rows"""
    Ac = sp.coo_matrix(Ac)
    b = lb["block"]
    assert np.abs(b[Ac.row] - b[Ac.col]).max() <= 1, "an entry couples blocks more than one apart"
    bsz = np.diff(lb["off"])
    assert bsz.sum() == Ac.shape[0] and bsz.min() >= 1
    assert lb["nblk"] == 1 or bsz.min() >= BT_MIN_BLOCK, bsz
    assert lb["refused"] == (bsz.max() > BT_MAX_BLOCK)
    assert np.array_equal(np.sort(lb["perm"]), np.arange(Ac.shape[0]))


def num_components(Ac):
    return int(connected_components(sp.csr_matrix(Ac), directed=False)[0])


# ---------------------------------------------------------------------------------------------------------------------
# extended-precision residuals and the reference solve
# ---------------------------------------------------------------------------------------------------------------------
HAVE_LONGDOUBLE = bool(np.finfo(np.longdouble).eps < 1e-18)


def _row_sums(terms, indptr):
    """sums of consecutive runs of `terms` (any dtype) delimited by indptr; an empty row sums to 0"""
    n = len(indptr) - 1
    out = np.zeros(n, dtype=terms.dtype)
    nz = np.nonzero(np.diff(indptr) > 0)[0]
    if nz.size:
        out[nz] = np.add.reduceat(terms, indptr[nz])
    return out


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a                # 2^27 + 1 (Dekker / Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _residual_dd(A, x, b):
    """b - A x with error-free products and a double-double accumulator per row: (hi, lo) arrays"""
    A = sp.csr_matrix(A)
    indptr = A.indptr
    n = A.shape[0]
    p, e = _two_prod(-A.data, x[A.indices])
    hi, lo = np.array(b, dtype=np.float64), np.zeros(n)
    length = np.diff(indptr)
    for k in range(int(length.max()) if n else 0):       # the k-th entry of every row that has one
        rows = np.nonzero(length > k)[0]
        pos = indptr[rows] + k
        s, t = _two_sum(hi[rows], p[pos])
        t = t + (lo[rows] + e[pos])
        hi[rows], lo[rows] = _two_sum(s, t)
    return hi, lo


def residual_ext(A, x, b, force_dd=False):
    """b - A x, the products and sums carried in extended precision (x87 long double where it has a 64-bit significand,
    double-double otherwise), rounded to fp64 at the end"""
    A = sp.csr_matrix(A)
    if HAVE_LONGDOUBLE and not force_dd:
        ld = np.longdouble
        terms = A.data.astype(ld) * np.asarray(x, dtype=ld)[A.indices]
        return (np.asarray(b, dtype=ld) - _row_sums(terms, A.indptr)).astype(np.float64)
    hi, lo = _residual_dd(A, np.asarray(x, dtype=np.float64), b)
    return hi + lo


def matvec_ext(A, x):
    return -residual_ext(A, x, np.zeros(sp.csr_matrix(A).shape[0]))


def norm_inf_op(A):
    return float(abs(sp.csr_matrix(A)).sum(axis=1).max())


def backward_error(A, x, b):
    """normwise backward error || b - A x ||_inf / (|| A ||_inf || x ||_inf + || b ||_inf), residual in extended precision"""
    r = residual_ext(A, x, b)
    return float(np.abs(r).max() / (norm_inf_op(A) * np.abs(x).max() + np.abs(b).max()))


def forward_error(x, x_ref):
    return float(np.abs(x - x_ref).max() / np.abs(x_ref).max())


def factor(A):
    """fp64 sparse LU (SuperLU), shared by reference_solve, lu_shaped_solve and cond_estimate"""
    return spla.splu(sp.csc_matrix(A))


def reference_solve(A, b, max_steps=40, lu=None):
    """x_ref of A x = b: fp64 sparse LU and iterative refinement on extended-precision residuals until the correction stops
    shrinking.  x_ref is kept as an unevaluated sum of two fp64 vectors (head, tail), so that it is good to well below fp64
    round-off.  Returns (head, tail, res): res = || b - A x_ref ||_inf / (|| A ||_inf || x_ref ||_inf + || b ||_inf)."""
    Ar = sp.csr_matrix(A)
    lu = lu or factor(A)
    b = np.asarray(b, dtype=np.float64)
    head = lu.solve(b)
    tail = np.zeros_like(head)
    # long double residuals first (fast), then double-double ones: cond(A) times the long double round-off is not two
    # orders below what a stiff case is judged with
    for dd in ([False, True] if HAVE_LONGDOUBLE else [True]):
        last = np.inf
        for _ in range(max_steps):
            # residual of head + tail: b - A head in extended precision, minus A tail (tail is tiny: fp64 suffices)
            r = residual_ext(Ar, head, b, force_dd=dd) - Ar @ tail
            d = lu.solve(r)
            step = float(np.abs(d).max())
            if not step < last:
                break
            last = step
            head, tail = _two_sum(head, tail + d)
            if step == 0.0:
                break
    r = residual_ext(Ar, head, b, force_dd=True) - Ar @ tail
    res = float(np.abs(r).max() / (norm_inf_op(Ar) * np.abs(head).max() + np.abs(b).max()))
    return head, tail, res


def lu_shaped_solve(A, b, lu=None):
    """The algorithmic shape of the code under test on the host: plain fp64 LU solve and ONE fp64 refinement step"""
    A = sp.csr_matrix(A)
    lu = lu or factor(A)
    x = lu.solve(b)
    return x + lu.solve(b - A @ x)


def cond_estimate(A, lu=None):
    """|| A ||_1 || A^-1 ||_1, the second factor by the LU factors and Hager's estimator (scipy onenormest)"""
    A = sp.csc_matrix(A)
    if A.shape[0] <= 2:
        return float(np.linalg.cond(A.toarray(), 1))
    lu = lu or factor(A)
    inv = spla.LinearOperator(A.shape, matvec=lu.solve, rmatvec=lambda v: lu.solve(v, "T"), dtype=np.float64)
    return float(spla.onenormest(A) * spla.onenormest(inv))


def right_hand_sides(Ac, lb, seed=0):
    """name -> rc: a random vector, Ac times a smooth vector, a unit vector in the last block of the model"""
    n = Ac.shape[0]
    rng = np.random.default_rng(seed)
    smooth = 1.0 + np.cos(np.arange(n) * (2.0 * np.pi / max(n, 2)))
    unit = np.zeros(n)
    unit[lb["perm"][-1]] = 1.0
    return {"random": rng.standard_normal(n), "smooth": sp.csr_matrix(Ac) @ smooth, "unit_last": unit}
