"""Matrices and runs of the block SpMV tests (not a test module; tests/test_gpu_spmv_block.py runs `child_main` in child
processes, one per setting of the library's options).

The claim is exact: every column of saamge_amd_spmv_block carries the bits capi.spmv gives for that column alone, on every
path the block call can take --

    square matrices with spmv_sell = 1   the SELL copy: sell_block_kernel over pair-coded, offset-coded and plain slices
                                         (the single call runs the staged kernels, sell_slice or sell_row_general)
    the same with spmv_sell = 0, and     the CSR path, spmv_block_kernel<L, .>: one rectangular matrix per value of
    every rectangular matrix             lanes_per_row that pick_lanes_per_row (csrc/common.h) can choose
    the Q2-elasticity operator           the operator-level dictionary: column by column through the single launcher

pick_lanes_per_row doubles L from 1 while 2 L <= 0.75 avg + 1 (avg = entries per row), up to 64:
    L = 1: avg < 4/3   2: < 4   4: < 28/3   8: < 20   16: < 124/3   32: < 84   64: otherwise
"""
import numpy as np
import scipy.sparse as sp

from saamge_amd import problems as pr

KS = (1, 2, 3, 5, 8, 9, 17)
KMAX = max(KS)
LD_PAD = 5
P_SHAPE = (2730, 1058)          # rows: 42 slices and 42 rows, no multiple of 64
# average entries per row of the rectangular matrices -> the lanes_per_row each must get
P_AVG = {1: 1.0, 2: 3.0, 4: 6.0, 8: 14.0, 16: 30.0, 32: 60.0, 64: 100.0}


def lanes_per_row(nnz, nrows):
    """pick_lanes_per_row of csrc/common.h"""
    avg = float(nnz) / nrows if nrows else 1.0
    lanes = 1
    while lanes < 64 and lanes * 2 <= avg * 0.75 + 1.0:
        lanes *= 2
    return lanes


def p_shaped(lanes, seed=0):
    """A P-shaped matrix whose average row length selects `lanes`: row lengths scattered around the average, every 13th row
    empty, one row several times the average (more than one pass of the L lanes)."""
    nrows, ncols = P_SHAPE
    rng = np.random.default_rng(100 + lanes + seed)
    avg = P_AVG[lanes]
    counts = rng.integers(max(int(avg * 0.5), 1), int(avg * 1.5) + 2, size=nrows)
    counts[::13] = 0
    counts[7] = min(ncols, int(avg * 5) + 3)
    # bring the total back to the wanted average (the empty rows took some away)
    want = int(round(avg * nrows))
    live = np.nonzero(counts)[0]
    i = 0
    while counts.sum() < want:
        counts[live[i % live.size]] += 1
        i += 1
    while counts.sum() > want:
        r = live[i % live.size]
        if counts[r] > 1:
            counts[r] -= 1
        i += 1
    indptr = np.r_[0, np.cumsum(counts)]
    indices = np.concatenate([np.sort(rng.choice(ncols, size=c, replace=False)) for c in counts if c] or [np.zeros(0, int)])
    data = rng.standard_normal(indices.size)
    A = sp.csr_matrix((data, indices.astype(np.int32), indptr.astype(np.int32)), shape=P_SHAPE)
    assert lanes_per_row(A.nnz, nrows) == lanes, (lanes, A.nnz / nrows)
    return A


def sell_matrices():
    """the seven matrices of tests/test_gpu_sell.py"""
    rng = np.random.default_rng(3)
    return {
        "stencil_const_short_rows": pr.poisson3d_problem((8, 8, 8), blk=(4, 4, 2)).A.tocsr(),
        "stencil_const": pr.poisson3d_problem((20, 12, 9), blk=(4, 4, 3)).A.tocsr(),
        "stencil_skew": pr.poisson3d_problem((12, 12, 12), blk=(4, 4, 4), coef="skew").A.tocsr(),
        "random": sp.random(1000, 1000, density=0.02, random_state=rng, format="csr"),
        "toeplitz_wide_band": sp.diags([np.full(6000 - abs(o), 1.0 + 0.01 * j) for j, o in enumerate(range(-600, 600, 40))],
                                       list(range(-600, 600, 40)), format="csr"),
        "stencil_2d": (sp.kron(sp.diags([1.0, 2.0, 1.0], [-1, 0, 1], shape=(40, 40)),
                               sp.diags([1.0, -4.0, 1.0], [-1, 0, 1], shape=(300, 300)))).tocsr(),
        "tiny": sp.csr_matrix(np.array([[2.0, -1.0, 0.0], [-1.0, 2.0, -1.0], [0.0, -1.0, 2.0]])),
    }


def matrices(which):
    if which == "dict":
        return {"elasticity_q2_10": pr.elasticity3d_q2_problem((10, 10, 10), blk=(2, 2, 2)).A.tocsr()}
    mats = sell_matrices()
    for lanes in P_AVG:
        mats["p_shaped_L%d" % lanes] = p_shaped(lanes)
    return mats


def check_matrix(capi, name, A):
    """every k and both leading dimensions against capi.spmv per column; returns the number of block calls made"""
    A = A.tocsr()
    A.sort_indices()
    nrows, ncols = A.shape
    rng = np.random.default_rng(17)
    X = rng.standard_normal((KMAX, ncols))
    ref = np.stack([capi.spmv(A, X[j].copy()) for j in range(KMAX)])       # the single-vector call, once per column
    calls = 0
    for k in KS:
        for pad in (0, LD_PAD):
            Xb = np.full((k, ncols + pad), np.nan)
            Xb[:, :ncols] = X[:k]
            Yb = np.full((k, nrows + pad), np.nan)
            capi.spmv_block(A, Xb, Yb)
            calls += 1
            for j in range(k):
                assert Yb[j, :nrows].tobytes() == ref[j].tobytes(), (name, k, pad, j)
            assert np.all(np.isnan(Yb[:, nrows:])), (name, k, pad, "padding rows of Y were written")
            assert np.array_equal(Xb[:, :ncols], X[:k]) and np.all(np.isnan(Xb[:, ncols:])), (name, k, pad, "X changed")
    return calls


def child_main(which):
    from saamge_amd import capi
    total = 0
    for name, A in matrices(which).items():
        total += check_matrix(capi, name, A)
        print("OK", name, flush=True)
    print("DONE", total)
