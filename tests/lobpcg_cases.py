"""Cases, references and bounds of the eigensolver tests (not a test module): tests/test_lobpcg_model.py holds the numpy
model to them, tests/test_gpu_lobpcg.py and tests/test_cxx_lobpcg.py the device.

The reference is scipy.linalg.eigh on the free-dof submatrices, with vectors.  Every bound is a theorem:

    eigenvalues   for x with ||x||_M = 1 and any theta an eigenvalue lies within beta = ||A x - theta M x||_{M^-1} of theta;
                  the same for the reference's own pairs gives beta_ref, so |theta_j - lambda_ref,j| <= beta_j + beta_ref,j
                  as long as both intervals single out the same eigenvalue: beta_j + beta_ref,j is asserted to stay below a
                  tenth of the smallest gap between the distinct reference eigenvalues involved.
    vectors       Davis-Kahan: ||(I - V_c V_c^T M) x_j||_M <= beta_j / gap_j, V_c the reference basis of the whole cluster
                  of lambda_j and gap_j the distance of the cluster (and of theta_j) to the rest of the reference spectrum;
                  for a whole cluster the smallest singular value of V_c^T M X_c is at least 1/2 (independent vectors
                  give nearly 1, dependent ones nearly 0).
"""
import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from saamge_amd import problems as pr

import solve_cases as sc

TOL = 1e-8
MAX_ITER = 80
CLUSTER_REL = 1e-8          # reference eigenvalues closer than this (relative) are one cluster: the distinct ones are 6e-3 apart

PROBLEMS = {
    "skew3": (lambda: sc.problem("skew3"), 2),
    "tiles": (lambda: sc.problem("tiles"), 1),
    "cube8": (lambda: pr.poisson3d_problem((8, 8, 8), blk=(4, 4, 4)), 1),
    "elast": (lambda: pr.elasticity3d_problem(4, blk=(2, 2, 2)), 1),
}
ROWS = {"skew3": (2601, 1026), "tiles": (2730, 1058), "cube8": (729, 386), "elast": (375, 75)}
# (case, mass, nev, nb, constrained)
# skew3 with the mass at (8, 8) takes the model 43 iterations (the ninth eigenvalue is close and the block has no guard
# column): beyond the 40 a case may need, so that one runs with two guard columns.  Likewise five pairs of tiles: the sixth
# eigenvalue 0.037709 lies 1.6 % above the fifth, (5, 5) takes 63 iterations (77 with the mass), (5, 7) takes 21.
TABLE = ([("skew3", m, nev, nb if (m, nev, nb) != ("q1", 8, 8) else 10, True)
          for m in (None, "q1") for nev, nb in ((1, 1), (3, 5), (8, 8), (4, 16))]
         + [("tiles", m, nev, nb, True) for m in (None, "q1") for nev, nb in ((4, 4), (5, 7))]
         + [("tiles", None, 5, 7, False),
            ("cube8", None, 4, 4, True), ("cube8", None, 3, 3, True),
            ("elast", None, 3, 6, True)])


def case_id(c):
    return "%s-%s-%d-%d%s" % (c[0], c[1] or "I", c[2], c[3], "" if c[4] else "-free")


@functools.lru_cache(maxsize=None)
def problem(name):
    return PROBLEMS[name][0]()


def coarsenings(name):
    return PROBLEMS[name][1]


@functools.lru_cache(maxsize=None)
def oracle_hierarchy(name):
    from oracle import saamge_oracle as o
    p = problem(name)
    return o.ml_produce_data(p.A, p.elem_to_dof, p.elmat, p.bdr, p.partitions[:coarsenings(name)], theta=sc.THETA)


def oracle_prec(name):
    from oracle import saamge_oracle as o
    H = oracle_hierarchy(name)
    return lambda r: o.vcycle(H, r)


def params(name):
    from saamge_amd import capi
    return capi.default_params(num_coarsenings=coarsenings(name), theta=sc.THETA)


def _mass_1d(ne):
    h = 1.0 / ne
    m = sp.diags([np.full(ne, h / 6.0), np.r_[h / 3.0, np.full(ne - 1, 2.0 * h / 3.0), h / 3.0], np.full(ne, h / 6.0)],
                 [-1, 0, 1])
    return sp.csr_matrix(m)


@functools.lru_cache(maxsize=None)
def mass(name, kind):
    """None (the identity) or the Q1 mass of the case's grid: the Kronecker product of the 1-D mass matrices (x fastest,
    like the dof numbering), essential rows and columns eliminated with the diagonal kept, like A"""
    if kind is None:
        return None
    assert kind == "q1"
    p = problem(name)
    nx, ny, nz = p.dims
    M = sp.csr_matrix(sp.kron(_mass_1d(nz), sp.kron(_mass_1d(ny), _mass_1d(nx))))
    ess = np.asarray(p.ess, dtype=bool)
    M = sp.coo_matrix(M)
    keep = ~((ess[M.row] | ess[M.col]) & (M.row != M.col))
    M = sp.csr_matrix((M.data[keep], (M.row[keep], M.col[keep])), shape=M.shape)
    M.sort_indices()
    return M


def start_block(name, nb, seed=11):
    return np.random.default_rng(seed).standard_normal((problem(name).A.shape[0], nb))


class Reference(object):
    """eigh of the pencil on the rows `free`, ascending, M-orthonormal vectors; clusters of equal eigenvalues"""

    def __init__(self, A, M, free):
        self.free = free
        self.A = sp.csr_matrix(A)[free][:, free].toarray()
        self.M = np.eye(self.A.shape[0]) if M is None else sp.csr_matrix(M)[free][:, free].toarray()
        self.lam, self.V = sla.eigh(self.A, self.M)
        self.Mchol = sla.cho_factor(self.M)
        first = np.r_[True, np.diff(self.lam) > CLUSTER_REL * self.lam[1:]]
        self.cluster = np.cumsum(first) - 1

    def beta(self, theta, x):
        """||A x - theta M x||_{M^-1} / ||x||_M for x on the free rows"""
        r = self.A @ x - theta * (self.M @ x)
        return float(np.sqrt(r @ sla.cho_solve(self.Mchol, r)) / np.sqrt(x @ (self.M @ x)))

    def members(self, j):
        return np.nonzero(self.cluster == self.cluster[j])[0]


@functools.lru_cache(maxsize=None)
def reference(name, kind, constrained=True):
    p = problem(name)
    n = p.A.shape[0]
    free = np.nonzero(~np.asarray(p.ess, dtype=bool))[0] if constrained else np.arange(n)
    return Reference(p.A, mass(name, kind), free)


def check_pairs(ref, lam, X, out=None):
    """hold the returned pairs (lam ascending by column, X on all rows) to the bounds of the module docstring; returns the
    largest |theta - lambda_ref| / (beta + beta_ref)"""
    lam = np.asarray(lam, dtype=np.float64)
    nev = lam.size
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(X))
    order = np.argsort(lam, kind="stable")
    Xf = np.asarray(X)[ref.free][:, order]
    lam = lam[order]
    rest = np.setdiff1d(np.arange(X.shape[0]), ref.free)
    assert not np.any(np.asarray(X)[rest]), "the constrained rows are not zero"
    involved = ref.lam[:ref.members(nev - 1)[-1] + 2]
    d = np.diff(involved)
    min_gap = float(np.min(d[d > CLUSTER_REL * involved[1:]]))
    worst = 0.0
    betas = []
    for j in range(nev):
        b = ref.beta(lam[j], Xf[:, j])
        b_ref = ref.beta(ref.lam[j], ref.V[:, j])
        betas.append(b)
        assert b + b_ref < 0.1 * min_gap, (j, b, b_ref, min_gap)
        assert abs(lam[j] - ref.lam[j]) <= b + b_ref, (j, lam[j], ref.lam[j], b, b_ref)
        worst = max(worst, abs(lam[j] - ref.lam[j]) / (b + b_ref))
    for j in range(nev):
        mem = ref.members(j)
        others = np.setdiff1d(np.arange(ref.lam.size), mem)
        gap = min(float(np.min(np.abs(ref.lam[others] - lam[j]))),
                  float(np.min(np.abs(ref.lam[others][:, None] - ref.lam[mem][None, :]))))
        Vc = ref.V[:, mem]
        x = Xf[:, j] / np.sqrt(Xf[:, j] @ (ref.M @ Xf[:, j]))
        e = x - Vc @ (Vc.T @ (ref.M @ x))
        assert np.sqrt(e @ (ref.M @ e)) <= betas[j] / gap, (j, float(np.sqrt(e @ (ref.M @ e))), betas[j], gap)
        if mem[0] == j and mem[-1] < nev:       # a whole cluster among the returned pairs
            Xc = Xf[:, mem] / np.sqrt(np.sum(Xf[:, mem] * (ref.M @ Xf[:, mem]), axis=0))
            assert np.linalg.svd(Vc.T @ (ref.M @ Xc), compute_uv=False)[-1] >= 0.5
    if out is not None:
        out["worst"] = worst
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the driver against the model: a tolerance that every entry of the model's history stays away from
# ---------------------------------------------------------------------------------------------------------------------
# LOBPCG with a V-cycle lowers rho by a factor 3 to 10 per iteration, so a history of several columns leaves no tolerance a
# factor 10 from all of its entries.  The start block of these cases makes one: column 0 is the reference's first eigenvector
# (rho ~ 1e-13: locked from the start), the others are eigenvectors plus 1 % of a grid-frequency sign pattern, which the
# first V-cycle removes -- rho falls from 0.3 .. 0.5 to 2e-3 in one iteration (measured with the oracle's V-cycle).  The
# tolerance between the two rows ends the run after one iteration with one column locked and nb - 1 V-cycles.
FOLLOW = [("skew3", "q1", 4, 4), ("skew3", "q1", 2, 4)]


def follow_start(name, kind, nb, eps=0.01):
    p, ref = problem(name), reference(name, kind, True)
    nx, ny, nz = p.dims
    iz, iy, ix = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    signs = [((-1.0) ** e).ravel() for e in (ix + iy + iz, ix + iy, iy + iz, ix + iz)]
    X = np.zeros((p.A.shape[0], nb))
    X[ref.free] = ref.V[:, :nb]
    for j in range(1, nb):
        X[:, j] += eps * np.abs(X[:, j]).max() * signs[j % 4]
    return X


def follow_tol(run_model, lo=1e-4):
    """The tolerance of a follow case, as solve_cases.stopping_cases places its thresholds: the geometric middle of the
    widest gap, above `lo`, in the model's rho (run_model(tol, max_iter) -> all of them, every column of the block and every
    iteration), taken from a provisional run of three iterations that locks nothing but what is converged to rounding.
    Locking feeds back into the history, so the model is run again AT that tolerance and every rho of that run must lie
    a factor solve_cases.SEPARATION from it: the device then locks the same columns in the same iterations unless it
    deviates by that factor.  Returns (tol, the separation found)."""
    v = np.sort(np.asarray(run_model(1e-9, 3), dtype=np.float64).ravel())
    v = v[np.isfinite(v) & (v > lo)]
    k = int(np.argmax(v[1:] / v[:-1]))
    tol = float(np.sqrt(v[k] * v[k + 1]))
    sep = sc.separation(tol, [float(x) for x in np.asarray(run_model(tol, MAX_ITER)).ravel() if np.isfinite(x)])
    assert sep >= sc.SEPARATION, (tol, sep)
    return tol, sep
