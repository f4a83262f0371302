"""The definition of the eigensolver (numpy): the lowest pairs of A x = lambda M x by Knyazev's LOBPCG with soft locking,
preconditioned by any callable r -> z.  csrc/lobpcg.hip follows it step for step (csrc/lobpcg_host.h is its small dense
half); the device is held to the theorems in tests/lobpcg_cases.py and to this model's iteration counts, not to its bits.

One iteration, with the basis S = [X, W, P] (nb + nw + np <= 48 columns) and A S, M S carried along:

    G_A = S^T (A S), G_M = S^T (M S), symmetrised
    G_M = D L L^T D (D = sqrt(diag G_M)): Gram-Schmidt in the order X, W, P -- W against X, P against X and W -- done on
        the coefficients.  A pivot at or below PIVOT_FLOOR(m) is a breakdown: P is dropped and the step repeated (a
        restart); a breakdown right after a restart ends the call.
    Rayleigh-Ritz on L^-1 D^-1 G_A D^-1 L^-T: theta ascending, C = D^-1 L^-T Q
    X <- S C[:, :nb];  P <- S C[:, active] with the rows of X set to zero (the part that comes from W and P)
    R = A X - M X diag(theta), rho_j = ||r_j|| / (|theta_j| ||M x_j||); columns with rho_j <= tol are locked
    W_j = mask(prec(r_j)) for the active columns, then A W and M W: the only operator products of the iteration
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
MAX_BLOCK = 16
MAX_BASIS = 48


def pivot_floor(m):
    """a pivot of the Cholesky factor of a unit-diagonal Gram matrix of order m at or below this is a breakdown: the
    squared sine of the angle to the span of the columns before it is within the rounding of its own evaluation"""
    return 64.0 * m * EPS


def hash_start(seed, n, nb):
    """the start block when no x0 is given: entry (i, j) from a 32-bit counter hash of (seed, i, j), uniform in
    [-1, 1) on a grid of 2^-31 (every step is exact, so the device makes the same bits)"""
    u = np.uint32
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=u)[:, None]
        j = np.arange(nb, dtype=u)[None, :]
        h = (u(seed & 0xFFFFFFFF) * u(0x9E3779B9)) ^ (i * u(0x85EBCA6B)) ^ (j * u(0xC2B2AE35) + u(0x27D4EB2F))
        h ^= h >> u(16)
        h *= u(0x7FEB352D)
        h ^= h >> u(15)
        h *= u(0x846CA68B)
        h ^= h >> u(16)
    return h.astype(np.float64) * 2.0 ** -31 - 1.0


def cholesky_scaled(G):
    """G = D L L^T D with D = sqrt(diag G) and L lower triangular -> (d, L, bad): bad = -1, or the first column whose
    diagonal entry or pivot is not safely positive (d and L are then filled up to it)"""
    m = G.shape[0]
    d = np.zeros(m)
    L = np.zeros((m, m))
    for j in range(m):
        if not (np.isfinite(G[j, j]) and G[j, j] > 0.0):
            return d, L, j
        d[j] = np.sqrt(G[j, j])
    floor = pivot_floor(m)
    for j in range(m):
        v = G[j:, j] / (d[j:] * d[j]) - L[j:, :j] @ L[j, :j]
        if not (np.isfinite(v[0]) and v[0] > floor):
            return d, L, j
        L[j:, j] = v / np.sqrt(v[0])
    return d, L, -1


def solve_lower(L, B):
    """L^-1 B by forward substitution"""
    Y = np.array(B, dtype=np.float64)
    for i in range(L.shape[0]):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def solve_upper_t(L, B):
    """L^-T B by back substitution"""
    Y = np.array(B, dtype=np.float64)
    for i in range(L.shape[0] - 1, -1, -1):
        Y[i] = (Y[i] - L[i + 1:, i] @ Y[i + 1:]) / L[i, i]
    return Y


def rayleigh_ritz(GA, GM):
    """the symmetric generalised eigenproblem of the Gram pair -> (theta ascending, C with C^T GM C = I), or
    (None, bad) on a breakdown"""
    GA = 0.5 * (GA + GA.T)
    GM = 0.5 * (GM + GM.T)
    d, L, bad = cholesky_scaled(GM)
    if bad >= 0:
        return None, bad
    At = solve_lower(L, solve_lower(L, GA / np.outer(d, d)).T)
    theta, Q = np.linalg.eigh(0.5 * (At + At.T))
    return theta, solve_upper_t(L, Q) / d[:, None]


def residuals(AX, MX, lam):
    R = AX - MX * lam[None, :]
    den = np.abs(lam) * np.sqrt(np.sum(MX * MX, axis=0))
    nr = np.sqrt(np.sum(R * R, axis=0))
    ok = np.isfinite(den) & (den > 0.0)
    return R, np.where(ok, nr / np.where(ok, den, 1.0), np.inf)


def lobpcg(A, M, prec, ess, x0, nev, nb=0, tol=1e-8, max_iter=100, seed=0, trace=None):
    """-> lam (nev), X (n x nev, M-orthonormal), res (nev: the rho_j), iters, converged, hist ((iters + 1) x nev).
    ess: boolean mask of the rows held at zero, or None.  x0: n x nb or None (hash_start(seed)).  trace: a list that
    receives one dict per Rayleigh-Ritz: it, restart, breakdown, and where a next iteration follows rho (all nb columns)
    and active (the columns that get a W next)."""
    n = A.shape[0]
    nb = nb or nev
    assert 1 <= nev <= nb <= MAX_BLOCK and tol > 0.0 and max_iter >= 0
    ess = np.zeros(n, dtype=bool) if ess is None else np.asarray(ess, dtype=bool)
    assert 3 * nb <= n - int(ess.sum())
    mul_m = (lambda V: np.asarray(M @ V)) if M is not None else (lambda V: V.copy())
    X = np.array(hash_start(seed, n, nb) if x0 is None else x0, dtype=np.float64).reshape(n, nb)
    X[ess] = 0.0
    AX, MX = np.asarray(A @ X), mul_m(X)
    empty = np.zeros((n, 0))
    W = AW = MW = P = AP = MP = empty
    hist = np.zeros((max_iter + 1, nev))
    lam, rho = np.zeros(nb), np.full(nb, np.inf)
    active = np.zeros(nb, dtype=bool)
    it, converged = 0, 0
    while True:
        restart = False
        while True:
            S, AS, MS = np.hstack([X, W, P]), np.hstack([AX, AW, AP]), np.hstack([MX, MW, MP])
            GA, GM = S.T @ AS, S.T @ MS
            theta, C = rayleigh_ritz(GA, GM)
            if theta is not None or restart:
                break
            restart = True
            P = AP = MP = empty
        if trace is not None:
            trace.append(dict(it=it, restart=restart, breakdown=theta is None))
        if theta is None:           # a breakdown right after a restart: the best X so far
            if it == 0:
                g = np.diag(GM)[:nb]
                ok = np.isfinite(g) & (g > 0.0)
                lam = np.where(ok, np.diag(GA)[:nb] / np.where(ok, g, 1.0), 0.0)
                _, rho = residuals(AX, MX, lam)
                hist[0] = rho[:nev]
            else:
                it -= 1
            break
        Cx = C[:, :nb]
        Cp = Cx[:, active].copy()
        Cp[:nb] = 0.0
        X, AX, MX, P, AP, MP = S @ Cx, AS @ Cx, MS @ Cx, S @ Cp, AS @ Cp, MS @ Cp
        lam = theta[:nb]
        R, rho = residuals(AX, MX, lam)
        hist[it] = rho[:nev]
        if np.all(rho[:nev] <= tol):
            converged = 1
            break
        if it == max_iter:
            break
        active = ~(rho <= tol)
        if trace is not None:
            trace[-1].update(active=active.copy(), rho=rho.copy())
        W = np.zeros((n, int(active.sum())))
        for k, j in enumerate(np.nonzero(active)[0]):
            W[:, k] = prec(R[:, j])
        W[ess] = 0.0
        AW, MW = np.asarray(A @ W), mul_m(W)
        it += 1
    return lam[:nev].copy(), X[:, :nev].copy(), rho[:nev].copy(), it, converged, hist[:it + 1].copy()
