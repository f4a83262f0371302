"""The eigensolver on the device (Hierarchy.lobpcg, blockvec_gram, blockvec_combine) against the dense reference, the numpy
model and longdouble products; cases, references and bounds: tests/lobpcg_cases.py.  Hierarchies are built once per case
and closed when the module is done; every case is solved once and its result shared by the tests that look at it."""
import ctypes as C

import numpy as np
import pytest

import lobpcg_cases as lc
import solve_cases as sc

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
_HIER, _SOLVED = {}, {}
DEVICE_POINTER_CASE = ("skew3", "q1", 3, 5, True)


def _capi():
    from saamge_amd import capi
    return capi


def _hier(name):
    if name not in _HIER:
        capi = _capi()
        _HIER[name] = capi.Hierarchy.from_problem(lc.problem(name), lc.params(name))
        assert _HIER[name].num_levels == lc.coarsenings(name) + 1
    return _HIER[name]


@pytest.fixture(scope="module", autouse=True)
def _close_hierarchies():
    yield
    for h in _HIER.values():
        h.close()
    _HIER.clear()
    _SOLVED.clear()


def _solve(case, **kw):
    name, kind, nev, nb, constrained = case
    return _hier(name).lobpcg(nev, nb, M=lc.mass(name, kind), x0=lc.start_block(name, nb), tol=lc.TOL, max_iter=lc.MAX_ITER,
                              constrain_essential=constrained, **kw)


def _solved(case):
    if case not in _SOLVED:
        _SOLVED[case] = _solve(case)
    return _SOLVED[case]


# ---- 1. every row of the table ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.TABLE, ids=lc.case_id)
def test_pairs_lie_within_the_residual_bounds_of_the_dense_reference(case):
    lam, X, res, iters, converged, hist = _solved(case)
    assert converged == 1 and iters <= lc.MAX_ITER
    assert hist.shape == (iters + 1, case[2]) and np.array_equal(hist[-1], res) and np.all(res <= lc.TOL)
    worst = lc.check_pairs(lc.reference(case[0], case[1], case[4]), lam, X)
    print("%s: %d iterations, |theta - lambda| / (beta + beta_ref) <= %.2e" % (lc.case_id(case), iters, worst))


def test_device_pointers_for_mass_start_block_and_vectors():
    import torch
    name, kind, nev, nb, _ = DEVICE_POINTER_CASE
    M = lc.mass(name, kind)
    n = M.shape[0]
    dev = "cuda"
    m = (torch.tensor(M.indptr.astype(np.int64), device=dev), torch.tensor(M.indices.astype(np.int32), device=dev),
         torch.tensor(M.data, device=dev))
    x0 = torch.tensor(np.ascontiguousarray(lc.start_block(name, nb).T), device=dev)       # column-major n x nb
    evecs = torch.full((nev, n), np.nan, dtype=torch.float64, device=dev)
    lam, X, res, iters, converged, hist = _hier(name).lobpcg(nev, nb, M=m, x0=x0, tol=lc.TOL, max_iter=lc.MAX_ITER, evecs=evecs)
    torch.cuda.synchronize()
    ref = _solved(DEVICE_POINTER_CASE)
    assert X is evecs and converged == 1
    # the same inputs through host pointers: the same bits
    assert np.array_equal(lam, ref[0]) and np.array_equal(evecs.cpu().numpy().T, ref[1]) and np.array_equal(hist, ref[5])


def test_null_start_block_is_the_hash_of_the_model():
    """max_iter = 0 returns the start after the mask, the M-orthonormalisation and one Rayleigh-Ritz.
    One column, M = I: X = x / ||x|| for the masked hash column x, which the device makes bit for bit (every step of the
    hash is exact).  The device's x^T x and numpy's norm are sums of n terms, each within n eps / 2 of the true norm after
    the root; the root, the reciprocal, the product and numpy's quotient add one rounding each: (n + 8) eps in all.
    Five columns with the mass: the device's Ritz values are held to the Ritz values of the model's block V by the
    residual theorem in span(V): for any c and theta a Ritz value lies within ||G_A c - theta G_M c||_{G_M^-1} / ||c||_{G_M},
    with G = V^T (.) V; the same for the reference's own pairs."""
    import scipy.linalg as sla
    from saamge_amd import lobpcg_model as model
    name = "skew3"
    p, h = lc.problem(name), _hier(name)
    n = p.A.shape[0]
    ess = np.asarray(p.ess, dtype=bool)
    lam, X, res, iters, converged, hist = h.lobpcg(1, 1, x0=None, seed=7, max_iter=0)
    x = model.hash_start(7, n, 1)[:, 0]
    x[ess] = 0.0
    assert iters == 0 and converged == 0 and hist.shape == (1, 1) and np.array_equal(hist[0], res)
    want = np.abs(x) / np.linalg.norm(x)
    assert np.array_equal(X[:, 0] == 0.0, x == 0.0) and np.all(np.abs(np.abs(X[:, 0]) - want) <= (n + 8) * EPS * want)
    assert not np.array_equal(model.hash_start(7, n, 1), model.hash_start(8, n, 1))
    M = lc.mass(name, "q1")
    lam, X, res, iters, converged, hist = h.lobpcg(3, 5, M=M, x0=None, seed=12345, max_iter=0)
    V = model.hash_start(12345, n, 5)
    V[ess] = 0.0
    GA, GM = V.T @ (p.A @ V), V.T @ (M @ V)
    GA, GM = 0.5 * (GA + GA.T), 0.5 * (GM + GM.T)
    theta_ref, Q = sla.eigh(GA, GM)
    chol = sla.cho_factor(GM)

    def beta(theta, c):
        r = GA @ c - theta * (GM @ c)
        return float(np.sqrt(r @ sla.cho_solve(chol, r)) / np.sqrt(c @ (GM @ c)))
    assert iters == 0 and np.all(np.isfinite(X))
    for j in range(3):
        c = np.linalg.lstsq(V, X[:, j], rcond=None)[0]
        assert abs(lam[j] - theta_ref[j]) <= beta(lam[j], c) + beta(theta_ref[j], Q[:, j]), (j, lam[j], theta_ref[j])


def test_a_repeated_start_column_ends_the_call_without_nan():
    """the breakdown path of the driver: the Gram matrix of a start block with a repeated column has a zero pivot, the
    restart has no P to drop, the call ends with converged = 0, the masked start block as X and Rayleigh quotients as evals"""
    name = "cube8"
    p = lc.problem(name)
    x0 = lc.start_block(name, 4)
    x0[:, 2] = x0[:, 0]
    lam, X, res, iters, converged, hist = _hier(name).lobpcg(4, 4, x0=x0, tol=lc.TOL, max_iter=lc.MAX_ITER)
    assert converged == 0 and iters == 0 and hist.shape == (1, 4) and np.array_equal(hist[0], res)
    assert not np.any(np.isnan(lam)) and not np.any(np.isnan(X)) and not np.any(np.isnan(res))
    masked = np.where(np.asarray(p.ess, dtype=bool)[:, None], 0.0, x0)
    assert np.array_equal(X, masked) and np.all(lam > 0.0) and lam[2] == lam[0]


# ---- 2. res is honest --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.TABLE, ids=lc.case_id)
def test_returned_residuals_are_the_residuals_of_the_returned_pairs(case):
    """rho_j recomputed from the returned pair <= tol + 64 eps (||A x|| + lambda ||M x||) / (lambda ||M x||): 64 bounds the
    terms of one residual entry (27 entries of A, 27 of M and the subtraction)"""
    lam, X, res, iters, converged, hist = _solved(case)
    A, M = lc.problem(case[0]).A, lc.mass(case[0], case[1])
    for j in range(case[2]):
        ax, mx = A @ X[:, j], (X[:, j] if M is None else M @ X[:, j])
        den = lam[j] * np.linalg.norm(mx)
        rho = np.linalg.norm(ax - lam[j] * mx) / den
        assert rho <= lc.TOL + 64 * EPS * (np.linalg.norm(ax) + den) / den, (j, rho, res[j])


# ---- 3. the driver follows the model ----------------------------------------------------------------------------------
def _vcycles(h, run):
    """V-cycles `run` makes, from the kernel profile: the prolongation kernels it launches over those of one V-cycle"""
    capi = _capi()

    def prolongations(f):
        capi.profile(True)
        capi.profile_reset()
        try:
            out = f()
            return out, sum(k["launches"] for k in capi.profile_stats() if k["name"].startswith("spmv_add"))
        finally:
            capi.profile(False)
            capi.profile_reset()
    n = int(h.level_info(0)["n"])
    _, one = prolongations(lambda: h.vcycle(np.ones(n)))
    out, count = prolongations(run)
    assert one > 0 and count % one == 0
    return out, count // one


@pytest.mark.parametrize("case", lc.FOLLOW, ids=lambda c: "%s-%s-%d-%d" % (c[0], c[1] or "I", c[2], c[3]))
def test_driver_locks_the_columns_the_model_locks_and_takes_as_many_vcycles(case):
    from saamge_amd import lobpcg_model as model
    name, kind, nev, nb = case
    p, h, M, x0 = lc.problem(name), _hier(name), lc.mass(name, kind), lc.follow_start(name, kind, nb)
    runs = {}

    def run_model(tol, max_iter):
        trace = []
        out = model.lobpcg(p.A, M, lambda r: h.vcycle(np.ascontiguousarray(r)), p.ess, x0, nev, nb, tol, max_iter, trace=trace)
        runs[tol] = (out, trace)
        return np.concatenate([t["rho"] for t in trace if "rho" in t] + [out[5][-1]])
    tol, sep = lc.follow_tol(run_model)
    (lam_m, X_m, res_m, it_m, conv_m, hist_m), trace = runs[tol]
    assert conv_m == 1
    (lam, X, res, iters, converged, hist), cycles = _vcycles(
        h, lambda: h.lobpcg(nev, nb, M=M, x0=x0, tol=tol, max_iter=lc.MAX_ITER))
    assert (iters, converged) == (it_m, 1)
    assert np.array_equal(hist <= tol, hist_m <= tol), "another set of locked columns"
    assert cycles == sum(int(t["active"].sum()) for t in trace if "active" in t) and 0 < cycles < nb * iters
    dev = np.max(np.abs(hist - hist_m) / hist_m)
    print("%s tol %.0e (separation %.1f): %d iterations, %d V-cycles, histories deviate by at most %.2e (relative)"
          % (name, tol, sep, iters, cycles, dev))


# ---- 4. determinism ---------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits():
    case = ("tiles", "q1", 4, 4, True)
    a, b = _solved(case), _solve(case)
    for u, v in zip(a, b):
        assert np.array_equal(np.asarray(u), np.asarray(v))


# ---- 5. the block kernels on their own ----------------------------------------------------------------------------------
def _blocks(n, p, q, seed):
    """S (n x p), T (n x q): normal entries; column 0 scaled by 1e150 and column 1 by 1e-150, so that an accumulator shared
    across columns would drown the small one (products stay within the range of fp64: n 1e300 < 1.8e308)"""
    rng = np.random.default_rng(seed)
    S, T = rng.standard_normal((n, p)), rng.standard_normal((n, q))
    for B in (S, T):
        B[:, 0] *= 1e150
        if B.shape[1] > 1:
            B[:, 1] *= 1e-150
    return S, T


def _padded(B, ld):
    """the block column-major with leading dimension ld, NaN in the padding: (buffer, n, p, ld)"""
    buf = np.full((B.shape[1], ld), np.nan)
    buf[:, :B.shape[0]] = B.T
    return (buf, B.shape[0], B.shape[1], ld)


def _on_device(block):
    import torch
    return (torch.tensor(block[0], device="cuda"),) + tuple(block[1:])


# n, p, q, symmetric, leading-dimension padding, device pointers: every n and every width of the issue's lists occurs
GRAM = [(1, 1, 1, False, 0, False), (1, 3, 2, False, 5, False), (63, 2, 3, False, 0, False), (64, 5, 8, False, 0, True),
        (65, 15, 16, False, 7, False), (65, 16, 16, True, 3, False), (2730, 17, 32, False, 0, False),
        (2730, 48, 47, False, 0, True), (2730, 48, 48, True, 0, False), (2730, 47, 47, True, 6, True),
        (63, 48, 1, False, 0, False), (64, 32, 32, True, 0, False), (70001, 5, 8, False, 0, False),
        (70001, 17, 17, True, 0, True)]


@pytest.mark.parametrize("n,p,q,sym,pad,device", GRAM)
def test_gram_matches_longdouble_within_the_dot_product_bound(n, p, q, sym, pad, device):
    """|G_ij - ref| <= n eps sum_k |s_ki| |t_kj|; two calls give the same bits"""
    capi = _capi()
    S, T = _blocks(n, p, q, seed=n + 100 * p + q)
    T = S if sym else T
    bs = _padded(S, n + pad)
    bt = None if sym else _padded(T, n + pad)
    if device:
        bs, bt = _on_device(bs), (None if sym else _on_device(bt))
    G = capi.blockvec_gram(bs, bt)
    ld = np.longdouble
    ref = S.astype(ld).T @ T.astype(ld)
    bound = n * EPS * (np.abs(S).T @ np.abs(T))
    assert G.shape == (p, q) and np.all(np.abs(G.astype(ld) - ref) <= bound), float(np.max(np.abs(G.astype(ld) - ref) / bound))
    assert np.array_equal(G, capi.blockvec_gram(bs, bt))
    if sym:
        assert np.array_equal(G, G.T)


COMBINE = [(1, 1, 1, False, 0, False), (63, 2, 3, True, 0, False), (64, 5, 8, False, 4, True), (65, 15, 16, True, 0, True),
           (65, 17, 5, False, 0, False), (2730, 32, 47, False, 0, False), (2730, 48, 48, True, 2, False),
           (2730, 47, 32, False, 0, True), (64, 16, 1, False, 0, False), (70001, 3, 2, True, 0, False),
           (70001, 8, 15, False, 0, True), (1, 48, 17, False, 0, False)]


@pytest.mark.parametrize("n,p,q,accumulate,pad,device", COMBINE)
def test_combine_matches_longdouble_within_the_dot_product_bound(n, p, q, accumulate, pad, device):
    """|Y_ij - ref| <= p eps (|S| |C|)_ij; accumulating adds Y0 as one more term: (p + 1) eps (|Y0| + |S| |C|)_ij"""
    capi = _capi()
    rng = np.random.default_rng(n + 100 * p + q)
    S, Y0 = _blocks(n, p, q, seed=n + p + q)
    Cm = rng.standard_normal((p, q))
    Cm[0, :] *= 1e-150        # the large column of S meets small coefficients, the small one large ones
    if p > 1:
        Cm[1, :] *= 1e150
    Y0 = Y0 if accumulate else np.full((n, q), np.nan)
    Y0[:, :2] = rng.standard_normal((n, min(q, 2))) if accumulate else Y0[:, :2]
    bs, by = _padded(S, n + pad), _padded(Y0, n + pad)
    if device:
        bs, by = _on_device(bs), _on_device(by)
    out = capi.blockvec_combine(bs, Cm, by, accumulate=accumulate)
    Y = (out[0].cpu().numpy() if device else out[0])[:, :n].T
    ld = np.longdouble
    ref = S.astype(ld) @ Cm.astype(ld) + (Y0.astype(ld) if accumulate else 0)
    bound = (p + 1 if accumulate else p) * EPS * (np.abs(S) @ np.abs(Cm) + (np.abs(Y0) if accumulate else 0.0))
    assert np.all(np.abs(Y.astype(ld) - ref) <= bound), float(np.max(np.abs(Y.astype(ld) - ref) / bound))
    if pad:
        assert np.all(np.isnan((out[0].cpu().numpy() if device else out[0])[:, n:])), "the padding was written"


def test_combine_in_place_is_the_only_overlap_allowed():
    capi = _capi()
    n, p = 65, 6
    rng = np.random.default_rng(3)
    S, Cm = rng.standard_normal((n, p)), rng.standard_normal((p, p))
    buf = _padded(S, n)
    capi.blockvec_combine(buf, Cm, buf)
    ld = np.longdouble
    assert np.all(np.abs(buf[0].T.astype(ld) - S.astype(ld) @ Cm.astype(ld)) <= p * EPS * (np.abs(S) @ np.abs(Cm)))
    before = buf[0].copy()
    shifted = (buf[0][1:], n, p - 1, n)        # starts one column into S
    with pytest.raises(RuntimeError, match="overlaps"):
        capi.blockvec_combine(buf, Cm[:, :p - 1], shifted)
    assert np.array_equal(buf[0], before)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
SENTINEL = -777.25


def _raw_lobpcg(h, o, M=(None, None, None), x0=None, null=()):
    """the C entry with outputs pre-filled with a sentinel -> (return code, message, outputs untouched)"""
    capi = _capi()
    lib = capi.load()
    n = 2601
    ev, X, res, hist = (np.full(s, SENTINEL) for s in (16, 16 * n, 16, 101 * 16))
    it, conv = C.c_int(-7), C.c_int(-7)
    args = dict(h=h.h if h is not None else None, o=C.byref(o) if o is not None else None, evals=capi._ptr(ev), evecs=capi._ptr(X))
    for k in null:
        args[k] = None
    rc = lib.saamge_amd_lobpcg(args["h"], capi._ptr(M[0]), capi._ptr(M[1]), capi._ptr(M[2]), args["o"], capi._ptr(x0),
                               args["evals"], args["evecs"], capi._ptr(res), C.byref(it), C.byref(conv), capi._ptr(hist))
    untouched = all(np.all(a == SENTINEL) for a in (ev, X, res, hist)) and it.value == -7 and conv.value == -7
    return rc, lib.saamge_amd_last_error().decode(), untouched


def _options(**kw):
    capi = _capi()
    o = capi.LobpcgOptions()
    capi.load().saamge_amd_lobpcg_options_default(C.byref(o))
    assert (o.nev, o.block, o.tol, o.max_iter, o.constrain_essential, o.seed) == (1, 0, 1e-8, 100, 1, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("null", ["h", "o", "evals", "evecs"])
def test_null_arguments_are_refused_by_name(null):
    rc, msg, untouched = _raw_lobpcg(_hier("skew3"), _options(), null=(null,))
    assert rc != 0 and untouched and msg.endswith("null argument: " + null), msg


@pytest.mark.parametrize("field,value", [("nev", 0), ("nev", 17), ("nev", -1), ("block", 2), ("block", 17), ("block", -1),
                                         ("tol", 0.0), ("tol", -1e-8), ("tol", float("nan")), ("max_iter", -1)])
def test_options_out_of_range_are_refused_by_name(field, value):
    rc, msg, untouched = _raw_lobpcg(_hier("skew3"), _options(**dict(dict(nev=3), **{field: value})))
    assert rc != 0 and untouched and field in msg, msg


def test_a_block_wider_than_a_third_of_the_unconstrained_rows_is_refused():
    from saamge_amd import problems as pr
    capi = _capi()
    prob = pr.poisson3d_problem((4, 4, 4), blk=(2, 2, 2))       # 27 unconstrained rows
    assert int(np.sum(~np.asarray(prob.ess, dtype=bool))) == 27
    with capi.Hierarchy.from_problem(prob, capi.default_params(num_coarsenings=1, theta=sc.THETA)) as h:
        rc, msg, untouched = _raw_lobpcg(h, _options(nev=10))
        assert rc != 0 and untouched and "block" in msg and "unconstrained" in msg, msg
        rc, msg, untouched = _raw_lobpcg(h, _options(nev=10, constrain_essential=0))       # 125 rows: 30 <= 125
        assert rc == 0 and not untouched, msg


def test_a_malformed_mass_matrix_is_refused_by_name():
    M = lc.mass("skew3", "q1")
    rp, col, val = M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.copy()
    bad_start, decreasing, bad_col, neg_col = rp.copy(), rp.copy(), col.copy(), col.copy()
    bad_start[0] = 1
    decreasing[1000] = decreasing[999] - 1
    bad_col[123] = 2601
    neg_col[7] = -1
    for m, word in (((bad_start, col, val), "Mrowptr"), ((decreasing, col, val), "Mrowptr"), ((rp, bad_col, val), "Mcol"),
                    ((rp, neg_col, val), "Mcol"), ((rp, None, val), "Mcol")):
        rc, msg, untouched = _raw_lobpcg(_hier("skew3"), _options(nev=2), M=m)
        assert rc != 0 and untouched and word in msg, msg


@pytest.mark.parametrize("kw,word", [(dict(p=0), " p "), (dict(p=49), " p "), (dict(q=0), " q "), (dict(q=49), " q "),
                                     (dict(lds=63), "lds"), (dict(ldt=63), "ldt")])
def test_gram_refuses_bad_shapes_by_name(kw, word):
    capi = _capi()
    a = dict(n=64, p=4, lds=64, q=4, ldt=64)
    a.update(kw)
    S, G = np.ones(64 * 64), np.full(49 * 49, SENTINEL)
    rc = capi.load().saamge_amd_blockvec_gram(C.c_int(a["n"]), C.c_int(a["p"]), capi._ptr(S), C.c_longlong(a["lds"]),
                                              C.c_int(a["q"]), capi._ptr(S), C.c_longlong(a["ldt"]), capi._ptr(G))
    assert rc != 0 and np.all(G == SENTINEL) and word in capi.load().saamge_amd_last_error().decode()


@pytest.mark.parametrize("kw,word", [(dict(p=0), " p "), (dict(p=49), " p "), (dict(q=0), " q "), (dict(q=49), " q "),
                                     (dict(lds=63), "lds"), (dict(ldy=63), "ldy")])
def test_combine_refuses_bad_shapes_by_name(kw, word):
    capi = _capi()
    a = dict(n=64, p=4, lds=64, q=4, ldy=64)
    a.update(kw)
    S, Cm, Y = np.ones(64 * 64), np.ones(49 * 49), np.full(64 * 64, SENTINEL)
    rc = capi.load().saamge_amd_blockvec_combine(C.c_int(a["n"]), C.c_int(a["p"]), capi._ptr(S), C.c_longlong(a["lds"]),
                                                 C.c_int(a["q"]), capi._ptr(Cm), capi._ptr(Y), C.c_longlong(a["ldy"]), C.c_int(0))
    assert rc != 0 and np.all(Y == SENTINEL) and word in capi.load().saamge_amd_last_error().decode()


# ---- 7. the call leaves nothing behind ----------------------------------------------------------------------------------
def test_the_call_returns_its_memory_and_leaves_the_hierarchy_as_it_found_it():
    capi = _capi()
    case = ("tiles", "q1", 4, 4, True)
    h, p = _hier("tiles"), lc.problem("tiles")
    _solved(case)
    x_a, it_a, conv_a, hist_a = h.pcg(p.b, rel_tol=1e-8)
    live = capi.memory_stats()[0]
    _solve(case)
    assert capi.memory_stats()[0] == live
    x_b, it_b, conv_b, hist_b = h.pcg(p.b, rel_tol=1e-8)
    assert it_a == it_b and np.array_equal(hist_a, hist_b) and np.array_equal(x_a, x_b)


def test_eigenvalues_scale_with_the_operator_after_update_operators():
    capi = _capi()
    name, scale = "cube8", 2.5
    prob = lc.problem(name)
    with capi.Hierarchy.from_problem(prob, lc.params(name)) as h:
        h.update_operators(np.ascontiguousarray(prob.A.data * scale))
        lam, X, res, iters, converged, hist = h.lobpcg(4, 4, x0=lc.start_block(name, 4), tol=lc.TOL, max_iter=lc.MAX_ITER)
    assert converged == 1
    lc.check_pairs(lc.reference(name, None, True), lam / scale, X)
