"""include/saamge_amd_mfem.hpp RUN: tests/cxx/mfem_adaptor_run drives the adaptor's entry points -- the call sequences of
tests/cxx/mock_driver.cpp -- against the defining single-rank stand-in tests/mfem_mini/mfem.hpp and the real library, one child
process per problem, and writes what it got.  Here the same hierarchy is built through capi.Hierarchy from the parameter
fields the driver dumped (the saamge_amd_params it passed) and the same arrays, and EVERYTHING is compared for identical bits:
the same library, inputs, options and kernels ran on both sides.  What that pins is the marshalling: csr_of (the driver's
matrix has its rows diagonal-first and otherwise unsorted), the element-matrix gather through Matrix::Elem, the elem_to_elem
chain that feeds the coarse partitioner, the uniform / mixed dispatch, fetch_operators, the 11-argument parameter mapping, the
tolerance mapping of kalchev_pcg, the plug trampolines and their lifetime."""
import functools
import shutil
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import adaptor_cases as ac
from saamge_amd import problems as pr

pytestmark = pytest.mark.gpu

_TMP = []
_OPEN = []
_CACHES = []


def _once(fn):
    """functools.lru_cache that also remembers a FAILURE: a child process that faulted, hung into its time limit or returned a
    non-zero status is started once per module -- every later test that needs its output fails with the same exception and
    launches nothing."""
    results = {}

    @functools.wraps(fn)
    def wrapper(*args):
        if args not in results:
            try:
                results[args] = (True, fn(*args))
            except Exception as e:      # (TimeoutExpired and AssertionError alike)
                results[args] = (False, e)
        ok, value = results[args]
        if not ok:
            raise value
        return value
    wrapper.cache_clear = results.clear
    _CACHES.append(wrapper)
    return wrapper


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    for h in _OPEN:
        h.close()
    del _OPEN[:]
    for d in _TMP:
        shutil.rmtree(d, ignore_errors=True)
    del _TMP[:]
    for f in _CACHES:
        f.cache_clear()


def _capi():
    from saamge_amd import capi
    return capi


def _same(a, b):
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), "first difference at %d of %d" % (int(np.flatnonzero(a.view(np.uint8) != b.view(np.uint8))[0]) // a.itemsize, a.size)


def _same_csr(out, pre, M):
    _same(out[pre + ".shape"], np.asarray(M.shape, dtype=np.int32))
    _same(out[pre + ".I"], M.indptr.astype(np.int32))
    _same(out[pre + ".J"], M.indices.astype(np.int32))
    _same(out[pre + ".V"], M.data)


def _same_ops(out, pre, h, level):
    _same_csr(out, pre + "interp", h.get_csr(level, "P"))
    _same_csr(out, pre + "restr", h.get_csr(level, "R"))
    _same_csr(out, pre + "Ac", h.get_csr(level, "Ac"))


def _run(arrays, scenarios):
    d = tempfile.mkdtemp(prefix="saamge_adaptor_")
    _TMP.append(d)
    ac.write_container(d + "/in.bin", arrays)
    return ac.run_driver(d + "/in.bin", scenarios, d + "/out.bin", timeout=120)


def _params(out, pre):
    """saamge_amd_params from the scalar fields the driver dumped: what it really passed, not a second guess."""
    capi = _capi()
    p = capi.default_params()
    assert len(out[pre + "theta"]) == capi.MAX_LEVELS and len(out[pre + "options"]) == len(capi.Options._fields_)
    p.num_coarsenings = int(out[pre + "num_coarsenings"][0])
    for i in range(capi.MAX_LEVELS):
        p.theta[i], p.nu_relax[i], p.nu_pro[i] = float(out[pre + "theta"][i]), int(out[pre + "nu_relax"][i]), int(out[pre + "nu_pro"][i])
    for k in ("avoid_ess_bdr_dofs", "testmesh", "coarse_solver", "coarse_max_iter", "workspace_bytes", "keep_debug",
              "dist_min_local_rows", "correct_nullspace", "algebraic", "do_aggregates", "eigensolver"):
        setattr(p, k, int(out[pre + k][0]))
    for k in ("coarse_rtol", "smooth_drop_tol", "eig_tol"):
        setattr(p, k, float(out[pre + k][0]))
    assert int(out[pre + "num_extra_modes"][0]) == 0
    for i, (name, _) in enumerate(capi.Options._fields_):
        setattr(p.options, name, int(out[pre + "options"][i]))
    return p


def _sorted_csr(arrays, values="A_val"):
    n = len(arrays["A_rowptr"]) - 1
    A = sp.csr_matrix((arrays[values].copy(), arrays["A_col"].copy(), arrays["A_rowptr"].copy()), shape=(n, n))
    A.sort_indices()
    return A


def _build(arrays, params, parts, nparts):
    """The comparison hierarchy: the C ABI on the same arrays (A sorted, which is the adaptor's job on the other side)."""
    capi = _capi()
    A = _sorted_csr(arrays)
    n = A.shape[0]
    eptr = arrays.get("elem_ptr")
    NE = len(eptr) - 1 if eptr is not None else len(arrays["elem_to_dof"]) // int(arrays["nde"][0])
    h = capi.Hierarchy(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64), n,
                       arrays["elem_to_dof"], arrays["elmat"], arrays["bdr"], [np.ascontiguousarray(p, dtype=np.int32) for p in parts],
                       [int(x) for x in nparts], params, NE, 0 if eptr is not None else int(arrays["nde"][0]), elem_ptr=eptr)
    _OPEN.append(h)
    return h


def _pcg(h, arrays, rtol, atol, max_iter=1000, start=None):
    """kalchev_pcg's return value and x from the C ABI: iterations, negative when not converged, -1 when the start vector
    already satisfies the criterion."""
    x, it, conv, _ = h.pcg(arrays["b"], (arrays["x0"] if start is None else start).copy(), rel_tol=rtol, abs_tol=atol,
                           max_iter=max_iter, squared_tol=False, zero_guess=False)
    return (-1 if conv and it == 0 else (it if conv else -it)), x


def _arrays(a):
    return {k: np.atleast_1d(np.asarray(v)) for k, v in a.items()}


# ---- the problems, one child process each -----------------------------------------------------------------------------------
@_once
def _mltest():
    prob = pr.mltest_problem(order=1, levels=3)
    a = ac.problem_arrays(prob, 2, dim=2, testmesh=1, correct_nullspace=0, theta=0.003, nu_relax=3)
    given = (a["A_rowptr"], a["A_col"], a["A_val"])
    for k in range(3):
        a["A_val_new%d" % k] = ac.scaled_values(given, k)
    a = _arrays(a)
    return prob, a, _run(a, ["ml", "counting", "plugs", "split", "update"])


@_once
def _poisson(levels):
    prob = pr.poisson3d_problem((8, 8, 8), blk=(4, 4, 2))
    a = ac.problem_arrays(prob, 1, nparts=[16, 2][:levels - 1], dim=3, theta=0.003, nu_relax=3, elems_per_agg=32, correct_nullspace=1)
    a["coarsenings"] = np.int32(levels - 1)
    a = _arrays(a)
    return prob, a, _run(a, ["default_hook", "encapsulate"] if levels == 3 else ["default_hook"])


@_once
def _mixed():
    prob = pr.poisson3d_mixed_problem((8, 8, 4), (4, 4, 2), wedges="half", coef="skew", seed=7)
    a = _arrays(ac.problem_arrays(prob, 1, dim=3, theta=0.003, nu_relax=3))
    return prob, a, _run(a, ["mixed"])


@_once
def _algebraic(case):
    if case == "laplace2d_window":
        T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(24, 24))
        A = (sp.kron(sp.identity(24), T) + sp.kron(T, sp.identity(24))).tocsr()
        part, theta = (np.arange(A.shape[0]) // 48).astype(np.int32), 0.02
    else:
        A = pr.poisson3d_problem((8, 8, 8), blk=(4, 4, 2)).A.tocsr()
        part, theta = (np.arange(A.shape[0]) // 60).astype(np.int32), 0.01
    a = _arrays(ac.algebraic_arrays(A, part, theta))
    return a, _run(a, ["algebraic"])


def _ml_case(name):
    """-> arrays, the driver's output, its prefix, the partitions of every coarsening as the driver must have used them."""
    if name == "ml":
        prob, a, out = _mltest()
        return a, out, "ml.", [a["part0"], a["part1"]]
    if name == "mixed":
        prob, a, out = _mixed()
        return a, out, "mixed.", [a["part0"]]
    levels = int(name[-1])
    prob, a, out = _poisson(levels)
    nparts = out["default_hook.nparts"]
    parts = [a["part0"]]
    for k in range(1, levels - 1):          # the default coarse partitioner: contiguous index ranges
        n_el = int(nparts[k - 1])
        parts.append((np.arange(n_el, dtype=np.int64) * int(nparts[k]) // n_el).astype(np.int32))
    return a, out, "default_hook.", parts


@_once
def _hierarchy(name):
    a, out, pre, parts = _ml_case(name)
    return _build(a, _params(out, pre + "params."), parts, out[pre + "nparts"])


ML_CASES = ["ml", "default_hook2", "default_hook3", "mixed"]


# ---- ml / default_hook / mixed: the multilevel sequence -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ML_CASES)
def test_ml_dims_and_operators(name):
    """ml_get_dims vs level_info; every level's interp / restr / Ac (fetch_operators through GetDiag) vs get_csr.  A wrong row
    order out of csr_of, a wrong element-matrix gather or the wrong entry point (uniform / mixed) changes these bits."""
    a, out, pre, parts = _ml_case(name)
    h = _hierarchy(name)
    nco = len(parts)
    assert int(out[pre + "num_levels"][0]) == nco and h.num_levels >= nco + 1
    info = [h.level_info(l) for l in range(nco)]
    _same(out[pre + "dims"], np.asarray([i["n"] for i in info] + [info[-1]["ncoarse"]], dtype=np.int32))
    for l in range(nco):
        _same_ops(out, "%sL%d." % (pre, l), h, l)
        assert int(out["%sL%d.level" % (pre, l)][0]) == l
        _same(out["%sL%d.theta" % (pre, l)], np.float64(out[pre + "params.theta"][l]))
    if name == "mixed":
        assert set(np.diff(a["elem_ptr"])) == {6, 8}          # (sizes differ: the _mixed entry point was the one to take)


@pytest.mark.parametrize("name", ML_CASES)
def test_ml_tables(name):
    """agg_fetch_tables: the five tables, mises, num_mises and agg_flags vs get_table / get_mis."""
    a, out, pre, parts = _ml_case(name)
    h = _hierarchy(name)
    for t in ("AE_to_dof", "dof_to_AE", "mis_to_dof", "mis_to_AE", "AE_to_mis"):
        I, J = h.get_table(0, t)
        _same(out[pre + t + ".I"], I)
        _same(out[pre + t + ".J"], J)
    mises, k, ncols, flags = h.get_mis(0)
    _same(out[pre + "mises"], mises)
    _same(out[pre + "agg_flags"], flags)
    assert int(out[pre + "num_mises"][0]) == h.level_info(0)["num_mises"] == len(k)


@pytest.mark.parametrize("name", ML_CASES)
def test_ml_cycles(name):
    """VCycleSolver(tg, false).Mult(b) vs vcycle; VCycleSolver(tg, true).Mult(b, x0) vs vcycle_iterative."""
    a, out, pre, parts = _ml_case(name)
    h = _hierarchy(name)
    _same(out[pre + "cycle"], h.vcycle(a["b"]))
    _same(out[pre + "cycle_it"], h.vcycle_iterative(a["b"], a["x0"].copy()))


@pytest.mark.parametrize("name", ML_CASES)
def test_ml_kalchev_pcg(name):
    """kalchev_pcg at RTOLERANCE / ATOLERANCE = 1e-6 / 0 and at 10e-12 / 10e-24 (the defaults of saamge_amd::api::kalchev_pcg)
    vs pcg(squared_tol=False, zero_guess=False): the return value with its sign / -1 convention, and x."""
    a, out, pre, parts = _ml_case(name)
    h = _hierarchy(name)
    for key, rtol, atol in (("pcg6", 1e-6, 0.0), ("pcgd", 10e-12, 10e-24)):
        ret, x = _pcg(h, a, rtol, atol)
        print("%s %s: kalchev_pcg returned %d, the C ABI gives %d" % (name, key, int(out[pre + key + ".ret"][0]), ret))
        assert int(out[pre + key + ".ret"][0]) == ret
        _same(out[pre + key + ".x"], x)
    assert int(out[pre + "pcgd.ret"][0]) >= int(out[pre + "pcg6.ret"][0]) > 0          # (both converged, the tighter one later)


@pytest.mark.parametrize("name", ML_CASES)
def test_ml_kalchev_pcg_return_conventions(name):
    """The other two conventions of the return value: the NEGATIVE iteration count when the loop ends unconverged (2
    iterations, a tolerance out of reach), and -1 when the start vector -- the solution just computed -- already satisfies
    the criterion (x then stays as it is)."""
    a, out, pre, parts = _ml_case(name)
    h = _hierarchy(name)
    ret, x = _pcg(h, a, 1e-30, 0.0, max_iter=2)
    assert int(out[pre + "pcgshort.ret"][0]) == ret == -2
    _same(out[pre + "pcgshort.x"], x)
    ret, x = _pcg(h, a, 1e-6, 1e300, start=out[pre + "pcgd.x"])
    assert int(out[pre + "pcgdone.ret"][0]) == ret == -1
    _same(out[pre + "pcgdone.x"], x)
    _same(out[pre + "pcgdone.x"], out[pre + "pcgd.x"])


@pytest.mark.parametrize("name", ML_CASES)
def test_builtin_smoother_called_directly(name):
    """tg->pre_smoother(A, b, x, tg->poly_data) with the default smpr_sym_poly, as a driver may call it, vs smoother(0, b, x)."""
    a, out, pre, parts = _ml_case(name)
    _same(out[pre + "smoother"], _hierarchy(name).smoother(0, a["b"], a["x0"].copy()))


def test_ml_reports_the_reference_iteration_count():
    """The anchor to the reference: its `threelevel` ctest solves the mltest fixture in 3 iterations at rel_tol = 1e-6.  That
    driver runs MFEM's CGSolver from x = 0, whose rule is (B r, r) < rel_tol^2 (B r0, r0): in kalchev_pcg's un-squared terms
    RTOLERANCE = 1e-12, ATOLERANCE = 0, start vector 0.  The C ABI's side of the comparison is the very call smoke() makes.
    (At RTOLERANCE = 1e-6 from x0, which test_ml_kalchev_pcg compares, both sides take 2.)"""
    prob, a, out = _mltest()
    x, it, conv, _ = _hierarchy("ml").pcg(a["b"], rel_tol=1e-6)
    print("ml pcgref.ret = %d, the C ABI gives %d" % (int(out["ml.pcgref.ret"][0]), it))
    assert conv and int(out["ml.pcgref.ret"][0]) == it == 3
    _same(out["ml.pcgref.x"], x)


@pytest.mark.parametrize("name", ["ml", "default_hook3"])
def test_coarse_partitioner_hook_gets_the_ae_graph(name):
    """The Table handed to the hook at level 1 is AE_to_elem x elem_to_elem x elem_to_AE as a set of columns per row, with
    every column once; the hook is asked for the level-1 number of parts on the level-0 number of agglomerates."""
    a, out, pre, parts = _ml_case(name)
    nparts = out[pre + "nparts"]
    assert out[pre + "hook.level"].tolist() == [1]
    assert out[pre + "hook.n_elem"].tolist() == [int(nparts[0])] and out[pre + "hook.nparts"].tolist() == [int(nparts[1])]
    NE = len(a["part0"])
    e2AE = sp.csr_matrix((np.ones(NE, dtype=np.int64), (np.arange(NE), a["part0"])), shape=(NE, int(nparts[0])))
    E2E = sp.csr_matrix((np.ones(len(a["e2e_J"]), dtype=np.int64), a["e2e_J"], a["e2e_I"]), shape=(NE, NE))
    want = sp.csr_matrix(e2AE.T @ E2E @ e2AE)
    want.eliminate_zeros()
    want.sort_indices()
    I, J = out[pre + "hook1.I"], out[pre + "hook1.J"]
    assert len(I) == int(nparts[0]) + 1 and len(J) == want.nnz
    assert [sorted(J[I[r]:I[r + 1]].tolist()) for r in range(len(I) - 1)] == [want.indices[want.indptr[r]:want.indptr[r + 1]].tolist()
                                                                           for r in range(want.shape[0])]
    if name == "ml":
        assert want.nnz > want.shape[0]          # (the graph has edges: the fixture's agglomerates touch)


def test_default_coarse_partition_is_contiguous_ranges():
    """default_hook at 3 levels: the hierarchy the default partitioner leads to is the one of e * nparts // n_el (compared
    bit for bit above); here: that partition really has the 2 parts asked for, so the comparison is not vacuous."""
    a, out, pre, parts = _ml_case("default_hook3")
    assert parts[1].tolist() == [0] * 8 + [1] * 8 and out[pre + "nparts"].tolist() == [16, 2]
    assert _hierarchy("default_hook3").level_info(1)["nparts"] == 2


def test_element_matrix_counters():
    """ComputeElementMatrix is called exactly NE times; a provider's matrices are deleted by the adaptor exactly when it says
    free_matr (NE times / never), and its matrices -- no DenseMatrix, read through Matrix::Elem -- give the same Ac."""
    prob, a, out = _mltest()
    NE = len(a["part0"])
    assert int(out["ml.compute_calls"][0]) == NE
    assert int(out["counting.provider_copies.calls"][0]) == NE and int(out["counting.provider_own.calls"][0]) == NE
    assert int(out["counting.provider_copies.deleted"][0]) == NE
    assert int(out["counting.provider_own.deleted"][0]) == 0
    h = _two_level_mltest()
    for q in ("provider_copies", "provider_own"):
        _same_csr(out, "counting.%s.Ac" % q, h.get_csr(0, "Ac"))


# ---- plugs --------------------------------------------------------------------------------------------------------------------
def _jacobi(d, log=None):
    def fn(level, b, x):
        if log is not None:
            log.append((level, len(b)))
        return x + 0.6 * (b - d * x) / d
    return fn


def _plug(h, levels, log=None):
    """The driver's plugs on the C ABI: x_i = r_i / Ac_ii on the coarsest operator, x_i += 0.6 (b_i - a_ii x_i) / a_ii on each
    level's operator; element-wise single IEEE operations on both sides."""
    dc = h.get_csr(levels - 1, "Ac").diagonal()
    h.set_coarse_solver(lambda r: r / dc)
    for l in range(levels):
        d = h.get_csr(l, "A").diagonal()
        h.set_smoother(l, _jacobi(d, log), _jacobi(d, log))


def _unplug(h, levels):
    h.set_coarse_solver(None)
    for l in range(levels):
        h.set_smoother(l, None, None)


def test_plugs_cycle_and_pcg():
    """A caller's coarse_solver and pre / post smoothers through the trampolines: cycle and kalchev_pcg vs the same arithmetic
    installed through set_coarse_solver / set_smoother; each smoother call was handed the level's own operator (Ag on
    level 0, level k-1's Ac on level k) with its height."""
    prob, a, out = _mltest()
    h = _hierarchy("ml")
    _same(out["plugs.builtin_cycle"], out["ml.cycle"])
    log = []
    _plug(h, 2, log)
    try:
        _same(out["plugs.cycle"], h.vcycle(a["b"]))
        dims = out["ml.dims"]
        assert out["plugs.smoother_op"].tolist() == [0, 1, 1, 0] == [l for l, _ in log]
        assert out["plugs.smoother_height"].tolist() == [int(dims[0]), int(dims[1]), int(dims[1]), int(dims[0])] == [m for _, m in log]
        assert int(out["plugs.coarse_calls"][0]) == 1
        ret, x = _pcg(h, a, 1e-6, 0.0)
        assert int(out["plugs.pcg6.ret"][0]) == ret
        _same(out["plugs.pcg6.x"], x)
        # kalchev_pcg as the FIRST call after the plugs were assigned (no Mult before it) sees them too
        assert int(out["plugs.pcg_first.ret"][0]) == ret
        _same(out["plugs.pcg_first.x"], x)
    finally:
        _unplug(h, 2)
    assert int(out["plugs.pcg6.ret"][0]) != int(out["ml.pcg6.ret"][0])          # (the plugs change the count: not vacuous)
    assert out["plugs.cycle"].tobytes() != out["ml.cycle"].tobytes()


def test_plugs_restored_builtins():
    """smpr_sym_poly and coarse_solver = NULL assigned back: the same solver object cycles with the built-ins again."""
    prob, a, out = _mltest()
    _same(out["plugs.restored_cycle"], out["ml.cycle"])
    assert int(out["plugs.restored_plug_calls"][0]) == 0
    # kalchev_pcg was the first call after the built-ins were assigned back: it unplugs by itself
    assert int(out["plugs.restored_pcg.ret"][0]) == int(out["ml.pcg6.ret"][0])
    _same(out["plugs.restored_pcg.x"], out["ml.pcg6.x"])


def test_plug_lifetime_across_solvers():
    """Solver A installs the plugs and is deleted, the caller restores the built-ins in tg_data, solver B cycles: the
    built-in cycle, and no plug is called (the state of what is installed lives in tg_data, not in a solver)."""
    prob, a, out = _mltest()
    _same(out["plugs.life_plugged_cycle"], out["plugs.cycle"])
    _same(out["plugs.life_cycle"], out["ml.cycle"])
    assert int(out["plugs.life_plug_calls"][0]) == 0
    # solver B's first call was kalchev_pcg
    assert int(out["plugs.life_pcg.ret"][0]) == int(out["ml.pcg6.ret"][0])
    _same(out["plugs.life_pcg.x"], out["ml.pcg6.x"])


# ---- split --------------------------------------------------------------------------------------------------------------------
@_once
def _two_level_mltest_cached():
    prob, a, out = _mltest()
    return _build(a, _params(out, "split.params."), [a["part0"]], out["split.nparts"])


def _two_level_mltest():
    return _two_level_mltest_cached()


def test_split_equals_produce_data():
    """tg_init_data + tg_build_hierarchy = tg_produce_data = the C ABI with one coarsening."""
    prob, a, out = _mltest()
    h = _two_level_mltest()
    for pre in ("split.", "split.produce."):
        _same_ops(out, pre, h, 0)
        _same(out[pre + "cycle"], h.vcycle(a["b"]))
        _same(out[pre + "cycle_it"], h.vcycle_iterative(a["b"], a["x0"].copy()))
        ret, x = _pcg(h, a, 1e-6, 0.0)
        assert int(out[pre + "pcg6.ret"][0]) == ret
        _same(out[pre + "pcg6.x"], x)


def test_split_keeps_tag_and_plugs():
    prob, a, out = _mltest()
    assert int(out["split.tag"][0]) == 7 and int(out["split.plugs_kept"][0]) == 1
    h = _two_level_mltest()
    _plug(h, 1)
    try:
        _same(out["split.plugged_cycle"], h.vcycle(a["b"]))
    finally:
        _unplug(h, 1)
    assert out["split.smoother_op"].tolist() == [0, 0]


@pytest.mark.parametrize("which", ["Ac_rowpart", "Ac_colpart", "interp_rowpart", "interp_colpart", "restr_rowpart", "restr_colpart"])
def test_split_operators_point_into_the_callers_struct(which):
    """After tg_build_hierarchy, RowPart() / ColPart() of Ac / interp / restr are tg_data.row_starts[...] of the CALLER's struct
    (a HypreParMatrix keeps the pointers it is given), and they hold the level's sizes."""
    prob, a, out = _mltest()
    assert int(out["split." + which][0]) == 1
    h = _two_level_mltest()
    info = h.level_info(0)
    assert out["split.starts"].tolist() == [0, info["ncoarse"], 0, info["n"]]


# ---- update -------------------------------------------------------------------------------------------------------------------
def test_update_coarse_operator():
    """tg_update_coarse_operator with new values (given diagonal-first and unsorted, like the matrix) under
    (perform_solve_init, coarse_direct) = (true, true), (true, false), (false, -) vs update_operators2(.., 1 / 2 / -1)."""
    prob, a, out = _mltest()
    capi = _capi()
    h = _build(a, _params(out, "update.params."), [a["part0"], a["part1"]], out["update.nparts"])
    previous = out["ml.cycle"]
    for k, cs in enumerate((1, 2, -1)):
        h.update_operators(_sorted_csr(a, "A_val_new%d" % k).data, coarse_solver=cs)
        x = h.vcycle(a["b"])
        _same(out["update.u%d.cycle" % k], x)
        assert x.tobytes() != previous.tobytes()
        previous = x
        assert int(out["update.u%d.coarse_kind" % k][0]) == h.coarse_solver_info()["kind"]
    # perform_solve_init = false leaves the solver that is in place (the reference: "the old solver object"): the inner PCG of step 1
    assert [int(out["update.u%d.coarse_kind" % k][0]) for k in range(3)] == [1, 2, 2]


# ---- encapsulate --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [2, 3])
def test_encapsulate_both_constructors(levels):
    """SpectralAMGSolver from the form (GetEssentialVDofs, the mesh's tables, the fine-partitioner hook) and from the topology
    as arguments: Mult(b) of both vs the C ABI with the parameters build() maps its arguments to."""
    prob, a, out = _poisson(3)
    pre = "encapsulate.levels%d." % levels
    nparts = out[pre + "nparts"]
    assert nparts.tolist() == [16, 1][:levels - 1]
    parts = [a["part0"]] + [np.zeros(16, dtype=np.int32)] * (levels - 2)
    h = _build(a, _params(out, pre + "params."), parts, nparts)
    x = h.vcycle(a["b"])
    _same(out[pre + "form.cycle"], x)
    _same(out[pre + "arrays.cycle"], x)
    assert int(out[pre + "form.compute_calls"][0]) == len(a["part0"]) and int(out[pre + "form.height"][0]) == len(a["b"])
    assert int(out[pre + "params.correct_nullspace"][0]) == 1 and int(out[pre + "params.coarse_solver"][0]) == (1 if levels == 3 else 0)


# ---- algebraic ----------------------------------------------------------------------------------------------------------------
@_once
def _algebraic_hierarchy(case, mode):
    capi = _capi()
    a, out = _algebraic(case)
    h = capi.Hierarchy.from_matrix(_sorted_csr(a), a["part0"], _params(out, "algebraic.%s.params." % mode))
    _OPEN.append(h)
    return h


@pytest.mark.parametrize("mode", ["plain", "window"])
@pytest.mark.parametrize("case", ["laplace2d_window", "poisson"])
def test_algebraic_driver(case, mode):
    """mock_algebraic_driver with window_amg false / true: the caller's coarse_solver assigned, a fresh VCycleSolver, kalchev_pcg at
    1e-12 / 1e-24 as its first call -- vs set_coarse_solver + pcg; then the built-in solver again; operators vs from_matrix; the
    host copy of Ac freed by tg_free_coarse_operator comes back from tg_fillin_coarse_operator with the same bits."""
    a, out = _algebraic(case)
    pre = "algebraic.%s." % mode
    assert int(out[pre + "params.algebraic"][0]) == (2 if mode == "window" else 1)
    h = _algebraic_hierarchy(case, mode)
    _same_ops(out, pre, h, 0)
    assert int(out[pre + "Ac_freed"][0]) == 1
    _same_ops(out, pre + "refetched.", h, 0)
    dc = h.get_csr(0, "Ac").diagonal()
    h.set_coarse_solver(lambda r: r / dc)
    try:
        ret, x = _pcg(h, a, 1e-12, 1e-24)
        assert int(out[pre + "plugged_pcg.ret"][0]) == ret
        _same(out[pre + "plugged_pcg.x"], x)
        _same(out[pre + "plugged_cycle"], h.vcycle(a["b"]))
    finally:
        h.set_coarse_solver(None)
    # the caller's solver was really called, and changes the result -- wherever there is a coarse space at all (the window
    # matrices of the Poisson case have no eigenvalue below theta: no coarse dof, no coarse solve on either side)
    nc = int(out[pre + "Ac.shape"][0])
    print("%s %s: %d coarse dofs, %d calls of the caller's coarse solver" % (case, mode, nc, int(out[pre + "coarse_calls"][0])))
    assert nc == h.level_info(0)["ncoarse"] and (int(out[pre + "coarse_calls"][0]) > 0) == (nc > 0)
    _same(out[pre + "cycle"], h.vcycle(a["b"]))
    assert (out[pre + "cycle"].tobytes() != out[pre + "plugged_cycle"].tobytes()) == (nc > 0)
    assert nc > 0 or (case, mode) == ("poisson", "window")
    ret, x = _pcg(h, a, 1e-6, 0.0)
    assert int(out[pre + "pcg6.ret"][0]) == ret
    _same(out[pre + "pcg6.x"], x)


def test_algebraic_modes_differ():
    a, out = _algebraic("laplace2d_window")
    assert out["algebraic.plain.Ac.V"].tobytes() != out["algebraic.window.Ac.V"].tobytes()
