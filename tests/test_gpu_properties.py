"""GPU tests that do not need the oracle at full size: committed golden fixtures, and
size-independent properties on larger problems / edge cases."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from saamge_amd import problems as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _capi():
    from saamge_amd import capi
    return capi


@pytest.mark.parametrize("name,prob_fn,nco,testmesh,theta", [
    ("mltest_q1_2level", lambda: pr.mltest_problem(order=1, levels=2), 1, True, 0.003),
    ("mltest_q1_3level", lambda: pr.mltest_problem(order=1, levels=3), 2, True, 0.003),
    ("mltest_q2_2level", lambda: pr.mltest_problem(order=2, levels=2), 1, True, 0.003),
    ("poisson3d_8_2level", lambda: pr.poisson3d_problem((8, 8, 8), blk=(4, 4, 2)), 1, False, 0.003),
    ("poisson3d_aniso_2level", lambda: pr.poisson3d_problem((12, 8, 4), blk=(4, 4, 2), K=(1, 1, 1000.0)), 1, False, 0.02),
])
def test_against_golden_fixture(name, prob_fn, nco, testmesh, theta):
    capi = _capi()
    g = np.load(os.path.join(GOLD, name + ".npz"))
    prob = prob_fn()
    params = capi.default_params(num_coarsenings=nco, theta=theta, testmesh=testmesh, keep_debug=True,
                                 coarse_rtol=1e-28)
    h = capi.Hierarchy.from_problem(prob, params)
    for l in range(nco):
        mises, k, ncols, flags = h.get_mis(l)
        assert np.array_equal(mises, g["l%d_mises" % l])                      # bit exact
        I, J = h.get_table(l, "mis_to_dof")
        assert np.array_equal(I, g["l%d_mis_to_dof_I" % l]) and np.array_equal(J, g["l%d_mis_to_dof_J" % l])
        assert np.array_equal(h.get_table(l, "mis_to_AE")[1], g["l%d_mis_to_AE_J" % l])
        assert np.array_equal(np.diff(h.get_table(l, "AE_to_dof")[0]), g["l%d_AE_sizes" % l])
        m, ev, X, Ds = h.get_ae_eigens(l)
        assert np.array_equal(m, g["l%d_ae_m" % l])
        assert np.array_equal(k, g["l%d_mis_k" % l])
        if l == 0 or name.startswith("mltest"):
            evg = g["l%d_evals" % l]
            assert np.allclose(np.concatenate(ev), evg[:sum(len(e) for e in ev)] if len(evg) != sum(len(e) for e in ev) else evg, atol=1e-11)
        Ac = h.get_csr(l, "Ac")
        assert Ac.shape[0] == int(g["l%d_Ac_dim" % l][0])
        assert np.isclose(Ac.diagonal().sum(), g["l%d_Ac_trace" % l][0], rtol=1e-7)  # 1e6 coefficient jumps: eigenvectors agree to ~cond*eps
        assert np.isclose(np.sqrt(Ac.multiply(Ac).sum()), g["l%d_Ac_fro" % l][0], rtol=1e-7)
    if "vcycle_x" in g.files:
        x = h.vcycle(prob.b)
        assert np.linalg.norm(x - g["vcycle_x"]) <= 1e-10 * np.linalg.norm(g["vcycle_x"])
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-6)
    assert conv and it == int(g["pcg_iters"][0])
    assert np.allclose(hist[:2], g["pcg_hist"][:2], rtol=1e-9)
    assert np.linalg.norm(x - g["pcg_x"]) <= 1e-8 * np.linalg.norm(g["pcg_x"])
    h.close()


@pytest.mark.parametrize("levels", [2, 3])
def test_properties_32cubed(levels):
    """Size-independent checks at a size the python oracle does not reach quickly."""
    capi = _capi()
    cb = [(2, 2, 2)] if levels == 3 else None
    prob = pr.poisson3d_problem((32, 32, 32), blk=(8, 8, 4), coarse_blk=cb, coef="checkerboard")
    # coarse_rtol: converge the inner coarsest PCG fully so that the cycle is a *linear* operator
    params = capi.default_params(num_coarsenings=levels - 1, keep_debug=True, coarse_rtol=1e-28)
    h = capi.Hierarchy.from_problem(prob, params)
    rng = np.random.default_rng(7)
    for l in range(levels - 1):
        A, P, R, Ac = (h.get_csr(l, w) for w in ("A", "P", "R", "Ac"))
        info = h.level_info(l)
        # coarse dims are consistent, P^T P = I (orthonormal MIS blocks), R = P^T exactly
        mises, k, ncols, flags = h.get_mis(l)
        assert k.sum() == info["ncoarse"] == P.shape[1]
        assert abs(P - R.T).max() == 0.0
        PtP = (P.T @ P).toarray()
        assert np.allclose(PtP, np.eye(P.shape[1]), atol=1e-11)
        # Galerkin product and symmetry
        ref = (P.T @ A @ P).toarray()
        assert np.allclose(Ac.toarray(), ref, atol=1e-12 * np.abs(ref).max())
        assert abs(Ac - Ac.T).max() <= 1e-12 * abs(Ac).max()
        # essential rows of P vanish (contrib_filter_boundary) on the finest level
        if l == 0:
            assert abs(P[prob.ess]).max() == 0.0
        # every AE contributed at least one vector (atleast_one)
        m, ev, X, Ds = h.get_ae_eigens(l)
        assert m.min() >= 1
        for e in ev:
            assert np.all(np.diff(e) >= -1e-14) and (len(e) == 1 or e[-1] <= params.theta[l] + 1e-12)
    # the V-cycle is a symmetric positive definite, linear operator
    u = rng.standard_normal(prob.ND) * (~prob.ess)
    v = rng.standard_normal(prob.ND) * (~prob.ess)
    Bu, Bv = h.vcycle(u), h.vcycle(v)
    assert abs(Bu @ v - u @ Bv) <= 1e-9 * abs(Bu @ v)
    assert Bu @ u > 0
    assert np.linalg.norm(h.vcycle(2.0 * u - 3.0 * v) - (2.0 * Bu - 3.0 * Bv)) <= 1e-9 * np.linalg.norm(Bu)
    # PCG: converged means the TRUE residual is small
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    assert conv and it < 60
    assert np.all(np.diff(hist) < 0)
    assert np.linalg.norm(prob.A @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)
    h.close()


def test_edge_cases():
    capi = _capi()
    # one AE only (no interface MIS), tiny theta -> the single smallest pair per AE
    prob = pr.poisson3d_problem((3, 3, 3), blk=(3, 3, 3))
    h = capi.Hierarchy.from_problem(prob, capi.default_params(theta=1e-12, keep_debug=True))
    m, ev, X, Ds = h.get_ae_eigens(0)
    assert list(m) == [1]
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-10)
    assert conv and np.linalg.norm(prob.A @ x - prob.b) <= 1e-8 * np.linalg.norm(prob.b)
    h.close()
    # ragged partition: AEs of 1 .. many elements, MISes of size 1, all-essential MISes on the boundary
    prob = pr.poisson3d_problem((5, 4, 3), blk=(2, 3, 2))
    part = prob.partitions[0].copy()
    part[0] = part.max() + 1            # a single-element AE in the corner
    prob.partitions = [part]
    h = capi.Hierarchy.from_problem(prob, capi.default_params(keep_debug=True))
    mises, k, ncols, flags = h.get_mis(0)
    I, J = h.get_table(0, "mis_to_dof")
    sizes = np.diff(I)
    ess_all = np.array([np.all(prob.ess[J[I[i]:I[i + 1]]]) for i in range(len(sizes))])
    assert np.all(k[ess_all] == 0)                      # skipped (contrib.cpp:578-605)
    assert np.all(k[(sizes == 1) & ~ess_all] == 1)      # size-1 MIS -> [1]
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-10)
    assert conv and np.linalg.norm(prob.A @ x - prob.b) <= 1e-8 * np.linalg.norm(prob.b)
    h.close()
    # error behaviour: bad partition ids are reported, not crashed on
    bad = pr.poisson3d_problem((4, 4, 4), blk=(2, 2, 2))
    p2 = bad.partitions[0].copy()
    p2[3] = 1000
    bad.partitions = [p2]
    params = capi.default_params()
    with pytest.raises(RuntimeError):
        e2d = np.ascontiguousarray(bad.elem_to_dof, dtype=np.int32)
        A = bad.A.tocsr()
        capi.Hierarchy(np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32),
                       np.ascontiguousarray(A.data), A.shape[0], e2d, np.ascontiguousarray(bad.elmat),
                       np.ascontiguousarray(bad.bdr), [p2.astype(np.int32)], [8], params, e2d.shape[0], 8)


def test_one_stage_and_two_stage_eigensolvers_agree():
    """The dense path (saamge_amd_params.eigensolver = 1) with the one-stage blocked Householder kernel
    (saamge_amd_options.eig_dense_one_stage) and with the two-stage band reduction, and the few-eigenpairs path on every
    agglomerate size: every path must give the same hierarchy (coarse dims) and PCG history."""
    code = (
        "import sys, json; sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "from saamge_amd import capi, problems as pr\n"
        "prob = pr.poisson3d_problem((16,16,8), blk=(8,8,4))\n"
        "import os\n"
        "h = capi.Hierarchy.from_problem(prob, capi.default_params(coarse_rtol=1e-28, eigensolver=os.environ.get('EIGSOLVER', 'subspace')))\n"
        "x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)\n"
        "print(json.dumps({'nc': h.level_info(0)['ncoarse'], 'it': it, 'hist': list(hist)}))\n" % ROOT)
    import json
    outs = []
    # the dense path: one-stage kernel, two-stage band reduction
    variants = [{"EIGSOLVER": "dense", "SAAMGE_AMD_TEST_OPTIONS": "eig_dense_one_stage=1"}, {"EIGSOLVER": "dense"}]
    # the few-eigenpairs path (Cholesky + shift-invert subspace iteration) on every agglomerate size
    # (strict: giving up on a batch is an error instead of the silent dense fallback), with and without the
    # known-null-vector shortcut and without the inertia certificate's kept factor
    variants += [{"SAAMGE_AMD_TEST_OPTIONS": "eig_min_n=0,eig_strict=1"},
                 {"SAAMGE_AMD_TEST_OPTIONS": "eig_min_n=0,eig_strict=1,eig_nullcheck=0"},
                 {"SAAMGE_AMD_TEST_OPTIONS": "eig_min_n=0,eig_strict=1,eig_keep_inertia_factor=0"}]
    for extra in variants:
        env = dict(os.environ, **extra)
        o = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert o.returncode == 0, o.stderr[-2000:]
        outs.append(json.loads(o.stdout.strip().splitlines()[-1]))
    for other in outs[1:]:
        assert outs[0]["nc"] == other["nc"] and outs[0]["it"] == other["it"]
        assert np.allclose(outs[0]["hist"], other["hist"], rtol=1e-8)


@pytest.mark.parametrize("case", ["poisson3d", "mltest1", "mltest2", "random_partition"])
def test_device_resident_inputs_build_the_same_hierarchy(case):
    """Level-0 inputs handed over as DEVICE pointers take the device build of the AE tables
    (csrc/topology.hip: build_relations_ae_device); host pointers take the host build.  Both must
    give bit-identical topology (first-encounter orders included) and the same P / Ac."""
    import torch
    capi = _capi()
    if case == "poisson3d":
        prob = pr.poisson3d_problem((12, 8, 8), blk=(4, 4, 2), coarse_blk=[(2, 2, 2)], coef="checkerboard")
        nco = 2
    elif case == "random_partition":
        prob = pr.poisson3d_problem((6, 5, 4), blk=(3, 5, 2))
        rng = np.random.default_rng(5)
        part = rng.integers(0, 7, size=prob.elem_to_dof.shape[0]).astype(np.int32)
        part[:7] = np.arange(7)                      # no empty agglomerate
        prob.partitions = [part]
        nco = 1
    else:
        prob = pr.mltest_problem(order=int(case[-1]), levels=3)
        nco = 2
    params = capi.default_params(num_coarsenings=nco, keep_debug=True, testmesh=case.startswith("mltest"))
    h_host = capi.Hierarchy.from_problem(prob, params)
    A = prob.A.tocsr()
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).cuda()
    e2d = np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32)
    parts = [np.ascontiguousarray(p_, dtype=np.int32) for p_ in prob.partitions[:nco]]
    nparts = [int(p_.max()) + 1 for p_ in parts]
    parts_in = [dev(parts[0], np.int32)] + parts[1:]
    params2 = capi.default_params(num_coarsenings=nco, keep_debug=True, testmesh=case.startswith("mltest"))
    h_dev = capi.Hierarchy(dev(A.indptr, np.int32), dev(A.indices, np.int32), dev(A.data, np.float64),
                           A.shape[0], dev(e2d, np.int32), dev(prob.elmat, np.float64),
                           dev(prob.bdr, np.int8), parts_in, nparts, params2, e2d.shape[0], e2d.shape[1])
    for lev in range(nco):
        for name in ("AE_to_dof", "dof_to_AE", "mis_to_dof", "mis_to_AE", "AE_to_mis", "elem_to_dof"):
            Ih, Jh = h_host.get_table(lev, name)
            Id, Jd = h_dev.get_table(lev, name)
            assert np.array_equal(Ih, Id) and np.array_equal(Jh, Jd), (lev, name)
        mh, md = h_host.get_mis(lev), h_dev.get_mis(lev)
        for a, b in zip(mh, md):
            assert np.array_equal(a, b)
        for which in ("P", "Ac"):
            Mh, Md = h_host.get_csr(lev, which), h_dev.get_csr(lev, which)
            assert np.array_equal(Mh.indices, Md.indices) and np.array_equal(Mh.data, Md.data), (lev, which)
    h_host.close()
    h_dev.close()


def test_dense_and_iterative_coarsest_solvers_agree():
    """Coarsest solve: dense Cholesky (the reference's serial --coarse-direct) and
    the inner PCG to 1e-28 give the same V-cycle and the same PCG run; the Cholesky path is
    exercised over many 64-column blocks (coarse dim > 1000)."""
    capi = _capi()
    prob = pr.poisson3d_problem((32, 32, 16), blk=(4, 4, 2))
    out = {}
    for kind in (1, 2):
        h = capi.Hierarchy.from_problem(prob, capi.default_params(coarse_solver=kind, coarse_rtol=1e-28))
        assert h.level_info(0)["ncoarse"] > 1000
        assert h.coarse_solver_info()["kind"] == kind
        b = np.cos(np.arange(prob.ND) * 0.21) * (~prob.ess)
        x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
        out[kind] = (h.vcycle(b), x, it, h.level_info(0)["coarse_iters"])
        assert conv
        h.close()
    assert out[1][3] == 0 and out[2][3] > 0          # direct vs iterative really ran
    assert out[1][2] == out[2][2]
    for i in (0, 1):
        assert np.linalg.norm(out[1][i] - out[2][i]) <= 1e-9 * np.linalg.norm(out[2][i])


@pytest.mark.parametrize("variant", ["plain", "nu_pro", "nullspace"])
def test_update_operators_keeps_interpolation(variant):
    """adapt_update_operators (src/adapt.cpp:171-219): new matrix values, same pattern -- every P is
    kept (no eigenproblem is solved again), all Galerkin operators, smoother diagonals and the
    coarsest solver follow the new matrix."""
    capi = _capi()
    prob = pr.poisson3d_problem((12, 8, 8), blk=(4, 4, 2), coarse_blk=[(2, 2, 2)], coef="checkerboard")
    kw = {"nu_pro": 1} if variant == "nu_pro" else ({"correct_nullspace": True} if variant == "nullspace" else {})
    params = capi.default_params(num_coarsenings=2, keep_debug=True, coarse_rtol=1e-28, **kw)
    h = capi.Hierarchy.from_problem(prob, params)
    nlev = h.num_levels - 1
    P_before = [h.get_csr(l, "P") for l in range(nlev)]
    A = prob.A.tocsr()
    A.sort_indices()
    A2 = A.copy()                                          # SPD, same pattern (explicit zeros kept), new values
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    A2.data = np.where(A.indices == rows, 1.5 * A.data, A.data * (1.0 + 0.1 * np.cos(rows + A.indices)))
    h.update_operators(A2.data)
    Al = A2
    for l in range(nlev):
        A_l, P, R, Ac = (h.get_csr(l, w) for w in ("A", "P", "R", "Ac"))
        assert abs(A_l - Al).max() <= 1e-12 * abs(Al).max()
        if variant != "nu_pro" or l == nlev:                # tentative P (and scaling_P) untouched
            assert np.array_equal(P.data, P_before[l].data) and np.array_equal(P.indices, P_before[l].indices)
        assert abs(P - R.T).max() == 0.0
        ref = (P.T @ A_l @ P).toarray()
        assert np.allclose(Ac.toarray(), ref, rtol=0, atol=1e-12 * np.abs(ref).max())
        Al = Ac
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    assert conv and np.linalg.norm(A2 @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)
    # same result as a hierarchy whose operators were rebuilt by hand from the kept P: the V-cycle is
    # linear, symmetric and uses the new smoother diagonals
    u, v = np.cos(np.arange(prob.ND) * 0.3) * (~prob.ess), np.sin(np.arange(prob.ND) * 0.2) * (~prob.ess)
    Bu, Bv = h.vcycle(u), h.vcycle(v)
    assert abs(v @ Bu - u @ Bv) <= 1e-9 * abs(v @ Bu)
    h.close()


def test_update_operators_chooses_the_coarsest_solver_again():
    """tg_update_coarse_operator(A, tg_data, perform_solve_init, coarse_direct) (inc/tg.hpp:610-612): the update sets
    the coarsest solver up again as coarse_direct says -- saamge_amd_update_operators2(h, val, 1 | 2).  Built with the
    explicit inverse; updated with the same values and coarse_solver = 2 the coarsest level is solved by the inner PCG
    (its iteration count shows in level_info), updated again with 1 it is the inverse again; the solutions agree."""
    capi = _capi()
    prob = pr.poisson3d_problem((12, 8, 8), blk=(4, 4, 2), coef="checkerboard")
    params = capi.default_params(num_coarsenings=1, coarse_rtol=1e-28, coarse_solver=1)
    h = capi.Hierarchy.from_problem(prob, params)
    A = prob.A.tocsr()
    A.sort_indices()
    res = []
    for kind in (None, 2, 1):
        if kind is not None:
            h.update_operators(A.data, coarse_solver=kind)
        x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-10)
        res.append((x, it, h.level_info(0)["coarse_iters"]))
        assert conv
    assert res[0][2] == 0 and res[1][2] > 0 and res[2][2] == 0          # direct, inner PCG, direct again
    assert res[0][1] == res[1][1] == res[2][1]
    for x, _, _ in res[1:]:
        assert np.linalg.norm(x - res[0][0]) <= 1e-9 * np.linalg.norm(res[0][0])
    with pytest.raises(Exception):
        h.update_operators(A.data, coarse_solver=7)
    h.close()


def test_hierarchy_on_a_nonzero_device():
    """The library's worker threads, helper streams and cached device blocks follow the CALLER's current device
    (round-1 advisor finding: HIP's current device is per host thread).  Needs a second visible GPU; on the one-GPU
    test box this is skipped, on a multi-GPU node it builds and solves on device 1 and compares with device 0."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible GPU")
    from saamge_amd import capi, problems
    out = []
    for dev in (0, 1):
        torch.cuda.set_device(dev)
        prob = problems.poisson3d_device((32, 32, 16), blk=(8, 8, 4), coarse_blk=[(2, 2, 2)], device="cuda:%d" % dev)
        params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3)
        h = capi.Hierarchy(prob.rowptr, prob.col, prob.val, prob.n, prob.elem_to_dof, prob.elmat, prob.bdr,
                           prob.partitions, prob.nparts, params, prob.NE_, 8)
        x = torch.zeros_like(prob.b)
        _, it, conv, hist = h.pcg(prob.b, x, rel_tol=1e-8, max_iter=100)
        assert conv
        out.append((it, [h.level_info(l)["ncoarse"] for l in range(2)], x.cpu().numpy()))
        h.close()
    torch.cuda.set_device(0)
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert np.allclose(out[0][2], out[1][2], rtol=0, atol=1e-12 * np.abs(out[0][2]).max())
