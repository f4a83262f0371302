"""CPU checks of tests/coarse_cases.py: the case builders, the host model of blocktri.hip's level structure and the
high-precision reference solve that tests/test_gpu_coarse_solvers.py judges the device solvers with.  The coarse operator
the library builds exists only on the GPU; here every case is looked at through the operator it is expected to produce
(piecewise constant orthonormal P on the case's agglomerates)."""
import numpy as np
import pytest
import scipy.sparse as sp

import coarse_cases as cc

CASES = cc.catalogue()


@pytest.fixture(scope="module")
def expected():
    cache = {}

    def get(name):
        if name not in cache:
            Ac = cc.expected_coarse_operator(CASES[name]["graph"], CASES[name]["shift"])
            cache[name] = (Ac, cc.level_blocks(Ac))
        return cache[name]
    return get


def test_the_catalogue_has_every_row_of_the_table():
    want = ["one_row", "two_rows", "small_grid_255", "small_grid_256", "small_grid_257", "small_grid_640", "path", "rod", "rod_stiff", "slab",
            "cube", "cube_stiff", "two_components", "three_components_uneven", "star", "permuted_cube", "too_wide",
            "semidefinite", "updated"]
    want += ["dense_edges_%d" % n for n in (cc.DNB - 1, cc.DNB, cc.DNB + 1, 2 * cc.DNB - 1, 2 * cc.DNB + 1, 3 * cc.DNB + 5,
                                            1000, 4097)]
    assert set(want) <= set(CASES)
    # kind 1 is left out exactly where the operator is beyond one dense inverse
    for name, case in CASES.items():
        assert (1 in case["kinds"]) == (case["graph"][0] <= cc.DENSE_MAX), name
    assert [n for n, c in CASES.items() if 1 not in c["kinds"]] == ["too_wide"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_builder_gives_a_symmetric_operator_with_the_stated_components(name):
    case = CASES[name]
    A, part = cc.build(case)
    assert A.shape[0] == A.shape[1] == part.size < 200000
    assert abs(A - A.T).max() == 0.0
    assert A.has_sorted_indices
    assert cc.num_components(A) == case["components"]
    nc = case["graph"][0]
    assert part.min() == 0 and part.max() == nc - 1 and np.all(np.bincount(part) >= 2)
    # every agglomerate is connected (its local Laplacian then has ONE zero eigenvalue: one coarse vector)
    same = part[A.tocoo().row] == part[A.tocoo().col]
    inner = sp.coo_matrix((np.ones(int(same.sum())), (A.tocoo().row[same], A.tocoo().col[same])), shape=A.shape)
    assert cc.num_components(inner) == nc
    # the agglomerate graph is the case's graph
    Q = sp.csr_matrix((np.ones(part.size), (np.arange(part.size), part)), shape=(part.size, nc))
    G = (Q.T @ abs(A) @ Q).tocoo()
    n, edges = case["graph"]
    if case["seed"] is None:
        got = {(int(i), int(j)) for i, j in zip(G.row, G.col) if i < j}
        assert got == {(int(min(a, b)), int(max(a, b))) for a, b in edges}
    d = A.diagonal()
    off = np.asarray(abs(A).sum(axis=1)).ravel() - d
    if case["shift"] > 0:
        assert np.all(d > off)                                 # strictly diagonally dominant: positive definite
    else:
        assert np.allclose(d, off) and abs(A @ np.ones(A.shape[0])).max() < 1e-12      # singular, constants in the kernel


@pytest.mark.parametrize("name", sorted(CASES))
def test_level_blocks_gives_a_block_tridiagonal_structure(name, expected):
    case = CASES[name]
    Ac, lb = expected(name)
    assert Ac.shape[0] == case["graph"][0]
    assert cc.num_components(Ac) == case["components"]
    cc.check_block_tridiagonal(Ac, lb)
    ex = case["expect"]
    assert lb["refused"] == bool(ex.get("refused", False))
    for key in ("nblk", "max_block"):
        if key in ex:
            assert lb[key] == ex[key], (key, lb[key])
    if "min_levels" in ex:
        assert lb["nlev"] >= ex["min_levels"]
    if "far_wins" in ex:
        assert lb["far_wins"] == ex["far_wins"] and lb["cost_far"] < lb["cost_vertex"]
    if 1 in case["kinds"]:
        assert Ac.shape[0] <= cc.DENSE_MAX


def test_the_shapes_the_cases_are_meant_to_reach(expected):
    """what the right-hand column of the case table says, on the model"""
    lb = expected("path")[1]
    assert np.array_equal(np.diff(lb["off"]), [256] * 10 + [256 + 184]) and np.all(lb["level_sizes"] == 1)
    lb = expected("rod")[1]
    assert np.sum(lb["level_sizes"] == 16) >= 590 and lb["nblk"] >= 36 and lb["max_block"] < 2 * cc.BT_MIN_BLOCK
    for name in ("cube", "cube_stiff", "permuted_cube", "updated"):
        lb = expected(name)[1]
        assert lb["far_wins"] and np.all(lb["level_sizes"] == 576) and lb["nblk"] == 26, name
    lb = expected("slab")[1]
    assert lb["far_wins"] and np.all(lb["level_sizes"] == 180) and np.all(np.diff(lb["off"]) == 360)
    # several components: some block holds rows of two of them, and the row of Ac that starts a component has no entry in the
    # previous block although it is not in the first one
    for name in ("two_components", "three_components_uneven"):
        Ac, lb = expected(name)
        comp = sp.csgraph.connected_components(Ac, directed=False)[1]
        mixed = [k for k in range(lb["nblk"]) if len(set(comp[lb["block"] == k])) > 1]
        assert mixed, name
        co = Ac.tocoo()
        has_lower = np.zeros(Ac.shape[0], bool)
        has_lower[co.row[lb["block"][co.col] == lb["block"][co.row] - 1]] = True
        assert np.any(~has_lower & (lb["block"] > 0)), name
    Ac, lb = expected("star")
    assert lb["nlev"] == 3 and np.diff(Ac.indptr).max() == Ac.shape[0] == 1500
    Ac, lb = expected("too_wide")
    assert Ac.shape[0] > cc.DENSE_MAX and lb["refused"] and lb["level_sizes"].max() > cc.BT_MAX_BLOCK and np.diff(Ac.indptr).max() <= 9
    # block sizes that are no multiples of the kernels' strides
    sizes = np.concatenate([np.diff(expected(n)[1]["off"]) for n in ("dense_edges_1000", "dense_edges_4097", "two_components")])
    assert np.any(sizes % 4 != 0) and np.any(sizes % 8 != 0) and np.any(sizes % 64 != 0) and np.any(sizes % 128 != 0)


def test_extended_residual_paths_agree_and_beat_fp64():
    """long double (where it has 64 significand bits) and the double-double fallback give the same residual; both see what
    plain fp64 does not"""
    A = cc.expected_coarse_operator(cc.grid_graph(7, 9, 5), cc.STIFF)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(A.shape[0])
    b = A @ x                                       # fp64: the true residual is pure round-off, ~1e-16 |A| |x|
    r_dd = cc.residual_ext(A, x, b, force_dd=True)
    hi, lo = cc._residual_dd(A, x, b)
    scale = cc.norm_inf_op(A) * np.abs(x).max()
    assert np.abs(lo).max() <= 1e-30 * scale + np.abs(hi).max() * 2.0 ** -52
    # exact check on data whose products and sums are exactly representable
    n, edges = cc.grid_graph(6, 5, 4)
    Ai = cc.graph_laplacian(n, edges, 2.0 ** -20)
    xi = rng.integers(-1000, 1000, n).astype(np.float64)
    bi = Ai @ xi
    assert np.all(cc.residual_ext(Ai, xi, bi, force_dd=True) == 0.0) and np.all(cc.residual_ext(Ai, xi, bi) == 0.0)
    bi[3] += 2.0 ** -30
    assert cc.residual_ext(Ai, xi, bi, force_dd=True)[3] == 2.0 ** -30
    if cc.HAVE_LONGDOUBLE:
        r_ld = cc.residual_ext(A, x, b)
        assert np.abs(r_ld - r_dd).max() <= 2.0 ** -60 * scale
        assert np.abs(r_dd).max() > 0.0
    # an empty row sums to zero
    E = sp.csr_matrix(([1.0], ([0], [0])), shape=(2, 2))
    assert np.array_equal(cc.residual_ext(E, np.ones(2), np.array([3.0, 5.0])), [2.0, 5.0])
    assert np.array_equal(cc.residual_ext(E, np.ones(2), np.array([3.0, 5.0]), force_dd=True), [2.0, 5.0])


@pytest.mark.parametrize("shape", [(4, 4, 600), (24, 24, 26, True)])
def test_reference_solve_reproduces_a_manufactured_solution_on_stiff_operators(shape):
    """The stiff shapes with data that make the right-hand side EXACT: unit weights, shift 2^-20, integer solution.  The
    reference must reach the accuracy it claims (condition estimate times its own residual) and be far more accurate than
    a plain fp64 LU solve with one refinement step."""
    n, edges = cc.grid_graph(*shape)
    A = cc.graph_laplacian(n, edges, 2.0 ** -20)
    x_true = np.random.default_rng(5).integers(-1000, 1000, n).astype(np.float64)
    b = A @ x_true
    assert np.all(cc.residual_ext(A, x_true, b, force_dd=True) == 0.0)          # b is exact
    head, tail, res = cc.reference_solve(A, b)
    cond = cc.cond_estimate(A)
    assert cond > 1e5
    err = float(np.abs((head - x_true) + tail).max() / np.abs(x_true).max())
    plain = cc.forward_error(cc.lu_shaped_solve(A, b), x_true)
    print("shape %s: cond %.2e, reference residual %.2e, reference error %.2e, LU + one step %.2e" % (shape, cond, res, err, plain))
    assert res <= 1e-18
    assert err <= cond * res + 1e-300          # (exact data: the double-double refinement may end on the very solution)
    assert 100.0 * err <= plain           # ... and is two orders better than the fp64 solve it serves to judge


def test_reference_solve_on_tiny_and_well_conditioned_operators():
    for g in (cc.grid_graph(1), cc.grid_graph(2), cc.grid_graph(5, 13)):
        Ac = cc.expected_coarse_operator(g, cc.WELL)
        lb = cc.level_blocks(Ac)
        for name, rc in cc.right_hand_sides(Ac, lb).items():
            head, tail, res = cc.reference_solve(Ac, rc)
            assert res <= 1e-18, (g[0], name, res)
            assert cc.backward_error(Ac, head, rc) <= 2.0 ** -52
