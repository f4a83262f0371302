"""The scenario driver of the MFEM adaptor (tests/cxx/mfem_adaptor_run, built next to the library) as far as it goes without a
GPU: it links the library, the container format survives a round trip between Python and the driver, the stand-in's Table
Transpose / Mult agree with scipy, and every refusal of include/saamge_amd_mfem.hpp that needs no hierarchy says what it should.
None of these scenarios creates a hierarchy."""
import numpy as np
import pytest
import scipy.sparse as sp

import adaptor_cases as ac


def _random_table(rng, rows, cols, empty_rows=()):
    M = sp.random(rows, cols, density=0.3, random_state=rng, format="lil")
    for r in empty_rows:
        M[r, :] = 0
    M = sp.csr_matrix(M)
    M.eliminate_zeros()
    J = M.indices.astype(np.int32).copy()
    for r in range(rows):                      # columns in no order
        J[M.indptr[r]:M.indptr[r + 1]] = rng.permutation(J[M.indptr[r]:M.indptr[r + 1]])
    return M.indptr.astype(np.int32), J


def _rows(I, J):
    return [sorted(int(c) for c in J[I[r]:I[r + 1]]) for r in range(len(I) - 1)]


def _bool(I, J, cols):
    return sp.csr_matrix((np.ones(len(J), dtype=np.int64), J, I), shape=(len(I) - 1, cols))


def test_container_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    arrays = {"ints": rng.integers(-2 ** 31, 2 ** 31 - 1, 1001).astype(np.int32),
              "doubles": np.concatenate([rng.standard_normal(77), [np.inf, -0.0, 5e-324, np.nan]]),
              "bytes": rng.integers(-128, 127, 13).astype(np.int8), "longs": np.array([2 ** 40 + 3, -7], dtype=np.int64),
              "empty": np.zeros(0), "scalar": np.float64(0.1), "a name with spaces.and.dots": np.int32(-1)}
    ac.write_container(tmp_path / "in.bin", arrays)
    back = ac.read_container(tmp_path / "in.bin")
    out = ac.run_driver(tmp_path / "in.bin", ["roundtrip"], tmp_path / "out.bin")
    assert list(out) == ["roundtrip." + k for k in arrays] and list(back) == list(arrays)
    for k, a in arrays.items():
        a = np.atleast_1d(a)
        for got in (back[k], out["roundtrip." + k]):
            assert got.dtype == a.dtype and got.tobytes() == a.tobytes(), k


@pytest.mark.parametrize("seed,shape", [(0, (7, 5, 9)), (1, (1, 1, 1)), (2, (12, 30, 4)), (3, (30, 3, 17))])
def test_stand_in_tables_match_scipy(tmp_path, seed, shape):
    """Table built in two passes (MakeI / AddAColumnInRow / MakeJ / AddConnection / ShiftUpI), its copy, SetDims, RowSize,
    Transpose and the boolean product Mult: unique columns per row, in any order; rows without a connection included."""
    rng = np.random.default_rng(seed)
    m, k, n = shape
    AI, AJ = _random_table(rng, m, k, empty_rows=(0,) if m > 1 else ())
    BI, BJ = _random_table(rng, k, n, empty_rows=(k - 1,) if k > 1 else ())
    ac.write_container(tmp_path / "in.bin", {"tA.I": AI, "tA.J": AJ, "tB.I": BI, "tB.J": BJ})
    out = ac.run_driver(tmp_path / "in.bin", ["tables"], tmp_path / "out.bin")
    for name in ("A", "setdims"):
        assert np.array_equal(out["tables.%s.I" % name], AI) and np.array_equal(out["tables.%s.J" % name], AJ)
    assert np.array_equal(out["tables.A.rowsize"], np.diff(AI))
    A, B = _bool(AI, AJ, k), _bool(BI, BJ, n)
    # the transpose has as many rows as the largest column that occurs, like MFEM's with ncols_A = -1
    At = sp.csr_matrix(A.T)
    At.sort_indices()
    want = _rows(At.indptr, At.indices)[:int(AJ.max()) + 1 if len(AJ) else 0]
    got = _rows(out["tables.At.I"], out["tables.At.J"])
    assert got == want
    assert len(out["tables.At.J"]) == len(AJ)
    AB = sp.csr_matrix(A @ B)
    AB.eliminate_zeros()
    AB.sort_indices()
    got = out["tables.AB.I"], out["tables.AB.J"]
    assert _rows(*got) == _rows(AB.indptr, AB.indices)
    assert len(got[1]) == AB.nnz                     # (every column once)


def test_csr_of_sorts_rows_with_their_values(tmp_path):
    """detail::csr_of on a matrix given the way hypre keeps a diagonal block -- the diagonal entry first, the rest in no order,
    explicit zeros kept: ascending columns per row, every value still with its column, the offsets untouched."""
    from saamge_amd import problems as pr
    A = pr.poisson3d_problem((3, 4, 2), blk=(3, 2, 2)).A
    rowptr, col, val = ac.diag_first_unsorted(A)
    assert any(np.any(np.diff(col[rowptr[i]:rowptr[i + 1]]) < 0) for i in range(A.shape[0]))      # (there is work to do)
    assert all(col[rowptr[i]] == i for i in range(A.shape[0]))
    ac.write_container(tmp_path / "in.bin", {"A_rowptr": rowptr, "A_col": col, "A_val": val})
    out = ac.run_driver(tmp_path / "in.bin", ["csr_of"], tmp_path / "out.bin")
    S = sp.csr_matrix(A)
    S.sort_indices()
    assert np.array_equal(out["csr_of.I"], S.indptr) and np.array_equal(out["csr_of.J"], S.indices)
    assert out["csr_of.V"].tobytes() == S.data.astype(np.float64).tobytes()
    assert np.count_nonzero(S.data == 0.0) > 0          # (the eliminated entries are stored zeros, and stay)


def test_element_matrix_gather_keeps_the_index_order(tmp_path):
    """detail::pack_element_matrices on NON-symmetric element matrices of two sizes: entry (a, b) of element e lands row-major at
    its offset, through a column-major DenseMatrix (from the form, deleted by the adaptor) and through a provider's own Matrix
    class (its own storage: nothing deleted; copies: one per element).  A transposed gather or a row / column-major slip shows."""
    rng = np.random.default_rng(11)
    elem_ptr = np.array([0, 3, 7, 10, 14], dtype=np.int32)
    nd = np.diff(elem_ptr)
    elmat = rng.standard_normal(int((nd * nd).sum()))
    n = 6
    e2d = np.concatenate([rng.permutation(n)[:k] for k in nd]).astype(np.int32)
    ac.write_container(tmp_path / "in.bin", {"A_rowptr": np.arange(n + 1, dtype=np.int32), "A_col": np.arange(n, dtype=np.int32),
                                             "A_val": np.ones(n), "elem_ptr": elem_ptr, "elem_to_dof": e2d, "elmat": elmat,
                                             "e2e_I": np.zeros(len(nd) + 1, dtype=np.int32), "e2e_J": np.zeros(0, dtype=np.int32),
                                             "bdr_attribute": np.zeros(n, dtype=np.int32)})
    out = ac.run_driver(tmp_path / "in.bin", ["gather"], tmp_path / "out.bin")
    for k in ("dense", "own", "copies"):
        assert out["gather." + k].tobytes() == elmat.tobytes(), k
    assert out["gather.own_deleted"].tolist() == [0] and out["gather.copies_deleted"].tolist() == [len(nd)]
    off = 0
    for k in nd:          # (the data really is non-symmetric)
        M = elmat[off:off + k * k].reshape(k, k)
        assert not np.array_equal(M, M.T)
        off += k * k


REFUSALS = {
    "mixed_and_distributed": "ml_produce_data: elements with different numbers of dofs are not supported on the per-rank path",
    "null_partitioning": "agg_create_partitioning_fine: a partitioning array is required",
    "csr_of_distributed": "saamge_amd: the HypreParMatrix is distributed over several MPI ranks (global size != local size)",
    "algebraic_distributed": "saamge_amd: the HypreParMatrix is distributed over several MPI ranks (global size != local size)",
    "distributed_without_dof_truedof": "ml_produce_data: a distributed HypreParMatrix needs agg_create_partitioning_fine's dof_truedof",
    "algebraic_ne_not_nd": "tg_produce_data_algebraic: agg_part_rels must map every dof to its AE (NE = ND)",
    "build_twice": "tg_build_hierarchy: this tg_data already holds a hierarchy",
    "build_without_elem_data": "tg_build_hierarchy: coarse-level construction (elem_data == NULL)",
    "fillin_without_interp": "tg_fillin_coarse_operator: no interpolation",
    "fillin_null": "tg_fillin_coarse_operator: no interpolation",
    "vcycle_on_level_1": "VCycleSolver: only the finest level's tg_data can be cycled from outside",
    "set_operator_not_hypre": "VCycleSolver::SetOperator : not HypreParMatrix!",
    "pcg_foreign_preconditioner": "kalchev_pcg: B must be a saamge::VCycleSolver of this library",
    "pcg_zero_rhs": "kalchev_pcg: zero_rhs (A-norm stopping rule) is not supported",
    "local_to_true_orphan": "saamge_amd: a local dof without a true dof in Dof_TrueDof",
}


@pytest.fixture(scope="module")
def refusals(tmp_path_factory):
    d = tmp_path_factory.mktemp("refusals")
    ac.write_container(d / "in.bin", {})
    return ac.run_driver(d / "in.bin", ["refusals"], d / "out.bin")


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusal_message(refusals, case):
    """Each refusal is the message mfem_error was called with (the stand-in throws it); a call that went through says
    "NOT REFUSED"."""
    assert ac.text(refusals["refusals." + case]).startswith(REFUSALS[case])


def test_local_to_true_and_single_rank_mpi(refusals):
    """detail::local_to_true on a hand-made Dof_TrueDof: 5 local dofs, rows 0 / 2 / 3 in diag (true dofs 10 + column), rows 1 / 4
    in offd (through col_map_offd = {3, 7}); and the stand-in's MPI calls: rank 0 of 1, every collective the one-rank copy."""
    assert refusals["refusals.local_to_true.gdof"].tolist() == [12, 7, 10, 11, 3]
    assert refusals["refusals.local_to_true.owned"].tolist() == [1, 0, 1, 1, 0]
    assert refusals["refusals.is_distributed"].tolist() == [1]
    assert refusals["refusals.vcycle_height"].tolist() == [4]
    assert refusals["refusals.mpi"].tolist() == [0.0, 1.0, 41.0, 0.0, 1.5, 2.5, 1.5, 2.5, 0.0, 1.5, 2.5]
