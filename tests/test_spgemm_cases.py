"""CPU checks of tests/spgemm_cases.py: every case has the property it is named for (the distinct-column count of its named row,
the eligibility predicates of the dense-B product, the row lengths on either side of a sort or chunk limit), the inputs respect
what the kernels rely on, and the plain references agree with scipy.  tests/test_gpu_spgemm.py runs the same cases on the
device."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import spgemm_cases as sc

PRODUCTS = sorted(sc.PATTERNS)
TRANSPOSES = sc.transpose_cases()
THRESHOLDS = sc.threshold_cases()


@functools.lru_cache(maxsize=None)
def case(name, family):
    return sc.product_case(name, family)


def test_long_double_has_a_64_bit_significand():
    assert sc.HAVE_LONGDOUBLE            # the general family's reference needs it


def test_the_catalogue_has_every_case_of_the_table():
    want = ["tier0_row_256", "tier1_row_257", "tier1_row_2048", "tier2_row_2049", "tier2_row_8192", "refused_row_8193",
            "hash_cols_2049", "dense_nnz_256n", "hash_nnz_256n_minus_1"]
    want += ["dense_cols_%d" % n for n in (1, 255, 256, 257, 300, 2048)]
    want += ["tier%d_%s" % (t, k) for t in (0, 1) for k in ("E_only", "d_only", "E_and_d", "E_is_B")]
    assert set(want) <= set(PRODUCTS)
    routes = {sc.PATTERNS[n]["expect"] for n in PRODUCTS}
    assert routes == {-1, 0, 1, 2, sc.ROUTE_DENSE, sc.ROUTE_REFUSED}
    assert {sc.PATTERNS[n]["A"].shape[0] for n in PRODUCTS if sc.PATTERNS[n]["kind"] == "pattern"} >= {1, 5, 7}


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("name", PRODUCTS)
def test_product_case_takes_the_route_it_is_named_for(name, family):
    c = case(name, family)
    A, B, E = c["A"], c["B"], c["E"]
    assert A.shape[1] == B.shape[0] and A.shape[0] <= 300
    for M in (A, B) + ((E,) if E is not None else ()):
        assert sc.rows_have_distinct_columns(M)
        assert M.indices.size == 0 or (M.indices.min() >= 0 and M.indices.max() < M.shape[1])
        assert np.all(M.data != 0.0)
    if E is not None:
        assert E.shape == (A.shape[0], B.shape[1])
    assert sc.model_route(A, B, **sc.operands(c)) == c["expect"]
    if c.get("shuffled"):
        assert not sc.rows_are_sorted(A) or not sc.rows_are_sorted(B)
    if "named_count" in c:
        counts = sc.product_row_counts(A, B, E)
        assert counts[c["named_row"]] == c["named_count"] == counts.max()
        assert np.sum(counts == counts.max()) == 1
    if family == "exact":
        for M in (A, B) + ((E,) if E is not None else ()):
            assert np.all(M.data == np.round(M.data)) and np.all(np.abs(M.data) <= 8)
        if c["d"] is not None:
            assert np.all(np.log2(c["d"]) == np.round(np.log2(c["d"])))
        assert c["alpha"] * 4 == round(c["alpha"] * 4) and c["beta"] * 4 == round(c["beta"] * 4)
    elif c["alpha"] != 1.0:
        assert abs(c["alpha"]) == sc.ALPHA_SMOOTH


@pytest.mark.parametrize("name", [n for n in PRODUCTS if sc.PATTERNS[n].get("m")])
def test_long_rows_come_from_overlapping_rows_of_B(name):
    c = case(name, "exact")
    A, B, r = c["A"], c["B"], c["named_row"]
    ks = A.indices[A.indptr[r]:A.indptr[r + 1]]
    lens = np.diff(B.indptr)[ks]
    assert len(ks) >= 24 and np.sum(lens == 0) == 2                       # tens of entries, two of them on empty rows of B
    assert lens[lens > 0].min() >= 90 and lens.max() <= 400
    hits = np.asarray((sc.pattern(A)[r] @ sc.pattern(B)).todense()).ravel()
    assert np.all(hits[c["hot"]] == c["m"])                                # these columns are hit by every entry of the row
    if A.shape[0] > 1:
        assert np.any(np.diff(A.indptr) == 0)                              # an empty row of A
        assert A.shape[0] % 2 == 1 and A.shape[0] % 4 != 0                 # no multiple of the waves per workgroup (4, 2)


@pytest.mark.parametrize("tier", (0, 1, 2))
def test_last_probe_cases_need_every_probe_of_their_table(tier):
    c = case("tier%d_last_probe" % tier, "exact")
    slots = sc.TIERS[tier]
    A, B, r = c["A"], c["B"], c["named_row"]
    ks = A.indices[A.indptr[r]:A.indptr[r + 1]]
    assert np.all(np.diff(ks) > 0)                                         # the row of A is walked in this order
    before = np.concatenate([B.indices[B.indptr[k]:B.indptr[k + 1]] for k in ks[:-1]])
    assert len(before) == len(np.unique(before)) == slots - 1 and np.array_equal(np.sort(before), np.sort(c["first"]))
    assert list(B.indices[B.indptr[ks[-1]]:B.indptr[ks[-1] + 1]]) == [c["last"]]
    assert sc.probes_needed(before, c["last"], slots) == slots
    assert sc.probes_needed(np.append(before, c["last"]), 4 * slots - 1, slots) is None


def test_operand_cases_fill_the_table_with_columns_of_E():
    for tier in (0, 1):
        c = case("tier%d_E_only" % tier, "exact")
        r = c["named_row"]
        without = sc.product_row_counts(c["A"], c["B"])[r]
        with_e = sc.product_row_counts(c["A"], c["B"], c["E"])[r]
        assert without < with_e == sc.TIERS[tier]                         # E brings columns the product does not have
        assert np.any(np.diff(c["E"].indptr) == 0)
        assert c["d"] is None and c["beta"] != 0.0
        assert case("tier%d_d_only" % tier, "exact")["E"] is None and case("tier%d_d_only" % tier, "exact")["d"] is not None
        both = case("tier%d_E_and_d" % tier, "general")
        assert both["E"] is not None and both["d"] is not None
        alias = case("tier%d_E_is_B" % tier, "general")
        assert alias["E"] is alias["B"] and alias["A"].shape[0] == alias["A"].shape[1]


@pytest.mark.parametrize("name", [n for n in PRODUCTS if n.startswith(("dense_", "hash_"))])
def test_dense_cases_and_their_twins_sit_on_the_eligibility_limits(name):
    c = case(name, "exact")
    A, B = c["A"], c["B"]
    n = A.shape[0]
    assert np.sum(np.diff(A.indptr) == 0) >= 2                            # empty rows of A
    lens = np.diff(B.indptr)
    assert np.any(lens[np.unique(A.indices)] == 0)                         # referenced empty rows of B
    if B.shape[1] > 1:
        assert np.setdiff1d(np.arange(B.shape[1]), B.indices).size >= 1   # structurally empty columns
    if name.startswith("dense_cols"):
        assert B.shape == (3000, int(name.rsplit("_", 1)[1])) and np.sum(np.diff(A.indptr) > 500) == 8
    if name == "hash_cols_2049":
        assert B.shape[1] == sc.DENSE_MAX_COLS + 1 and len(A.indices) >= sc.DENSE_MIN_ROW * n
        assert np.any(B.indices == sc.DENSE_MAX_COLS)
    if name == "dense_nnz_256n":
        assert len(A.indices) == sc.DENSE_MIN_ROW * n
    if name == "hash_nnz_256n_minus_1":
        assert len(A.indices) == sc.DENSE_MIN_ROW * n - 1 and B.shape[1] <= sc.DENSE_MAX_COLS
    if "twin_of" in c:
        base = case(c["twin_of"], "exact")
        # the rows and columns the change does not reach: the same operands, so the same product
        rows, nc = c["same_rows"], c["same_cols"]
        assert abs(c["A"][rows] @ c["B"][:, :nc] - base["A"][rows] @ base["B"]).max() == 0
        assert sc.model_route(base["A"], base["B"]) == sc.ROUTE_DENSE


@functools.lru_cache(maxsize=None)
def reference(name, family):
    c = case(name, family)
    return sc.reference_product(c["A"], c["B"], extended=family == "general", **sc.operands(c))


@pytest.mark.parametrize("name", ["tier0_row_256", "tier1_E_and_d", "tier0_E_is_B", "dense_cols_257", "hash_nnz_256n_minus_1", "no_rows"])
def test_reference_product_agrees_with_scipy(name):
    for family in sc.FAMILIES:
        c = case(name, family)
        C, bound = reference(name, family)
        assert sc.rows_are_sorted(C) and len(bound) == len(C.data)
        assert np.array_equal(np.diff(C.indptr), sc.product_row_counts(c["A"], c["B"], c["E"]))     # the structural pattern
        D = sp.diags(c["d"]) if c["d"] is not None else sp.identity(c["A"].shape[0])
        want = c["alpha"] * (D @ c["A"] @ c["B"])
        if c["E"] is not None:
            want = want + c["beta"] * c["E"]
        diff = abs(C - want)
        if family == "exact":
            assert diff.max() == 0 if diff.nnz else True
        else:
            slack = sp.csr_matrix((bound, C.indices, C.indptr), shape=C.shape) * 4.0 - diff
            assert slack.nnz == 0 or slack.data.min() >= 0.0
            assert np.all(bound >= 0.0) and (len(bound) == 0 or bound.max() < 1e-10)


def test_an_exact_case_keeps_an_entry_that_cancels_to_zero():
    C, _ = reference("tier1_row_2048", "exact")
    assert np.any(C.data == 0.0)
    assert not np.any(np.signbit(C.data[C.data == 0.0]))


@pytest.mark.parametrize("name", sorted(TRANSPOSES))
def test_transpose_cases(name):
    P = TRANSPOSES[name]
    assert sc.rows_have_distinct_columns(P)
    R = sc.reference_transpose(P)
    assert R.shape == P.shape[::-1] and sc.rows_are_sorted(R)
    assert abs(R - P.T).max() == 0 if P.nnz else R.nnz == 0
    if name.startswith("column_lengths"):
        lens = np.diff(R.indptr)
        assert tuple(lens) == sc.TRANSPOSE_LENGTHS
        assert {0, 1, 2, 64, sc.SORT_LDS - 1, sc.SORT_LDS, sc.SORT_LDS + 1, 5000} <= set(lens)
        assert lens[0] == 0 and lens[-1] == 0 and lens[5] == 0
    if "unsorted" in name:
        assert not sc.rows_are_sorted(P)
    assert {"no_entries", "no_columns"} <= set(TRANSPOSES)
    assert TRANSPOSES["no_entries"].nnz == 0 and TRANSPOSES["no_columns"].shape[1] == 0


def test_threshold_cases():
    A, tol = THRESHOLDS["chunks"]
    lens = np.diff(A.indptr)
    assert tuple(lens[:7]) == sc.THRESHOLD_LENGTHS == (0, 1, sc.CHUNK - 1, sc.CHUNK, sc.CHUNK + 1, 2 * sc.CHUNK, 200)
    assert A.shape[0] % 4 != 0 and not sc.rows_are_sorted(A)
    assert np.sum(A.data == tol) > 20 and np.sum(A.data == -tol) > 20
    C = sc.reference_threshold(A, tol)
    kept = np.diff(C.indptr)
    assert kept[7] == 0 and lens[7] > sc.CHUNK                            # a row that loses everything
    assert kept[8] == lens[8] > 2 * sc.CHUNK                              # a row that loses nothing
    assert kept[9] == 22                                                   # +tol and -tol go, the ones stay
    assert not np.any(np.abs(C.data) == tol)
    Z, zero = THRESHOLDS["tol_zero_explicit_zeros"]
    assert zero == 0.0 and np.sum(Z.data == 0.0) > 100 and np.any(np.signbit(Z.data) & (Z.data == 0.0))
    assert sc.reference_threshold(Z, zero).nnz == np.sum(Z.data != 0.0)
    assert sc.reference_threshold(*THRESHOLDS["everything_dropped"]).nnz == 0
    assert sc.reference_threshold(*THRESHOLDS["nothing_dropped_negative_tol"]).nnz == Z.nnz
    for name, (M, t) in THRESHOLDS.items():
        assert sc.rows_have_distinct_columns(M), name
        # order kept: the reference is the input with the dropped entries taken out
        keep = np.abs(M.data) > t
        R = sc.reference_threshold(M, t)
        assert np.array_equal(R.indices, M.indices[keep]) and np.array_equal(R.data.view(np.int64), M.data[keep].view(np.int64))
