"""The general sparse products, the transpose and the threshold of csrc/spgemm.hip through their own entry points
(saamge_amd_spgemm, saamge_amd_csr_transpose, saamge_amd_csr_threshold), on the cases of tests/spgemm_cases.py: every table
tier of the hash product on both sides of its limit, the refusal beyond the last one, the dense-B product and its ineligible
twins, both sort paths of the transpose, threshold rows of several chunks.  The pattern must be the structural one, every row
sorted, the values bitwise those of an exact reference (integer family) or within the entrywise bound derived from the kernel's
arithmetic of a long double reference (general family); the reported route must be the one the case is written for, and a second
call must return the same bits (spgemm.hip promises run-to-run reproducibility).  tests/test_spgemm_cases.py proves on the CPU
that the cases have the properties they are named for."""
import functools

import numpy as np
import pytest

import spgemm_cases as sc

pytestmark = pytest.mark.gpu

PRODUCTS = sorted(n for n in sc.PATTERNS if sc.PATTERNS[n]["expect"] != sc.ROUTE_REFUSED)
DENSE = sorted(n for n in sc.PATTERNS if sc.PATTERNS[n]["expect"] == sc.ROUTE_DENSE)
TRANSPOSES = sc.transpose_cases()
THRESHOLDS = sc.threshold_cases()


@functools.lru_cache(maxsize=None)
def case(name, family):
    return sc.product_case(name, family)


@functools.lru_cache(maxsize=None)
def reference(name, family):
    c = case(name, family)
    return sc.reference_product(c["A"], c["B"], extended=family == "general", **sc.operands(c))


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def same_arrays(X, Y):
    return (X.shape == Y.shape and np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)
            and np.array_equal(bits(X.data), bits(Y.data)))


def check_values(got, want, bound, family, what):
    if family == "exact":
        bad = np.nonzero(bits(got) != bits(want))[0]
        assert bad.size == 0, "%s: %d of %d values differ, first at %d: %r != %r" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])
    else:
        err = np.abs(got - want)
        worst = float((err / np.where(bound > 0, bound, 1.0)).max()) if err.size else 0.0
        print("%s: largest error / bound = %.3f over %d entries" % (what, worst, err.size))
        assert np.all(err <= bound), "%s: error %.3e beyond its bound %.3e (%.2f times)" % (
            what, err[np.argmax(err - bound)], bound[np.argmax(err - bound)], worst)


def sub_block(C, rows, ncols, extra=None):
    """(indptr, indices, data[, extra]) of the given rows of C restricted to the columns below ncols"""
    r = np.repeat(np.arange(C.shape[0]), np.diff(C.indptr))
    keep = np.isin(r, rows) & (C.indices < ncols)
    out = (np.bincount(r[keep], minlength=C.shape[0])[rows], C.indices[keep], C.data[keep])
    return out + ((extra[keep],) if extra is not None else ())


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("name", PRODUCTS)
def test_product_matches_the_reference_on_its_route(name, family):
    from saamge_amd import capi
    c = case(name, family)
    want, bound = reference(name, family)
    C, route = capi.spgemm(c["A"], c["B"], **sc.operands(c))
    assert route == c["expect"], "route %r, the case is written for %r" % (route, c["expect"])
    assert C.shape == want.shape
    assert np.array_equal(C.indptr, want.indptr)
    assert np.array_equal(C.indices, want.indices)                     # (the reference's rows are sorted)
    assert sc.rows_are_sorted(C)
    check_values(C.data, want.data, bound, family, name)
    if "twin_of" in c:       # where the change from the eligible case does not reach, the other route gives that case's product
        base_want, base_bound = reference(c["twin_of"], family)
        rows, nc = c["same_rows"], c["same_cols"]
        g, w = sub_block(C, rows, nc), sub_block(base_want, rows, base_want.shape[1], base_bound)
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])
        check_values(g[2], w[2], w[3], family, name + " against " + c["twin_of"])
    C2, route2 = capi.spgemm(c["A"], c["B"], **sc.operands(c))
    assert route2 == route and same_arrays(C, C2), "a second call gives other bits"


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("name", DENSE)
def test_dense_and_hash_routes_agree_bit_for_bit(name, family):
    """d = 1 changes no value (alpha d A_ik = A_ik exactly) and makes the product ineligible for the dense-B route: the same
    fused multiply-adds in the same order on the other route."""
    from saamge_amd import capi
    c = case(name, family)
    Cd, route_d = capi.spgemm(c["A"], c["B"])
    Ch, route_h = capi.spgemm(c["A"], c["B"], d=np.ones(c["A"].shape[0]))
    assert route_d == sc.ROUTE_DENSE and route_h in (0, 1, 2)
    assert route_h == sc.model_route(c["A"], c["B"], d=np.ones(1))
    assert same_arrays(Cd, Ch)


def test_row_beyond_the_last_table_is_refused_and_the_library_goes_on():
    from saamge_amd import capi
    c = case("refused_row_8193", "exact")
    assert c["expect"] == sc.ROUTE_REFUSED
    with pytest.raises(RuntimeError, match="a product row has more than ~8000 entries"):
        capi.spgemm(c["A"], c["B"])
    small = case("tier0_row_256", "exact")
    C, route = capi.spgemm(small["A"], small["B"])
    want, _ = reference("tier0_row_256", "exact")
    assert route == 0 and same_arrays(C, want)


def test_entry_point_refuses_malformed_arrays():
    """(the kernels trust offsets and column indices; the entry point checks them on the host)"""
    from saamge_amd import capi
    c = case("tier0_row_256", "exact")
    bad = c["B"].copy()
    bad.indices[3] = bad.shape[1]
    with pytest.raises(RuntimeError, match="column index out of range"):
        capi.spgemm(c["A"], bad)
    bad = c["A"].copy()
    bad.indptr[2] = bad.indptr[1] - 1
    with pytest.raises(RuntimeError, match="row offsets must ascend"):
        capi.spgemm(bad, c["B"])


@pytest.mark.parametrize("name", sorted(TRANSPOSES))
def test_transpose(name):
    from saamge_amd import capi
    P = TRANSPOSES[name]
    want = sc.reference_transpose(P)
    R = capi.csr_transpose(P)
    assert sc.rows_are_sorted(R)
    assert same_arrays(R, want)                         # the values move bit for bit
    assert same_arrays(capi.csr_transpose(P), R)
    assert same_arrays(capi.csr_transpose(R), sc.sorted_rows(P))


@pytest.mark.parametrize("name", sorted(THRESHOLDS))
def test_threshold(name):
    from saamge_amd import capi
    A, tol = THRESHOLDS[name]
    want = sc.reference_threshold(A, tol)               # the numpy mask abs(v) > tol row by row, the input order kept
    C = capi.csr_threshold(A, tol)
    assert same_arrays(C, want)
    assert same_arrays(capi.csr_threshold(A, tol), C)
