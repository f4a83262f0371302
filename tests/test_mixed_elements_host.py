"""CPU tests (no GPU) of the mixed hex / wedge inputs: the generator's element matrices and operator, and the oracle's
hierarchy on such a mesh (the composition the GPU tests in test_gpu_mixed_elements.py rely on)."""
import os
import re

import numpy as np
import pytest

from oracle import saamge_oracle as o
from saamge_amd import problems as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _elements(prob):
    """(dofs, matrix) per element, in element order."""
    out = []
    off = 0
    for e in range(prob.NE):
        a, b = int(prob.elem_ptr[e]), int(prob.elem_ptr[e + 1])
        nd = b - a
        out.append((prob.elem_to_dof[a:b], prob.elmat[off:off + nd * nd].reshape(nd, nd)))
        off += nd * nd
    assert off == prob.elmat.size
    return out


def _mixed_oracle(monkeypatch, prob, ncoars, **kw):
    """The oracle on a mesh of elements of different sizes: every building block takes a variable Table; only
    ml_produce_data turns its input into one with Table.from_fixed, which here passes a Table through."""
    orig = o.Table.from_fixed
    monkeypatch.setattr(o.Table, "from_fixed",
                        staticmethod(lambda arr, ncols: arr if isinstance(arr, o.Table) else orig(arr, ncols)))
    e2d = o.Table(prob.elem_ptr, prob.elem_to_dof, prob.ND)
    elmats = [K for (_, K) in _elements(prob)]
    return o.ml_produce_data(prob.A, e2d, elmats, prob.bdr, prob.partitions[:ncoars], **kw)


@pytest.mark.parametrize("wedges,coef", [("half", None), ("all", "skew"), ("random", "checkerboard")])
def test_generator_operator_is_sum_of_element_matrices(wedges, coef):
    prob = pr.poisson3d_mixed_problem((5, 4, 3), (2, 2, 3), wedges=wedges, coef=coef, seed=1)
    nd = np.diff(prob.elem_ptr)
    assert prob.NE == len(nd) and set(np.unique(nd)) <= {6, 8}
    if wedges != "random":
        assert (nd == 6).any() and (wedges == "all") == (nd == 6).all()
    assert len(prob.partitions[0]) == prob.NE
    A0 = np.zeros((prob.ND, prob.ND))
    for d, K in _elements(prob):
        A0[np.ix_(d, d)] += K
    # the generator's A is A0 with the essential rows / columns zeroed, diagonal kept
    keep = ~prob.ess
    A = prob.A.toarray()
    assert np.allclose(A[np.ix_(keep, keep)], A0[np.ix_(keep, keep)], rtol=1e-14, atol=1e-14 * np.abs(A0).max())
    assert np.allclose(np.diag(A), np.diag(A0), rtol=1e-14)
    # a split cell's two wedges share its agglomerate
    w = np.flatnonzero(nd == 6)
    pairs = w[::2]
    assert np.array_equal(w[1::2], pairs + 1)
    assert np.array_equal(prob.partitions[0][pairs], prob.partitions[0][pairs + 1])


def test_element_matrices_spsd_with_constant_null_space():
    prob = pr.poisson3d_mixed_problem((4, 4, 2), (2, 2, 2), wedges="random", coef="skew", seed=2)
    for d, K in _elements(prob):
        assert np.allclose(K, K.T, rtol=0, atol=1e-15 * np.abs(K).max())
        assert np.abs(K @ np.ones(len(d))).max() <= 1e-13 * np.abs(K).max()
        w = np.linalg.eigvalsh(K)
        assert w[0] >= -1e-13 * w[-1]
        assert w[1] > 1e-8 * w[-1]          # the constants only


def test_wedges_reproduce_linear_functions():
    """P1 wedges contain the linear functions: u = a.x gives u^T K_e u = |a|^2 V_e (coefficient 1), exactly."""
    n = (4, 4, 2)
    prob = pr.poisson3d_mixed_problem(n, (2, 2, 2), wedges="random", seed=5)
    nvx, nvy = n[0] + 1, n[1] + 1
    g = np.arange(prob.ND)
    X = np.stack([(g % nvx) / n[0], ((g // nvx) % nvy) / n[1], (g // (nvx * nvy)) / n[2]], axis=1)
    rng = np.random.default_rng(0)
    vol = 1.0 / np.prod(n)
    checked = 0
    for d, K in _elements(prob):
        V = vol / 2 if len(d) == 6 else vol
        for _ in range(3):
            a = rng.standard_normal(3)
            u = X[d] @ a
            assert abs(u @ K @ u - (a @ a) * V) <= 1e-12 * (a @ a) * V
        checked += len(d) == 6
    assert checked > 0


def test_oracle_builds_a_mixed_hierarchy(monkeypatch):
    prob = pr.poisson3d_mixed_problem((4, 4, 2), (2, 2, 2), wedges="half")
    H = _mixed_oracle(monkeypatch, prob, 1)
    rel = H.levels[0].rel
    assert rel.elem_to_dof.nrows == prob.NE and np.array_equal(rel.elem_to_dof.I, prob.elem_ptr)
    assert rel.nparts == 4
    # every element's dofs lie in its agglomerate
    for e in range(prob.NE):
        assert set(rel.elem_to_dof.row(e)) <= set(rel.AE_to_dof.row(prob.partitions[0][e]))
    x, it, conv, hist = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and it <= 10
    assert np.linalg.norm(prob.A @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)


def test_mixed_entries_declared():
    src = open(os.path.join(ROOT, "include", "saamge_amd.h")).read()
    for name in ("saamge_amd_ml_produce_data_mixed", "saamge_amd_ml_produce_data_mixed64"):
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        args = " ".join(m.group(1).split())
        assert "int NE, const int *elem_ptr, const int *elem_to_dof, const double *elmat" in args
