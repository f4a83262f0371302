"""The reference elements of the element layer (csrc/elmat_ref.h: shape functions, rules, tables, the dispatch over the types)
are plain host C++: tests/cxx/elmat_ref_test.cpp prints every table as hexadecimal doubles and this test holds each value's bits
to saamge_amd/elmat_model.py, without a GPU.  The kernels read these tables; the GPU tests hold what they compute from them."""
import os
import struct
import subprocess

import pytest

from saamge_amd import elmat_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout
    return p.stdout


def _bits(x):
    return struct.pack("<d", float(x))


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """{"types": {index: (dim, nd)}, "face_types": ..., "mass_points": {(dim, nd): n},
    (table, dim, nd): {"nq": n, ("w", q): bits, ("dN", q, a, j): bits, ("N", q, a): bits}}"""
    exe = str(tmp_path_factory.mktemp("elmat_ref") / "elmat_ref_test")
    _run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "saamge_amd", "csrc"),
          os.path.join(ROOT, "tests", "cxx", "elmat_ref_test.cpp"), "-o", exe])
    out = _run([exe])
    assert "elmat_ref test ok" in out
    rec = {"types": {}, "face_types": {}, "mass_points": {}}
    for line in out.splitlines():
        w = line.split()
        if w[0] in ("type", "face_type"):
            assert int(w[1]) not in rec[w[0] + "s"]
            rec[w[0] + "s"][int(w[1])] = (int(w[2]), int(w[3]))
        elif w[0] == "mass_points":
            rec["mass_points"][(int(w[1]), int(w[2]))] = int(w[3])
        elif w[0] in ("stiff", "mass", "face"):
            t = rec.setdefault((w[0], int(w[1]), int(w[2])), {})
            key = "nq" if w[3] == "nq" else (w[3],) + tuple(int(x) for x in w[4:-1])
            assert key not in t, line
            t[key] = int(w[4]) if w[3] == "nq" else _bits(float.fromhex(w[-1]))
    return rec


def _expect(nq, weight, gradients, values, nd, axes):
    """the table the model defines: the same keys as a printed one"""
    t = {"nq": nq}
    for q in range(nq):
        t[("w", q)] = _bits(weight(q))
        dN = gradients(q)
        N = values(q) if values else None
        assert len(dN) == nd and all(len(d) == axes for d in dN)
        for a in range(nd):
            for j in range(axes):
                t[("dN", q, a, j)] = _bits(dN[a][j])
            if values:
                t[("N", q, a)] = _bits(N[a])
    return t


def _same(got, want, what):
    assert set(got) == set(want), what
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, "%s: %d of %d values differ, the first at %s" % (what, len(wrong), len(want), wrong[0])
    return len(want) - 1


def test_dispatch_list_is_the_models_type_index(printed):
    assert printed["types"] == {t: k for k, t in model.ALL_TYPE_INDEX.items()} and len(printed["types"]) == 9
    assert printed["face_types"] == {t: k for k, t in model.FACE_TYPE_INDEX.items()} and len(printed["face_types"]) == 6


def test_point_counts_are_the_models(printed):
    assert printed["mass_points"] == {k: model.MASS_NPOINTS[k] for k in model.ALL_TYPE_INDEX}
    for (dim, nd) in model.ALL_TYPE_INDEX:
        assert printed[("stiff", dim, nd)]["nq"] == model.NPOINTS[(dim, nd)]
        assert printed[("mass", dim, nd)]["nq"] == model.MASS_NPOINTS[(dim, nd)]
    for (dim, fn) in model.FACE_TYPE_INDEX:
        assert printed[("face", dim, fn)]["nq"] == len(model.face_rule(dim, fn))


@pytest.mark.parametrize("dim,nd", sorted(model.ALL_TYPE_INDEX))
def test_stiffness_tables_have_the_models_bits(printed, dim, nd):
    want = _expect(model.NPOINTS[(dim, nd)], lambda q: model.point_weight(dim, nd, q),
                   lambda q: model.reference_gradients(dim, nd, q), None, nd, dim)
    _same(printed[("stiff", dim, nd)], want, "stiffness rule of (%d, %d)" % (dim, nd))


@pytest.mark.parametrize("dim,nd", sorted(model.ALL_TYPE_INDEX))
def test_mass_tables_have_the_models_bits(printed, dim, nd):
    want = _expect(model.MASS_NPOINTS[(dim, nd)], lambda q: model.mass_point_weight(dim, nd, q),
                   lambda q: model.mass_reference_gradients(dim, nd, q), lambda q: model.shape_values(dim, nd, q), nd, dim)
    _same(printed[("mass", dim, nd)], want, "mass rule of (%d, %d)" % (dim, nd))


@pytest.mark.parametrize("dim,fn", sorted(model.FACE_TYPE_INDEX))
def test_face_tables_have_the_models_bits(printed, dim, fn):
    rule = model.face_rule(dim, fn)
    want = _expect(len(rule), lambda q: rule[q][2], lambda q: rule[q][1], lambda q: rule[q][0], fn, dim - 1)
    _same(printed[("face", dim, fn)], want, "rule of the face (%d, %d)" % (dim, fn))


def test_no_table_is_left_out(printed):
    tables = {k for k in printed if isinstance(k, tuple)}
    assert tables == {(t, d, n) for t in ("stiff", "mass") for (d, n) in model.ALL_TYPE_INDEX} | \
        {("face", d, n) for (d, n) in model.FACE_TYPE_INDEX}
