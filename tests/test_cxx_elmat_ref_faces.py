"""The tables of the face points (csrc/elmat_ref.h: ref_node, FaceGradTable, face_points, with_face_nodes) are plain host C++:
tests/cxx/elmat_ref_faces_test.cpp prints, per element type and local face, the reference position of every face point in the
element and the gradients of all the element's nodes there as hexadecimal doubles, and this test holds each value's bits to
saamge_amd/elmat_model.py (REF_NODES, face_ref_point, face_gradients), without a GPU.  bdr_eval_kernel reads these tables; the GPU
tests hold what it computes from them."""
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
    """{"face_points": {(dim, fn): n}, "ref_node": {(dim, nd, a, k): bits},
    (dim, nd, lf): {"fn": n, "nq": n, ("node", c): id, ("xi", q, k): bits, ("dN", q, a, k): bits}}"""
    exe = str(tmp_path_factory.mktemp("elmat_ref_faces") / "elmat_ref_faces_test")
    _run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "saamge_amd", "csrc"),
          os.path.join(ROOT, "tests", "cxx", "elmat_ref_faces_test.cpp"), "-o", exe])
    out = _run([exe])
    assert "elmat_ref faces test ok" in out and "bad fork" not in out
    rec = {"face_points": {}, "ref_node": {}}
    for line in out.splitlines():
        w = line.split()
        if w[0] == "face_points":
            rec["face_points"][(int(w[1]), int(w[2]))] = int(w[3])
        elif w[0] == "ref_node":
            key = tuple(int(x) for x in w[1:5])
            assert key not in rec["ref_node"], line
            rec["ref_node"][key] = _bits(float.fromhex(w[5]))
        elif w[0] == "facegrad":
            t = rec.setdefault(tuple(int(x) for x in w[1:4]), {})
            if w[4] in ("fn", "nq"):
                key, value = w[4], int(w[5])
            elif w[4] == "node":
                key, value = ("node", int(w[5])), int(w[6])
            else:
                key, value = (w[4],) + tuple(int(x) for x in w[5:-1]), _bits(float.fromhex(w[-1]))
            assert key not in t, line
            t[key] = value
    return rec


def test_point_counts_and_reference_nodes_are_the_models(printed):
    assert printed["face_points"] == model.FACE_NPOINTS and len(model.FACE_NPOINTS) == 6
    want = {(dim, nd, a, k): _bits(model.REF_NODES[(dim, nd)][a][k]) for (dim, nd) in model.ALL_TYPE_INDEX for a in range(nd)
            for k in range(dim)}
    assert printed["ref_node"] == want


def test_no_face_is_left_out(printed):
    faces = {k for k in printed if isinstance(k, tuple)}
    assert faces == {(dim, nd, lf) for (dim, nd), f in model.FACE_NODES.items() for lf in range(len(f))}
    assert len(faces) == 3 + 4 + 4 + 5 + 6 + 4 + 6 + 3 + 4


@pytest.mark.parametrize("dim,nd", sorted(model.ALL_TYPE_INDEX))
def test_face_gradient_tables_have_the_models_bits(printed, dim, nd):
    values = 0
    for lf, nodes in enumerate(model.FACE_NODES[(dim, nd)]):
        got = printed[(dim, nd, lf)]
        nq = model.FACE_NPOINTS[(dim, len(nodes))]
        want = {"fn": len(nodes), "nq": nq}
        for c, node in enumerate(nodes):
            want[("node", c)] = node
        for q in range(nq):
            xi, dN = model.face_ref_point(dim, nd, lf, q), model.face_gradients(dim, nd, lf, q)
            assert len(xi) == dim and len(dN) == nd and all(len(d) == dim for d in dN)
            for k in range(dim):
                want[("xi", q, k)] = _bits(xi[k])
                for a in range(nd):
                    want[("dN", q, a, k)] = _bits(dN[a][k])
        assert set(got) == set(want), (dim, nd, lf)
        wrong = [k for k in want if got[k] != want[k]]
        assert not wrong, "face %d of (%d, %d): %d of %d values differ, the first at %s" % (lf, dim, nd, len(wrong), len(want), wrong[0])
        values += nq * nd * dim
    assert values == sum(model.FACE_NPOINTS[(dim, len(n))] for n in model.FACE_NODES[(dim, nd)]) * nd * dim
