"""The uniform refinement through the C++ layer: saamge_amd::api::MeshRefine links the library under -Wall -Wextra -Werror,
refuses levels = 0, levels above the cap, dim = 4, a NULL vertex list and a node count that is no type without a GPU, leaving the
handle argument untouched, and on the GPU gives the model's integers, coordinate bits and interpolations on a sheared two-hex
mesh refined twice."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout
    return p.stdout


def _build_api_test(tmp_path):
    lib_dir = os.path.join(ROOT, "saamge_amd")
    assert os.path.exists(os.path.join(lib_dir, "libsaamge_amd.so")), "run __graft_entry__.build() first"
    exe = str(tmp_path / "mesh_refine_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC, os.path.join(ROOT, "tests", "cxx", "mesh_refine_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_api_mirror_links_and_refuses_without_a_gpu(tmp_path):
    assert "mesh refine api test ok" in _run([_build_api_test(tmp_path)])


@pytest.mark.gpu
def test_api_mirror_gives_the_model_integers_and_bits(tmp_path):
    from saamge_amd import elmat_model as em
    from saamge_amd import mesh_refine_model as rm
    out = _run([_build_api_test(tmp_path), "gpu"])
    assert "mesh refine api test ok" in out
    nx, gx = 2, 3
    NV = gx * 4
    e2v = np.array([(lz * 2 + ly) * gx + e + lx for e in range(nx) for (lx, ly, lz) in em.HEX_LOC], np.int32).reshape(nx, 8)
    k = np.arange(NV)
    i, j, l = k % gx, (k // gx) % 2, k // (2 * gx)
    X = np.stack([i / 3.0 + 0.1 * j, j / 7.0 + 0.1 * l, l / 11.0 + 0.1 * i], axis=1)
    R = rm.MeshRefine(NV, 3, X, e2v, levels=2, want_interp=True)
    want = dict(zip(("coords", "elem_ptr", "elem_to_vertex"), R.arrays()))
    want["coords"] = want["coords"].view(np.int64)
    for lv in range(2):
        want.update({"rowptr%d" % lv: R.P[lv].rowptr, "col%d" % lv: R.P[lv].col, "val%d" % lv: R.P[lv].val.view(np.int64)})
    lines = {t.split()[0]: np.array([int(w) for w in t.split()[1:]], np.int64) for t in out.splitlines()
             if t.split() and t.split()[0] in want}
    for tag, w in want.items():
        assert np.array_equal(lines[tag], np.asarray(w).ravel()), tag
