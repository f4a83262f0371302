"""The eigensolver through the C++ layer: saamge_amd::api::lobpcg links the library and refuses bad arguments without a GPU
and, on the GPU, solves cube8 for four pairs, which are held to the bounds of tests/lobpcg_cases.py here."""
import os
import subprocess

import numpy as np
import pytest

import lobpcg_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout
    return p.stdout


def _build_api_test(tmp_path):
    lib_dir = os.path.join(ROOT, "saamge_amd")
    assert os.path.exists(os.path.join(lib_dir, "libsaamge_amd.so")), "run __graft_entry__.build() first"
    exe = str(tmp_path / "lobpcg_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC, os.path.join(ROOT, "tests", "cxx", "lobpcg_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_api_mirror_links_and_refuses_bad_arguments(tmp_path):
    assert "lobpcg api test ok" in _run([_build_api_test(tmp_path)])


@pytest.mark.gpu
def test_api_mirror_finds_the_lowest_pairs_of_cube8(tmp_path):
    name, nev = "cube8", 4
    p = lc.problem(name)
    A = p.A.tocsr()
    n, NE, nde = A.shape[0], p.elem_to_dof.shape[0], p.elem_to_dof.shape[1]
    part = np.asarray(p.partitions[0], dtype=np.int32)
    x0 = lc.start_block(name, nev)
    problem, out = str(tmp_path / "cube8.bin"), str(tmp_path / "pairs.bin")
    with open(problem, "wb") as f:
        for a, dt in ((np.array([n, A.nnz, NE, nde, int(part.max()) + 1]), np.int32), (A.indptr, np.int32), (A.indices, np.int32),
                      (A.data, np.float64), (p.elem_to_dof, np.int32), (p.elmat, np.float64), (p.bdr, np.int8), (part, np.int32),
                      (x0.T, np.float64)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    text = _run([_build_api_test(tmp_path), "gpu", problem, out])
    assert "lobpcg api test ok" in text
    got = np.fromfile(out, dtype=np.float64)
    lam, res, X = got[:nev], got[nev:2 * nev], got[2 * nev:].reshape(nev, n).T
    assert np.all(res <= lc.TOL)
    lc.check_pairs(lc.reference(name, None, True), lam, X)
