"""The element matrices with coefficients at the points through the C++ layer: saamge_amd::api::element_matrices_points_into
and element_mass_points_into link the library under -Wall -Wextra -Werror, refuse kind, ncoef, vdim and the NULL arguments without
a GPU and, on the GPU, give the model's doubles bit for bit on two sheared hexahedra with eight different coefficients each."""
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
    exe = str(tmp_path / "elmat_kq_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC, os.path.join(ROOT, "tests", "cxx", "elmat_kq_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_api_mirror_links_and_refuses_without_a_gpu(tmp_path):
    assert "elmat kq api test ok" in _run([_build_api_test(tmp_path)])


@pytest.mark.gpu
def test_api_mirror_gives_the_model_doubles(tmp_path):
    from saamge_amd import elmat_model as em
    out = _run([_build_api_test(tmp_path), "gpu"])
    nx, gx = 2, 3
    e2v = np.array([(lz * 2 + ly) * gx + e + lx for e in range(nx) for (lx, ly, lz) in em.HEX_LOC], np.int32).reshape(nx, 8)
    X = np.array([[0.25 * i + 0.03125 * j * k, 0.5 * j + 0.015625 * i * k, 0.5 * k + 0.0078125 * i * j]
                  for k in range(2) for j in range(2) for i in range(gx)])
    q = np.arange(8 * nx)
    kq = np.array([[1.0 + 0.0625 * p + 0.25 * d for d in range(3)] + [0.03125 * (p % 5) - 0.015625 * d for d in range(3)] for p in q])
    lm = np.stack([2.0 - 0.03125 * q, 0.5 + 0.0625 * q], axis=1)
    sigma = 1.0 + 0.125 * q
    K = em.element_matrices_points(X, e2v, 0, kq)
    want = {
        "diffusion": K, "elasticity": em.element_matrices_points(X, e2v, 1, lm),
        "mass": em.element_mass_points(X, e2v, sigma), "sum": em.element_mass_points(X, e2v, sigma, add_to=K),
    }
    lines = {l.split()[0]: np.array([float.fromhex(t) for t in l.split()[1:]]) for l in out.splitlines()
             if l.split() and l.split()[0] in want}
    for tag, w in want.items():
        assert np.array_equal(lines[tag], np.asarray(w).ravel()), tag
