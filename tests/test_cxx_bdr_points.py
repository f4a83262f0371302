"""The boundary data at the face points through the C++ layer: saamge_amd::api::boundary_points_into, boundary_eval_into,
boundary_mass_points_into and boundary_loads_points_into link the library under -Wall -Wextra -Werror, refuse vdim = 2 in 3D, NULL
data, NULL lists and NF < 0 without a GPU and, on the GPU, give the model's doubles bit for bit on a two-hex mesh with three
listed faces."""
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
    exe = str(tmp_path / "bdr_points_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC, os.path.join(ROOT, "tests", "cxx", "bdr_points_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_api_mirror_links_and_refuses_wrong_arguments(tmp_path):
    assert "bdr points api test ok" in _run([_build_api_test(tmp_path)])


@pytest.mark.gpu
def test_api_mirror_gives_the_model_doubles(tmp_path):
    from saamge_amd import elmat_model as em
    out = _run([_build_api_test(tmp_path), "gpu"])
    nx, gx = 2, 3
    e2v = np.array([(lz * 2 + ly) * gx + e + lx for e in range(nx) for (lx, ly, lz) in em.HEX_LOC], np.int32).reshape(nx, 8)
    X = np.array([[0.25 * i + 0.03125 * j * k, 0.5 * j + 0.015625 * i * k, 0.5 * k + 0.0078125 * i * j]
                  for k in range(2) for j in range(2) for i in range(gx)])
    u3 = np.array([[0.5 * d + 0.125 * i * j - 0.0625 * k + 0.25 * i * k for d in range(3)] for k in range(2) for j in range(2)
                   for i in range(gx)])
    fe, fl = [0, 1, 0], [4, 2, 0]
    fp, xq, wmeas, normal = em.boundary_points(X, e2v, fe, fl)
    uq, gradq = em.boundary_eval(X, e2v, fe, fl, u3, vdim=3)
    want = {
        "xq": xq, "wmeas": wmeas, "normal": normal, "uq": uq, "gradq": gradq,
        "mass_points": em.boundary_mass_points(X, e2v, fe, fl, 1.0 + 0.0625 * np.arange(12), add_to=np.zeros((nx, 8, 8))),
        "loads_points": em.boundary_loads_points(X, e2v, fe, fl, uq, vdim=3, add_to=np.zeros((nx, 24))),
    }
    assert fp.tolist() == [0, 4, 8, 12]
    lines = {l.split()[0]: np.array([float.fromhex(t) for t in l.split()[1:]]) for l in out.splitlines()
             if l.split() and l.split()[0] in want}
    for tag, w in want.items():
        assert np.array_equal(lines[tag], np.asarray(w).ravel()), tag
