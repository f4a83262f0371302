"""The element matrices through the C++ layer: saamge_amd::api::element_matrices links the library, refuses bad arguments
without a GPU and, on the GPU, gives the model's matrices bit for bit."""
import ctypes as C
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
    exe = str(tmp_path / "elmat_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC, os.path.join(ROOT, "tests", "cxx", "elmat_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_api_mirror_links_and_refuses_bad_arguments(tmp_path):
    assert "elmat api test ok" in _run([_build_api_test(tmp_path)])


def test_c_entry_refuses_bad_arguments_before_any_device_work():
    from saamge_amd import capi
    lib = capi.load()
    x, v, c = np.zeros((8, 3)), np.arange(8, dtype=np.int32), np.ones(1)

    def call(NV, dim, coords, NE, nde, lists, kind, ncoef, coef):
        info = (C.c_longlong * 8)()
        rc = lib.saamge_amd_element_matrices(C.c_int(NV), C.c_int(dim), capi._ptr(coords), C.c_int(NE), C.c_int(nde), None,
                                             capi._ptr(lists), C.c_int(kind), C.c_int(ncoef), capi._ptr(coef), None, None, None,
                                             None, info)
        return rc, lib.saamge_amd_last_error().decode(), list(info)
    for args, match in (((8, 4, x, 1, 8, v, 0, 1, c), "dim"), ((8, 3, x, 1, 8, v, 2, 1, c), "kind"),
                        ((8, 3, x, 1, 8, v, 0, 2, c), "ncoef"), ((8, 3, None, 1, 8, v, 0, 1, c), "null argument"),
                        ((8, 3, x, 1, 8, None, 0, 1, c), "null argument"), ((8, 3, x, 1, 8, v, 0, 1, None), "null argument"),
                        ((8, 3, x, 1, 5, v, 0, 1, c), "nde = 5"), ((8, 3, x, -1, 8, v, 0, 1, c), "NE < 0")):
        rc, err, info = call(*args)
        assert rc != 0 and match in err and err.count("saamge_amd_element_matrices"), (args, rc, err)
        assert info[6] == -1 and info[5] == 0
    with pytest.raises(RuntimeError, match="ncoef") as e:
        capi.element_matrices(x, v.reshape(1, 8), 0, np.ones((1, 2)))
    assert e.value.info[6] == -1


@pytest.mark.gpu
def test_api_mirror_gives_the_model_matrices(tmp_path):
    from saamge_amd import elmat_model as em
    out = _run([_build_api_test(tmp_path), "gpu"])
    nx, ny, nz = 3, 2, 2
    vx, vy, vz = nx + 1, ny + 1, nz + 1
    NE = nx * ny * nz
    loc = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
    e2v = np.array([((z + c) * vy + y + b) * vx + x + a for z in range(nz) for y in range(ny) for x in range(nx)
                    for (a, b, c) in loc], np.int32).reshape(NE, 8)
    X = np.array([[0.25 * i + 0.03125 * j * k, 0.5 * j + 0.015625 * i * k, 0.5 * k + 0.0078125 * i * j]
                  for k in range(vz) for j in range(vy) for i in range(vx)])
    e = np.arange(NE)
    k6 = np.stack([1.0 + 0.0625 * e, np.full(NE, 1.5), 2.0 - 0.03125 * e, np.full(NE, 0.125), np.full(NE, -0.0625),
                   np.full(NE, 0.25)], axis=1)
    lm = np.stack([1.0 + 0.125 * e, 0.5 + 0.0625 * e], axis=1)
    lines = {l.split()[0]: l.split()[1:] for l in out.splitlines() if l.split()[0] in ("diffusion", "elasticity", "dofs")}
    for tag, kind, coef in (("diffusion", 0, k6), ("elasticity", 1, lm)):
        want = em.element_matrices(X, e2v, kind, coef)
        assert np.array_equal(np.array([float.fromhex(t) for t in lines[tag]]), want.ravel())
    assert np.array_equal(np.array(lines["dofs"], np.int32), em.dof_lists(3, e2v, 1)[1])
