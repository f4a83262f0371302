"""The assembled operator through the C++ layer: saamge_amd::api::AssembledOperator links the library, refuses bad arguments
without a GPU and, on the GPU, gives the model's operator, update and right-hand side bit for bit."""
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
    exe = str(tmp_path / "operator_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC, os.path.join(ROOT, "tests", "cxx", "operator_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_api_mirror_links_and_refuses_bad_arguments(tmp_path):
    assert "operator api test ok" in _run([_build_api_test(tmp_path)])


def _matrices(NE, step):
    a, b = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    K = np.where(a == b, 8.0, -1.0 - 0.125 * ((a ^ b) & 3))
    return K[None, :, :] * (1.0 + step * np.arange(NE))[:, None, None]


@pytest.mark.gpu
def test_api_mirror_gives_the_model_operator(tmp_path):
    from saamge_amd import assemble_model as am
    out = _run([_build_api_test(tmp_path), "gpu"])
    nx, ny, nz = 3, 2, 2
    vx, vy, vz = nx + 1, ny + 1, nz + 1
    NE, n = nx * ny * nz, vx * vy * vz
    e2d = np.array([((z + (c >> 2)) * vy + y + ((c >> 1) & 1)) * vx + x + (c & 1)
                    for z in range(nz) for y in range(ny) for x in range(nx) for c in range(8)], np.int32).reshape(NE, 8)
    bdr = np.where(np.arange(n) % vx == 0, 0x0A, 0x08).astype(np.int8)
    lines = {" ".join(l.split()[:2]): l.split()[2:] for l in out.splitlines() if l.split()[0] in ("first", "second")}
    for tag, step in (("first", 0.0625), ("second", 0.3)):
        rowptr, col, val = am.assemble(n, None, e2d, _matrices(NE, step), bdr)
        assert np.array_equal(np.array(lines[tag + " rowptr"], np.int64), rowptr)
        assert np.array_equal(np.array(lines[tag + " col"], np.int32), col)
        assert np.array_equal(np.array([float.fromhex(v) for v in lines[tag + " val"]]), val)
    x = 0.25 + 0.0625 * np.arange(n)
    b = 1.0 - 0.03125 * np.arange(n)
    want = am.eliminate_rhs(n, None, e2d, _matrices(NE, 0.0625), bdr, x, b)
    got = [l.split()[1:] for l in out.splitlines() if l.startswith("rhs ")][0]
    assert np.array_equal(np.array([float.fromhex(v) for v in got]), want)
