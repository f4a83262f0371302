"""The small dense half of the eigensolver (csrc/lobpcg_host.h: Cholesky with a reported pivot, triangular solves, the
symmetric generalised eigenproblem of order <= 48, the assembly of the coefficients) is plain host C++:
tests/cxx/lobpcg_host_test.cpp holds it to eigenvalues written out by numpy, without a GPU and under the address and
undefined-behaviour sanitizers.  The device driver calls the same functions."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout
    return p.stdout


def test_the_dense_half_factors_solves_and_finds_the_eigenvalues_numpy_wrote_out(tmp_path):
    exe = str(tmp_path / "lobpcg_host_test")
    _run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
          os.path.join(ROOT, "saamge_amd", "csrc"), os.path.join(ROOT, "tests", "cxx", "lobpcg_host_test.cpp"), "-o", exe])
    assert "lobpcg host test ok" in _run([exe])
