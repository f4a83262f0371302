"""The kernel plan of the dense eigensolver (csrc/eig_dense_plan.h: which kernel, how many threads, which grid, how much LDS for
which batch) is plain host C++: tests/cxx/eig_dense_plan_test.cpp holds every threshold to its value, without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout
    return p.stdout


def test_plan_thresholds_hold_their_values(tmp_path):
    exe = str(tmp_path / "eig_dense_plan_test")
    _run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "saamge_amd", "csrc"),
          os.path.join(ROOT, "tests", "cxx", "eig_dense_plan_test.cpp"), "-o", exe])
    assert "eig_dense plan test ok" in _run([exe])
