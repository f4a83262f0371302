"""The order-2 simplices through the C++ layer: saamge_amd::api links the library; 6 nodes in 2D and 10 in 3D pass the size checks
of the five element-layer calls and other node counts are refused, without a GPU; on the GPU one 6-node triangle and one 10-node
tetrahedron give the closed forms of their stiffness, mass, loads and face mass, and a face index of 4 on a tetrahedron is
refused."""
import os
import subprocess

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
    exe = str(tmp_path / "elmat_p2_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC, os.path.join(ROOT, "tests", "cxx", "elmat_p2_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_api_mirror_links_accepts_the_two_node_counts_and_refuses_others(tmp_path):
    assert "elmat p2 api test ok" in _run([_build_api_test(tmp_path)])


@pytest.mark.gpu
def test_api_mirror_gives_the_closed_forms_of_one_triangle_and_one_tetrahedron(tmp_path):
    out = _run([_build_api_test(tmp_path), "gpu"])
    print(out)
    assert "elmat p2 api test ok" in out and out.count("worst") == 7
