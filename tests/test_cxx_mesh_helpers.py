"""The pieces the mesh kernels share (csrc/mesh_helpers.h: the sorting networks of four and eight, the bisection for the last
entry <= x, the slot across a face; csrc/elmat_types.h: the corners of the 27-node hexahedron) are plain host C++:
tests/cxx/mesh_helpers_test.cpp holds them to std::sort, std::upper_bound and values written out, without a GPU and under the
address and undefined-behaviour sanitizers.  The kernels call the same functions; the GPU tests hold what they compute with them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout
    return p.stdout


def test_the_shared_helpers_sort_search_and_index_as_written_out(tmp_path):
    exe = str(tmp_path / "mesh_helpers_test")
    _run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
          os.path.join(ROOT, "saamge_amd", "csrc"), os.path.join(ROOT, "tests", "cxx", "mesh_helpers_test.cpp"), "-o", exe])
    assert "mesh helpers test ok" in _run([exe])
