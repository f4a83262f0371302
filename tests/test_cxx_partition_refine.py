"""The partitioner's boundary refinement through the C and C++ layers: the header compiles as C99 with the new entry points;
the MFEM adaptor's hook compiles with `refine_rounds` set against the declaration-only stand-in tests/mfem_stub/mfem.hpp;
saamge_amd::api::partition_refine / partition_mesh_refined refuse bad arguments without a GPU and, on the GPU, give the
model's partitions and counts."""
import os
import subprocess

import numpy as np
import pytest

import partition_seeding_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

C99 = r'''#include "saamge_amd.h"
int main(void) {
    long long xadj[3] = {0, 1, 2}, info[4] = {0, 0, 0, 0};
    int adj[2] = {1, 0}, part[2] = {0, 1};
    int (*mesh)(int, int, const int *, const int *, int, int, const int *, const saamge_amd_partition_options_v2 *, const int *,
                void *, saamge_amd_partitioning **) = saamge_amd_partition_mesh_refined;
    saamge_amd_partition_refine_info(info);
    /* refused before the graph is looked at: no GPU needed */
    return !(mesh && saamge_amd_partition_refine(2, xadj, adj, 2, part, -1, 0, 0, 0u, 0, 0, info) != 0 && part[1] == 1);
}
'''


def _run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout
    return p.stdout


def _lib_dir():
    lib_dir = os.path.join(ROOT, "saamge_amd")
    assert os.path.exists(os.path.join(lib_dir, "libsaamge_amd.so")), "run __graft_entry__.build() first"
    return lib_dir


def _build_api_test(tmp_path):
    lib_dir = _lib_dir()
    exe = str(tmp_path / "partition_refine_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC,
          os.path.join(ROOT, "tests", "cxx", "partition_refine_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_header_compiles_as_c99_with_the_new_entry_points(tmp_path):
    lib_dir = _lib_dir()
    src = tmp_path / "refine_c_abi.c"
    src.write_text(C99)
    exe = str(tmp_path / "refine_c_abi")
    _run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, str(src), "-o", exe, "-L", lib_dir, "-lsaamge_amd",
          "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    _run([exe])


def test_device_partitioner_hook_compiles_with_the_member(tmp_path):
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-DSAAMGE_AMD_WITH_MFEM", "-I", INC,
          "-I", os.path.join(ROOT, "tests", "mfem_stub"), "-c",
          os.path.join(ROOT, "tests", "cxx", "mock_partition_refine_driver.cpp"),
          "-o", str(tmp_path / "mock_partition_refine_driver.o")])


def test_calls_written_before_the_change_still_compile(tmp_path):
    for name in ("mock_partition_growth_driver", "mock_partition_seeding_driver", "mock_partition_driver"):
        _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-DSAAMGE_AMD_WITH_MFEM", "-I", INC,
              "-I", os.path.join(ROOT, "tests", "mfem_stub"), "-c", os.path.join(ROOT, "tests", "cxx", name + ".cpp"),
              "-o", str(tmp_path / (name + ".o"))])


def test_api_mirror_links_and_refuses_bad_arguments(tmp_path):
    assert "partition refine api test ok" in _run([_build_api_test(tmp_path)])


@pytest.mark.gpu
def test_api_mirror_gives_the_model_partitions_with_refinement(tmp_path):
    from saamge_amd import partition_model as pm
    out = _run([_build_api_test(tmp_path), "gpu"])
    assert "partition refine api test ok" in out
    ep, e2d, ND = sc.grid_mesh((6, 6, 4))
    info = []
    parts, nparts, _ = pm.partition_mesh(ep, e2d, ND, [8, 4], refine_rounds=[8, 8], refine_info=info)
    plain = pm.partition_mesh(ep, e2d, ND, [8, 4])[0]
    assert not np.array_equal(parts[0], plain[0])
    lines = [l for l in out.splitlines() if l.startswith("level")]
    assert len(lines) == 2
    for k, l in enumerate(lines):
        w = l.split()
        assert int(w[3]) == nparts[k]
        assert np.array_equal(np.array(w[5:], int), parts[k])
    got = [l for l in out.splitlines() if l.startswith("refine info")]
    assert len(got) == 1 and [int(x) for x in got[0].split()[2:]] == info
