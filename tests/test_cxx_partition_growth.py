"""The partitioner's `growth` option through the C++ layers: the MFEM adaptor's ml_device_partitioner compiles with the
field set against the declaration-only stand-in tests/mfem_stub/mfem.hpp; saamge_amd::api::partition_graph / partition_mesh
refuse a bad value without a GPU and, on the GPU, give the model's partition and counts with balanced growth."""
import os
import subprocess

import numpy as np
import pytest

import partition_seeding_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout
    return p.stdout


def _build_api_test(tmp_path):
    lib_dir = os.path.join(ROOT, "saamge_amd")
    assert os.path.exists(os.path.join(lib_dir, "libsaamge_amd.so")), "run __graft_entry__.build() first"
    exe = str(tmp_path / "partition_growth_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC,
          os.path.join(ROOT, "tests", "cxx", "partition_growth_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_device_partitioner_hook_compiles_with_the_field(tmp_path):
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-DSAAMGE_AMD_WITH_MFEM", "-I", INC,
          "-I", os.path.join(ROOT, "tests", "mfem_stub"), "-c",
          os.path.join(ROOT, "tests", "cxx", "mock_partition_growth_driver.cpp"),
          "-o", str(tmp_path / "mock_partition_growth_driver.o")])


def test_api_mirror_links_and_refuses_a_bad_growth(tmp_path):
    assert "partition growth api test ok" in _run([_build_api_test(tmp_path)])


@pytest.mark.gpu
def test_api_mirror_gives_the_model_partition_with_balanced_growth(tmp_path):
    from saamge_amd import partition_model as pm
    out = _run([_build_api_test(tmp_path), "gpu"])
    assert "partition growth api test ok" in out
    ep, e2d, ND = sc.grid_mesh((6, 6, 4))
    info = []
    parts, nparts, _ = pm.partition_mesh(ep, e2d, ND, [8, 4], growth=1, growth_info=info)
    lines = [l for l in out.splitlines() if l.startswith("level")]
    assert len(lines) == 2
    for k, l in enumerate(lines):
        w = l.split()
        assert int(w[3]) == nparts[k]
        assert np.array_equal(np.array(w[5:], int), parts[k])
    got = [l for l in out.splitlines() if l.startswith("growth info")]
    assert len(got) == 1 and [int(x) for x in got[0].split()[2:]] == info
