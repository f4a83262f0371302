"""The partitioner through the C++ layers: the MFEM adaptor's ml_device_partitioner compiles against the declaration-only
stand-in tests/mfem_stub/mfem.hpp; saamge_amd::api::partition_graph / partition_mesh link the library, refuse bad arguments
without a GPU and, on the GPU, give the model's partition."""
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
    exe = str(tmp_path / "partition_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC, os.path.join(ROOT, "tests", "cxx", "partition_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_device_partitioner_hook_compiles_against_stub(tmp_path):
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-DSAAMGE_AMD_WITH_MFEM", "-I", INC,
          "-I", os.path.join(ROOT, "tests", "mfem_stub"), "-c", os.path.join(ROOT, "tests", "cxx", "mock_partition_driver.cpp"),
          "-o", str(tmp_path / "mock_partition_driver.o")])


def test_adaptor_takes_the_produced_count_when_the_hook_is_installed():
    """The rule itself, read from the header: with the device partitioner installed the level sizes come from
    max(partition) + 1, and a caller's own std::function switches that off again."""
    hdr = open(os.path.join(INC, "saamge_amd_mfem.hpp")).read()
    assert "if (counted) nparts[(size_t)k] = detail::count_parts(parts[(size_t)k].data(), n_el);" in hdr
    assert "n_el = nparts[(size_t)k - 1]" in hdr
    assert "inline void ml_set_coarse_partitioner(const ml_partitioner_t &p) { ml_coarse_partitioner() = p; detail::partitioner_counts()[1] = false; }" in hdr


def test_api_mirror_links_and_refuses_bad_arguments(tmp_path):
    assert "partition api test ok" in _run([_build_api_test(tmp_path)])


@pytest.mark.gpu
def test_api_mirror_gives_the_model_partition(tmp_path):
    from saamge_amd import partition_model as pm
    out = _run([_build_api_test(tmp_path), "gpu"])
    n, nv = 4, 5
    e2d = np.array([((z + (c >> 2)) * nv + y + ((c >> 1) & 1)) * nv + x + (c & 1)
                    for z in range(n) for y in range(n) for x in range(n) for c in range(8)], np.int32)
    parts, nparts, _ = pm.partition_mesh(np.arange(0, 8 * n ** 3 + 1, 8), e2d, nv ** 3, [8, 4])
    lines = [l for l in out.splitlines() if l.startswith("level")]
    assert len(lines) == 2
    for k, l in enumerate(lines):
        w = l.split()
        assert int(w[3]) == nparts[k]
        assert np.array_equal(np.array(w[5:], int), parts[k])
