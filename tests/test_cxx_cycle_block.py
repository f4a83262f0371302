"""The chunking rule of the block kernels (saamge_amd/csrc/block_chunks.h: plain constexpr C++) held on the CPU, and the four
block calls through the C++ layer: compiled and their refusals checked without a GPU, run on `tiles` on the GPU against the
single-vector calls, byte for byte (tests/cxx/cycle_block_api_test.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import solve_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "saamge_amd", "csrc")


def _run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout
    return p.stdout


def _build(tmp_path):
    lib_dir = os.path.join(ROOT, "saamge_amd")
    assert os.path.exists(os.path.join(lib_dir, "libsaamge_amd.so")), "run __graft_entry__.build() first"
    exe = str(tmp_path / "cycle_block_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC, "-I", CSRC,
          os.path.join(ROOT, "tests", "cxx", "cycle_block_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_chunk_rule_holds_and_the_api_mirror_refuses_bad_arguments(tmp_path):
    assert "cycle block api test ok" in _run([_build(tmp_path)])


@pytest.mark.gpu
def test_api_mirror_block_calls_equal_single_calls_on_tiles(tmp_path):
    p = sc.problem("tiles")
    A = p.A.tocsr()
    A.sort_indices()
    n, NE, nde = A.shape[0], p.elem_to_dof.shape[0], p.elem_to_dof.shape[1]
    part = np.asarray(p.partitions[0], dtype=np.int32)
    rng = np.random.default_rng(5)
    cols = np.stack([np.asarray(p.b, dtype=np.float64), rng.standard_normal(n), np.zeros(n)])       # K = 3 columns
    problem = str(tmp_path / "tiles.bin")
    with open(problem, "wb") as f:
        for a, dt in ((np.array([n, A.nnz, NE, nde, int(part.max()) + 1]), np.int32), (A.indptr, np.int32), (A.indices, np.int32),
                      (A.data, np.float64), (p.elem_to_dof, np.int32), (p.elmat, np.float64), (p.bdr, np.int8), (part, np.int32),
                      (cols, np.float64)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    assert "cycle block api test ok" in _run([_build(tmp_path), "gpu", problem])
