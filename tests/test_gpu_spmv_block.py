"""saamge_amd_spmv_block against saamge_amd_spmv, bit for bit per column, on every path of the block SpMV family; matrices
and assertions: tests/spmv_block_cases.py.  One child process per setting of the library's options (they are read when the
library is loaded), as tests/test_gpu_sell.py does."""
import os
import subprocess
import sys

import pytest

import spmv_block_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))

_CODE = "import sys; sys.path[:0] = [%r, %r]; import spmv_block_cases as bc; bc.child_main(%r)"

# saamge_amd_options.sell: bit 0 coded slices at all, 1 pair coding, 2 short-chain path, 3 dictionary, 4 node blocks
SETTINGS = {
    "sell31": "spmv_sell=1,sell=31",
    "sell27": "spmv_sell=1,sell=27",              # without the short-chain path
    "offsets_only": "spmv_sell=1,sell=29",        # no pair coding
    "plain": "spmv_sell=1,sell=28",               # no codes
    "csr": "spmv_sell=0",
}
DICT_SETTINGS = {
    "dict_blocks": "spmv_sell=1,sell=31",
    "dict": "spmv_sell=1,sell=15",                # without bit 4: no node blocks
    "no_dict": "spmv_sell=1,sell=7",              # without bits 3 and 4: plain slices through sell_block_kernel
}


def _child(which, options):
    env = dict(os.environ, SAAMGE_AMD_TEST_OPTIONS=options)
    o = subprocess.run([sys.executable, "-c", _CODE % (ROOT, TESTS, which)], env=env, capture_output=True, text=True, timeout=600)
    assert o.returncode == 0, o.stdout[-4000:] + o.stderr[-4000:]
    done = [l for l in o.stdout.splitlines() if l.startswith("DONE")]
    ok = [l.split()[1] for l in o.stdout.splitlines() if l.startswith("OK")]
    return ok, int(done[0].split()[1])


@pytest.mark.gpu
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_block_columns_equal_single_spmv(setting):
    ok, calls = _child("all", SETTINGS[setting])
    assert len(ok) == 7 + len(bc.P_AVG) and calls == len(ok) * len(bc.KS) * 2


@pytest.mark.gpu
@pytest.mark.parametrize("setting", sorted(DICT_SETTINGS))
def test_block_columns_equal_single_spmv_on_the_dictionary_operator(setting):
    ok, calls = _child("dict", DICT_SETTINGS[setting])
    assert ok == ["elasticity_q2_10"] and calls == len(bc.KS) * 2


def test_rectangular_matrices_cover_every_lanes_per_row():
    """the shapes the CSR block kernel is instantiated for, each with empty rows and a row count that is no multiple of 64"""
    assert sorted(bc.P_AVG) == [1, 2, 4, 8, 16, 32, 64]
    for lanes in bc.P_AVG:
        A = bc.p_shaped(lanes)
        assert A.shape == bc.P_SHAPE and A.shape[0] % 64 != 0
        assert bc.lanes_per_row(A.nnz, A.shape[0]) == lanes
        assert (A.indptr[1:] == A.indptr[:-1]).sum() >= A.shape[0] // 13
