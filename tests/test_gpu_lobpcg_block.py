"""The eigensolver applies its V-cycles and operator products to blocks of columns; every output keeps the bits it had when
they ran one column at a time.  tests/golden/lobpcg_parent_digests.json holds sha256 of evals, evecs, res, hist, iters and
converged as the library gave them before the switch (tests/golden/make_lobpcg_digests.py, run once on an MI355X); the
cases: tests/lobpcg_block_cases.py."""
import json
import os

import pytest

import lobpcg_block_cases as bc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lobpcg_parent_digests.json")


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_every_output_keeps_the_bits_of_the_column_by_column_eigensolver(case):
    from saamge_amd import capi
    assert hasattr(capi.load(), "saamge_amd_vcycle_block"), "this library predates the block solve phase"
    with open(GOLDEN) as f:
        want = json.load(f)[bc.case_id(case)]
    got = bc.run(capi, case)
    assert sorted(got) == sorted(bc.FIELDS)
    assert got == want
