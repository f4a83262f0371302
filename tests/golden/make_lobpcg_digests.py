#!/usr/bin/env python3
"""Writes tests/golden/lobpcg_parent_digests.json: sha256 of every output of Hierarchy.lobpcg for the cases of
tests/lobpcg_block_cases.py, on one MI355X.  It was run once, with the library of the commit before the eigensolver went
over to block V-cycles and block products; tests/test_gpu_lobpcg_block.py asserts that the digests have not moved.

    python tests/golden/make_lobpcg_digests.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from saamge_amd import capi  # noqa: E402

import lobpcg_block_cases as bc  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lobpcg_parent_digests.json")
    digests = {bc.case_id(c): bc.run(capi, c) for c in bc.CASES}
    with open(out, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    for k, v in sorted(digests.items()):
        print(k, v["evals"][:16], v["evecs"][:16], v["hist"][:16])


if __name__ == "__main__":
    main()
