"""The shared pieces of the device index tables (csrc/devtab.h, csrc/devsort.h) on their own: tests/cxx/devtab_test.hip, which
csrc/Makefile builds next to the library, holds the scans, the table transpose in its four forms, the compaction, the
elementwise kernels, the histogram and the stable sort to serial host loops.  The program runs once, as a child process."""
import pathlib
import subprocess

import pytest

pytestmark = pytest.mark.gpu

PROGRAM = pathlib.Path(__file__).resolve().parent / "cxx" / "devtab_test"
GROUPS = ("scan int", "scan roff_t", "transpose (sorted, two-step, unsorted, async)", "compact",
          "fill, iota, convert, gather, scatter", "histogram", "stable sort by key")


def test_devtab_program():
    assert PROGRAM.exists(), "tests/cxx/devtab_test is missing: build() (make -C saamge_amd/csrc) builds it"
    p = subprocess.run([str(PROGRAM)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, text=True)
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0, p.stdout
    assert lines and lines[-1] == "devtab test ok", p.stdout
    assert lines[:-1] == [g + ": ok" for g in GROUPS], p.stdout
