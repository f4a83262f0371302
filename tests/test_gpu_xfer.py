"""The transfer layer (csrc/xfer.h) on its own: tests/cxx/xfer_test.hip, which csrc/Makefile builds next to the library, puts
every form of copy -- staged and direct uploads, enqueue-only uploads and their refusals, the reads back, the copies into a
caller's memory, the input and output wrappers, device to device -- through sizes around the staging threshold and compares
with patterns written on the host or by a fill kernel.  The program runs once, as a child process."""
import pathlib
import subprocess

import pytest

pytestmark = pytest.mark.gpu

PROGRAM = pathlib.Path(__file__).resolve().parent / "cxx" / "xfer_test"
GROUPS = ("sources", "enqueue-only bounds", "device to host", "wrappers", "copy_device")


def test_xfer_program():
    assert PROGRAM.exists(), "tests/cxx/xfer_test is missing: build() (make -C saamge_amd/csrc) builds it"
    p = subprocess.run([str(PROGRAM)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, text=True)
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0, p.stdout
    assert lines and lines[-1] == "xfer test ok", p.stdout
    assert lines[:-1] == [g + ": ok" for g in GROUPS], p.stdout
