"""The helper every overlap worker of the setup runs through (csrc/side_task.h: start a piece of work on a thread of its own
or in line, keep what it throws, rethrow it once at the join) is plain host C++: tests/cxx/side_task_test.cpp checks it
without a GPU, once under the thread sanitizer and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout
    return p.stdout


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_a_side_task_hands_over_results_and_exceptions_at_the_join(tmp_path, sanitize):
    exe = str(tmp_path / "side_task_test")
    _run(["g++", "-std=c++17", "-pthread", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=" + sanitize,
          "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "saamge_amd", "csrc"),
          os.path.join(ROOT, "tests", "cxx", "side_task_test.cpp"), "-o", exe])
    assert "side task test ok" in _run([exe])
