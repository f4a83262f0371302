"""The `ae_order` option through the C++ layer: saamge_amd::api::ae_order / level_order_info compile and link, the field is the
last one of saamge_amd_options, a bad mode is refused without a GPU; on the GPU the wrapper gives the model's integers."""
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
    exe = str(tmp_path / "ae_order_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC,
          os.path.join(ROOT, "tests", "cxx", "ae_order_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_api_mirror_links_and_refuses_a_bad_ae_order(tmp_path):
    assert "ae order api test ok" in _run([_build_api_test(tmp_path)])


@pytest.mark.gpu
def test_api_mirror_gives_the_models_order(tmp_path):
    from saamge_amd import ae_order_model as om
    out = _run([_build_api_test(tmp_path), "gpu"])
    assert "ae order api test ok" in out
    nx = ny = 12
    vx, nv = nx + 1, (nx + 1) * (ny + 1)
    num = (np.arange(nv) * 59) % nv
    quads = [[y * vx + x, y * vx + x + 1, (y + 1) * vx + x + 1, (y + 1) * vx + x] for y in range(ny) for x in range(nx)]
    elems = [[[int(num[v]) for v in q] for q in quads if (q[0] // vx < 8) == (a == 0)] for a in range(2)]
    lines = [l.split() for l in out.splitlines() if l.startswith("mode")]
    assert len(lines) == 4
    taken = 0
    for w in lines:
        mode, a = int(w[1]), int(w[3])
        pairs = [t.split(":") for t in w[11:]]
        dofs = np.array([int(d) for d, _ in pairs])
        pos = np.array([int(p) for _, p in pairs])
        want = om.ae_order(dofs, elems[a], mode)
        assert (int(w[5]), int(w[7]), int(w[9])) == want[1:]
        assert np.array_equal(pos, want[0])
        taken += want[3]
    assert taken == 2
