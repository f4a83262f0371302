"""The face table through the C++ layer: saamge_amd::api::FaceTable, face_nodes and face_dofs_into link the library under
-Wall -Wextra -Werror, refuse dim = 4, a NULL vertex list and comp_mask = 0 without a GPU and, on the GPU, give the model's
integers on a two-hex mesh and the flags of one face."""
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
    exe = str(tmp_path / "mesh_faces_api_test")
    _run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", INC, os.path.join(ROOT, "tests", "cxx", "mesh_faces_api_test.cpp"),
          "-o", exe, "-L", lib_dir, "-lsaamge_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_api_mirror_links_and_refuses_dim_4_a_null_vertex_list_and_an_empty_mask(tmp_path):
    assert "mesh faces api test ok" in _run([_build_api_test(tmp_path)])


@pytest.mark.gpu
def test_api_mirror_gives_the_model_integers(tmp_path):
    from saamge_amd import elmat_model as em
    from saamge_amd import mesh_model as mm
    out = _run([_build_api_test(tmp_path), "gpu"])
    nx, gx = 2, 3
    NV = gx * 4
    e2v = np.array([(lz * 2 + ly) * gx + e + lx for e in range(nx) for (lx, ly, lz) in em.HEX_LOC], np.int32).reshape(nx, 8)
    T = mm.FaceTable(NV, 3, e2v)
    ptr, nodes = mm.face_nodes(3, e2v, None, [0], [4])
    flags = np.ones(3 * NV, np.int8)
    assert mm.face_dofs(3, e2v, None, [0], [4], 3, 5, 0x02, flags) == [1, 4, 8, -1]
    all_flags = np.zeros(NV, np.int8)
    mm.face_dofs(3, e2v, None, T.bdr_elem, T.bdr_local, 1, 1, 0x02, all_flags)
    want = dict(zip(("slot_ptr", "nbr_elem", "nbr_local", "bdr_elem", "bdr_local", "xadj", "adj"), T.arrays()))
    want.update(face_ptr=ptr, face_nodes=nodes, flags=flags, all_flags=all_flags)
    lines = {l.split()[0]: np.array([int(t) for t in l.split()[1:]], np.int64) for l in out.splitlines()
             if l.split() and l.split()[0] in want}
    for tag, w in want.items():
        assert np.array_equal(lines[tag], np.asarray(w).ravel()), tag
