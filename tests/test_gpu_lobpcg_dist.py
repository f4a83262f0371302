"""The eigensolver refuses a hierarchy whose level 0 is row-partitioned over several ranks (multi-rank is not built): two
gloo ranks share the card as in tests/test_gpu_dist.py, with dist_min_local_rows = 1 every level is row-partitioned, and
each rank calls saamge_amd_lobpcg with outputs pre-filled with a sentinel.  The refusal comes before any collective, so
every rank returns on its own: a nonzero code, a message that names `h` and the row partition, nothing written."""
import json
import os
import socket
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = textwrap.dedent("""
    import sys, json, ctypes as C
    sys.path.insert(0, %r)
    import numpy as np
    from saamge_amd import capi, problems as pr
    from saamge_amd.dist import Group
    grp = Group(backend="gloo")
    prob = pr.poisson3d_problem((16, 16, 16), blk=(8, 8, 4), coarse_blk=[(2, 2, 2)], coef="checkerboard")
    params = capi.default_params(num_coarsenings=2, dist_min_local_rows=1)
    h = capi.Hierarchy.from_problem(prob, params, group=grp)
    n, sentinel = prob.ND, -777.25
    o = capi.LobpcgOptions()
    lib = capi.load()
    lib.saamge_amd_lobpcg_options_default(C.byref(o))
    o.nev, o.max_iter = 2, 5
    ev, X, res, hist = (np.full(s, sentinel) for s in (2, 2 * n, 2, 6 * 2))
    it, conv = C.c_int(-7), C.c_int(-7)
    rc = lib.saamge_amd_lobpcg(h.h, None, None, None, C.byref(o), None, capi._ptr(ev), capi._ptr(X), capi._ptr(res),
                               C.byref(it), C.byref(conv), capi._ptr(hist))
    out = dict(partitioned=bool(h.level_info(0)["row_partitioned"]), rc=int(rc), msg=lib.saamge_amd_last_error().decode(),
               untouched=bool(all(np.all(a == sentinel) for a in (ev, X, res, hist)) and it.value == -7 and conv.value == -7))
    x, iters, converged, _ = h.pcg(prob.b, rel_tol=1e-8)          # the hierarchy still solves after the refusal
    out["pcg_converged"] = bool(converged)
    json.dump(out, open(sys.argv[1], "w"))
    h.close()
    grp.barrier()
    grp.close()
""" % ROOT)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_a_row_partitioned_level_0_is_refused_on_every_rank(tmp_path):
    world = 2
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    port = _free_port()
    procs, outs = [], []
    for rank in range(world):
        env = dict(os.environ, WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        outs.append(str(tmp_path / ("r%d.json" % rank)))
        procs.append(subprocess.Popen([sys.executable, str(script), outs[-1]], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, lg in zip(procs, logs):
        assert p.returncode == 0, lg[-3000:]
    for o in outs:
        r = json.load(open(o))
        assert r["partitioned"], r
        assert r["rc"] != 0 and r["untouched"], r
        assert "lobpcg: h:" in r["msg"] and "row-partitioned" in r["msg"], r
        assert r["pcg_converged"], r
