"""Row patterns of the staged SELL tiles (csrc/sparse.hip, sell_row_patterns_kernel): a staged tile streams one byte per row
naming one of at most SELL_PMAX distinct code-word rows instead of every row's code words.  The products and their order are
those of the code-word path, so every result is bit for bit what saamge_amd_options.sell bit 6 (row patterns OFF) gives."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

_CODE = r"""
import sys, hashlib, numpy as np, scipy.sparse as sp, torch
sys.path.insert(0, %r)
from saamge_amd import capi, problems as pr
rng = np.random.default_rng(3)

def overflow_operator(n=8192):
    # 17 fixed diagonals, one value each (pair-coded, one table per tile); the rows of every odd tile take a random subset of
    # them (more than SELL_PMAX distinct rows: the tile keeps its code words), those of the even tiles all of them
    offs = np.arange(-40, 41, 5)
    r = np.random.default_rng(11)
    rows, cols, vals = [], [], []
    for i in range(n):
        pick = np.ones(offs.size, bool) if (i // 256) %% 2 == 0 else r.random(offs.size) < 0.5
        pick[offs == 0] = True
        for j in np.nonzero(pick)[0]:
            c = i + offs[j]
            if 0 <= c < n:
                rows.append(i); cols.append(c); vals.append(1.0 + 0.125 * j)
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n))

mats = {
  "stencil_const_short_rows": pr.poisson3d_problem((8, 8, 8), blk=(4, 4, 2)).A.tocsr(),
  "toeplitz_wide_band": sp.diags([np.full(6000 - abs(o), 1.0 + 0.01 * j) for j, o in enumerate(range(-600, 600, 40))],
                                 list(range(-600, 600, 40)), format="csr"),
  "stencil_2d": (sp.kron(sp.diags([1.0, 2.0, 1.0], [-1, 0, 1], shape=(40, 40)), sp.diags([1.0, -4.0, 1.0], [-1, 0, 1], shape=(300, 300)))).tocsr(),
  "tiny": sp.csr_matrix(np.array([[2.0, -1.0, 0.0], [-1.0, 2.0, -1.0], [0.0, -1.0, 2.0]])),
  "overflow": overflow_operator(),
}
for name, A in mats.items():
    A = A.tocsr(); A.sort_indices()
    x = rng.standard_normal(A.shape[1])
    y = capi.spmv(A, x)
    err = np.abs(y - A @ x).max() / (np.abs(A) @ np.abs(x)).max()
    print("RESULT", name, repr(float(err)), hashlib.sha256(y.tobytes()).hexdigest(), flush=True)
    print("---", name, file=sys.stderr, flush=True)

# fused smoother step, residual and plain modes on a small Poisson hierarchy: smoother, V-cycle and PCG
print("--- hierarchy", file=sys.stderr, flush=True)
prob = pr.poisson3d_problem((24, 24, 24), blk=(4, 4, 4))
h = capi.Hierarchy.from_problem(prob, capi.default_params(num_coarsenings=1))
n0 = h.level_info(0)["n"]
bb = torch.tensor(rng.standard_normal(n0), dtype=torch.float64, device="cuda:0")
xx = torch.zeros_like(bb)
h.smoother(0, bb, xx)
h.smoother(0, bb, xx)
outs = [xx.cpu().numpy(), np.asarray(h.vcycle(prob.b), dtype=np.float64)]
xs, it, conv, hist = h.pcg(prob.b, rel_tol=1e-10, max_iter=50)
outs += [np.asarray(hist, dtype=np.float64), np.asarray(xs, dtype=np.float64)]
h.close()
print("RESULT hierarchy 0.0", hashlib.sha256(b"".join(v.tobytes() for v in outs)).hexdigest(), flush=True)
"""

_PLAN = re.compile(r"build_sell: staging plan: (\d+) of (\d+) tiles, largest \d+ doubles, row patterns in (\d+) tiles \(at most (\d+)\)")


def _run(patterns):
    sell = 31 if patterns else 31 | 64
    env = dict(os.environ, SAAMGE_AMD_TEST_OPTIONS="spmv_sell=1,debug=2,sell=%d" % sell)
    o = subprocess.run([sys.executable, "-c", _CODE % ROOT], env=env, capture_output=True, text=True, timeout=900)
    assert o.returncode == 0, o.stdout + o.stderr
    res = {}
    for line in o.stdout.splitlines():
        if line.startswith("RESULT"):
            _, name, err, digest = line.split()
            res[name] = (float(err), digest)
    # staging-plan census of each operator, under the name of the operator built before the next "---" marker
    plans, cur = {}, []
    for line in o.stderr.splitlines():
        m = _PLAN.search(line)
        if m:
            cur.append(tuple(int(v) for v in m.groups()))
        elif line.startswith("--- "):
            plans[line[4:].strip()] = cur
            cur = []
    plans["hierarchy"] = plans.get("hierarchy", []) + cur
    return res, plans


def test_row_patterns_give_the_same_bits_as_code_words():
    on, plans_on = _run(True)
    off, plans_off = _run(False)
    assert set(on) == set(off) and len(on) == 6
    for name in on:
        assert on[name][0] <= 1e-15, (name, on[name])
        assert on[name][1] == off[name][1], name      # identical bits
    # the paths really ran: pattern tiles with the switch on, none with it off
    # (operators whose staged tiles keep a table per slice take sell_staged_kernel, without patterns: 0 pattern tiles)
    for name in ("stencil_const_short_rows", "stencil_2d", "toeplitz_wide_band"):
        staged, _, pat, pmax = plans_on[name][-1]
        assert pat in (0, staged) and pmax <= 16, (name, plans_on[name])
    assert sum(plans_on[name][-1][2] for name in ("stencil_const_short_rows", "stencil_2d", "toeplitz_wide_band")) > 0, plans_on
    staged, _, pat, pmax = plans_on["overflow"][-1]
    assert 0 < pat < staged and pmax <= 16, plans_on["overflow"]      # the odd tiles overflow and keep their code words
    assert any(p[0] > 0 and p[2] > 0 for p in plans_on["hierarchy"]), plans_on["hierarchy"]
    assert all(p[2] == 0 for ps in plans_off.values() for p in ps), plans_off


def test_fine_level_tiles_of_the_scale_golden_are_mostly_pattern_tiles(capfd):
    """On the 64 x 64 x 32 three-level golden nearly every staged tile of the fine-level operator has at most SELL_PMAX row
    patterns (debug census: 530 of 544; the others, at the faces where y- and z-lines end inside one tile, keep their code
    words), and the golden comes out with both kinds of tile in one operator."""
    import test_gpu_scale as S
    from saamge_amd import capi
    old = capi.set_options(debug=2)
    try:
        g, out = S._run("scale_64x64x32", "subspace")
        S._check(g, out, "scale_64x64x32/row patterns")
    finally:
        capi.load().saamge_amd_set_options(__import__("ctypes").byref(old))
    plans = [tuple(int(v) for v in m.groups()) for m in _PLAN.finditer(capfd.readouterr().err)]
    fine = max(plans, key=lambda p: p[1])
    assert fine[0] > 0 and 0.9 * fine[0] <= fine[2] < fine[0] and fine[3] <= 16, plans


def test_scale_golden_with_row_patterns_off():
    import test_gpu_scale as S
    from saamge_amd import capi
    old = capi.set_options(sell=31 | 64)
    try:
        g, out = S._run("scale_64x64x32", "subspace")
        S._check(g, out, "scale_64x64x32/sell=95")
    finally:
        capi.load().saamge_amd_set_options(__import__("ctypes").byref(old))
