"""The columns of tests/cycle_block_cases.py leave the PCG loop at different steps -- checked here with the oracle's PCG on
the CPU, so that tests/test_gpu_cycle_block.py compares block and single calls over every exit of the loop."""
import pytest

import cycle_block_cases as cb
import lobpcg_cases as lc


@pytest.mark.parametrize("name", cb.HIERARCHIES)
@pytest.mark.parametrize("nu", cb.NUS)
def test_columns_take_every_exit_of_the_oracles_pcg(name, nu):
    from oracle import saamge_oracle as o
    H = lc.oracle_hierarchy(name)
    saved = [lv.roots for lv in H.levels]
    try:
        for lv in H.levels:
            lv.roots = o.sas_poly_roots(nu)
        cols = cb.columns(name)
        out = [o.solve(H, cols[j], rel_tol=cb.PCG_KW["rel_tol"], abs_tol=cb.ABS_TOL[name, nu], max_iter=cb.MAX_ITER)[1:3]
               for j in range(cb.KMAX)]
    finally:
        for lv, r in zip(H.levels, saved):
            lv.roots = r
    iters, conv = [int(i) for i, _ in out], [bool(c) for _, c in out]
    print(name, nu, list(zip(iters, conv)))
    assert iters[0] == 0 and conv[0]                                  # the zero column
    assert iters[1] != iters[0]                                       # already two columns differ
    first5 = list(zip(iters[:5], conv[:5]))
    assert (cb.MAX_ITER, False) in first5                             # one stops on max_iter ...
    assert any(c and 0 < i < cb.MAX_ITER for i, c in first5)          # ... one converges before it
    assert len(set(iters[:5])) >= 3
