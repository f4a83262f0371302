"""Setup time of an all-hex Q1 grid against the same grid with half of its vertical columns split into P1 wedges
(problems.poisson3d_mixed_problem, wedges="half"), device-resident inputs: the mixed mesh goes through
saamge_amd_ml_produce_data_mixed, the hexes through saamge_amd_ml_produce_data.  After one warm-up each, `--reps` setups
of each, alternating, are timed without the profiler; then one profiled setup of each gives the ae_rows / ae_build
kernel times.  Prints one JSON line.

    python tools/mixed_setup_time.py [--n 128] [--blk 8,8,4] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from saamge_amd import capi, problems

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--blk", default="8,8,4")
    ap.add_argument("--coarse-blk", default="8,8,4")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    blk = tuple(int(x) for x in a.blk.split(","))
    cblk = [tuple(int(x) for x in a.coarse_blk.split(","))]
    dev = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).cuda()

    hexp = problems.poisson3d_device(a.n, blk=blk, coarse_blk=cblk, device="cuda")
    t0 = time.perf_counter()
    mp = problems.poisson3d_mixed_problem(a.n, blk, coarse_blk=cblk, wedges="half")
    gen_s = time.perf_counter() - t0
    A = mp.A.tocsr()
    mixed = dict(rowptr=dev(A.indptr, np.int32), col=dev(A.indices, np.int32), val=dev(A.data, np.float64),
                 e2d=dev(mp.elem_to_dof, np.int32), eptr=dev(mp.elem_ptr, np.int32), elmat=dev(mp.elmat, np.float64),
                 bdr=dev(mp.bdr, np.int8), parts=[dev(mp.partitions[0], np.int32)] + list(mp.partitions[1:]),
                 nparts=[int(p.max()) + 1 for p in mp.partitions])
    del mp, A

    def setup(kind):
        params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3)
        stream = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()
        t = time.perf_counter()
        if kind == "hex":
            h = capi.Hierarchy(hexp.rowptr, hexp.col, hexp.val, hexp.n, hexp.elem_to_dof, hexp.elmat, hexp.bdr,
                               hexp.partitions, hexp.nparts, params, hexp.NE_, 8, stream=stream)
        else:
            m = mixed
            h = capi.Hierarchy(m["rowptr"], m["col"], m["val"], int(m["rowptr"].numel()) - 1, m["e2d"], m["elmat"], m["bdr"],
                               m["parts"], m["nparts"], params, int(m["eptr"].numel()) - 1, 0, stream=stream,
                               elem_ptr=m["eptr"])
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t)
        info = h.level_info(0)
        h.close()
        return ms, info

    out = {"n": a.n, "blk": blk, "mixed_generator_s": round(gen_s, 1)}
    for kind in ("hex", "mixed"):
        setup(kind)                                   # warm-up
    times = {"hex": [], "mixed": []}
    for _ in range(a.reps):
        for kind in ("hex", "mixed"):
            times[kind].append(setup(kind)[0])
    for kind in ("hex", "mixed"):
        capi.profile(True)
        capi.profile_reset()
        _, info = setup(kind)
        stats = {r["name"]: r for r in capi.profile_stats()}
        capi.profile(False)
        out[kind] = {"setup_ms": [round(t, 1) for t in times[kind]], "setup_ms_median": round(float(np.median(times[kind])), 1),
                     "rows": int(info["n"]), "nparts": int(info["nparts"]),
                     "ae_rows_ms": round(stats["ae_rows"]["ms"], 3) if "ae_rows" in stats else None,
                     "ae_build_ms": round(stats["ae_build"]["ms"], 3) if "ae_build" in stats else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
