"""Times the device assembly of the fine operator: the whole of saamge_amd_operator_assemble, the numeric pass alone
(saamge_amd_operator_update), the peak device bytes above the output, and the numeric pass against its HBM lower bound
(elmat read once + val written once at --hbm-gbs), beside the hierarchy setup of the same problem on the assembled
operator.  Host clock closed by a synchronise, one warm-up, `--reps` repetitions (all listed).  One JSON line per case.

    python tools/assemble_time.py [--hex 128,256] [--mixed 64] [--q2 32,96] [--reps 3] [--hbm-gbs 8000] [--no-setup]

symbolic_ms is the time of the assembly minus the numeric pass timed alone (it includes the dof -> element table, the
checks and the row lists).  A case that does not fit the device is reported as skipped with the error.
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
    ap.add_argument("--hex", default="128,256")
    ap.add_argument("--mixed", default="64")
    ap.add_argument("--q2", default="32,96")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--no-setup", action="store_true")
    a = ap.parse_args()
    ints = lambda v: [int(x) for x in v.split(",") if x]
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), r

    def dev(x, dt):
        return x if hasattr(x, "data_ptr") else torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).cuda()

    def hex_case(n):
        p = problems.poisson3d_device(n, blk=(8, 8, 4), coarse_blk=[(8, 8, 4)], device="cuda")
        return dict(n=p.n, NE=p.NE_, nde=8, eptr=None, e2d=p.elem_to_dof, elmat=p.elmat, bdr=p.bdr, parts=p.partitions,
                    nparts=p.nparts, nc=2)

    def mixed_case(n):
        p = problems.poisson3d_mixed_problem(n, (8, 8, 4), coarse_blk=[(8, 8, 4)], wedges="half")
        parts = [dev(q, np.int32) for q in p.partitions]
        return dict(n=p.ND, NE=p.NE, nde=0, eptr=dev(p.elem_ptr, np.int32), e2d=dev(p.elem_to_dof, np.int32),
                    elmat=dev(p.elmat, np.float64), bdr=dev(p.bdr, np.int8), parts=parts,
                    nparts=[int(q.max()) + 1 for q in p.partitions], nc=2)

    def q2_case(n):
        p = problems.elasticity3d_q2_device(n, blk=(4, 4, 4), device="cuda")
        return dict(n=p.n, NE=p.NE_, nde=81, eptr=None, e2d=p.elem_to_dof, elmat=p.elmat, bdr=p.bdr, parts=p.partitions,
                    nparts=p.nparts, nc=1)

    cases = [("hex%d" % n, hex_case, n) for n in ints(a.hex)] + [("mixed%d" % n, mixed_case, n) for n in ints(a.mixed)] + \
            [("q2_elasticity%d" % n, q2_case, n) for n in ints(a.q2)]
    for name, make, n in cases:
        try:
            c = make(n)
            asm = lambda: capi.Operator(c["n"], c["e2d"], c["elmat"], c["bdr"], elem_ptr=c["eptr"], nde=c["nde"], NE=c["NE"],
                                        stream=stream())
            _, op = timed(asm)                     # warm-up
            nnz, paths = op.nnz, op.path_counts()
            timed(lambda: op.update(c["elmat"]))
            t_num = [timed(lambda: op.update(c["elmat"]))[0] for _ in range(a.reps)]
            op.close()
            out_bytes = 8 * (c["n"] + 1) + 12 * nnz
            t_asm = []
            live0 = capi.memory_stats(reset_peak=True)[0]
            for _ in range(a.reps):
                t, op = timed(asm)
                t_asm.append(t)
                if _ + 1 < a.reps:
                    op.close()
            peak = capi.memory_stats()[1] - live0
            elmat_bytes = 8 * int(c["elmat"].numel())
            bound_ms = 1e3 * (elmat_bytes + 8 * nnz) / (a.hbm_gbs * 1e9)
            rec = {"case": name, "rows": c["n"], "elements": c["NE"], "nnz": nnz, "paths": paths,
                   "assemble_ms": [round(x, 2) for x in t_asm], "numeric_ms": [round(x, 2) for x in t_num],
                   "symbolic_ms": [round(x - min(t_num), 2) for x in t_asm],
                   "peak_bytes_above_output": int(peak - out_bytes), "output_bytes": int(out_bytes),
                   "numeric_hbm_bound_ms": round(bound_ms, 3), "numeric_fraction_of_bound": round(bound_ms / min(t_num), 3)}
            if not a.no_setup:
                params = capi.default_params(num_coarsenings=c["nc"], theta=0.003, nu_relax=3)
                rp, cp, vp, _ = op.arrays()
                mk = capi._DevicePointer

                def setup():
                    h = capi.Hierarchy(mk(rp, "int64"), mk(cp, "int32"), mk(vp, "float64"), c["n"], c["e2d"], c["elmat"], c["bdr"],
                                       c["parts"], c["nparts"], params, c["NE"], c["nde"], stream=stream(), elem_ptr=c["eptr"])
                    torch.cuda.synchronize()
                    h.close()
                timed(setup)
                rec["setup_ms"] = [round(timed(setup)[0], 2) for _ in range(a.reps)]
            op.close()
            print(json.dumps(rec), flush=True)
        except (RuntimeError, MemoryError) as e:
            print(json.dumps({"case": name, "skipped": str(e)[:200]}), flush=True)
        c = None
        torch.cuda.empty_cache()
        capi.release_cached_memory()


if __name__ == "__main__":
    main()
