#!/usr/bin/env python
"""One block V-cycle on k columns (Hierarchy.vcycle_block) against k single V-cycles (Hierarchy.vcycle), per column.

Workloads:
    poisson128        3-D Poisson 128^3 Q1, constant coefficient, two levels: pair-coded fine level (1 B per entry)
    poisson128_skew   the same grid with coef="skew": offset-coded fine level (9 B per entry)
    elasticity_q2_32  3-D elasticity, Q2 hexes at 32^3, three levels: the operator-level dictionary on the fine level

Protocol: all vectors live on the device; for k = 1, 2, 4, 8 one warm-up, then `--cycles` block V-cycles and `--cycles` x k
single ones, each series under a host clock closed by a synchronise; `--reps` repetitions, all listed.  Beside each: the
bytes one block cycle must move -- the matrix data of every level once (Sell::stream_bytes, pre- and post-smoother steps
and the residual each stream it; P and R as CSR, 12 B per entry) plus the vectors k times -- over the copy rate DESIGN.md
section 4.15 measured (6.29 TB/s).  The block results are compared with the single ones bit for bit before anything is timed.

    python tools/vcycle_block_time.py [--workload NAME ...] [--ks 1 2 4 8] [--cycles 20] [--reps 3] [--out FILE]
    python tools/vcycle_block_time.py --workload NAME --trace-k 8      (only k block cycles: for a kernel trace of its own)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
WORKLOADS = ["poisson128", "poisson128_skew", "elasticity_q2_32"]


def build(name, capi, problems, torch):
    if name.startswith("poisson128"):
        prob = problems.poisson3d_device(128, blk=(8, 8, 4), coarse_blk=[], device="cuda", coef="skew" if name.endswith("skew") else None)
        params = capi.default_params(num_coarsenings=1, theta=0.003, nu_relax=3)
        nde = 8
    else:
        prob = problems.elasticity3d_q2_device(32, blk=(4, 4, 4), coarse_blk=[(2, 2, 2)], device="cuda")
        params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3)
        nde = 81
    h = capi.Hierarchy(prob.rowptr, prob.col, prob.val, prob.n, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions,
                       prob.nparts, params, prob.NE_, getattr(prob, "nde_", nde), stream=torch.cuda.current_stream().cuda_stream)
    return h, int(prob.n), prob


def cycle_bytes(h, k, nu=3):
    """bytes one block V-cycle on k columns must move: per level the operator's stream 2 (3 nu + 1) times (the steps of both
    smoothers but the first of the pre-smoother, and the residual), P and R once each, and per application the vectors it
    reads and writes, k times"""
    deg = 3 * nu + 1
    matrix = vectors = 0.0
    for lev in range(h.num_levels - 1):
        info, fmt = h.level_info(lev), h.level_format(lev)
        n, nc = info["n"], info["ncoarse"]
        apps = 2 * deg
        matrix += apps * float(fmt["stream_bytes"]) + 2 * 12.0 * info["nnzP"]
        # smoother step: x in, b in, x out; residual: x, b, r; restriction: r in, rc out; prolongation: xc in, x in and out
        vectors += k * 8.0 * ((apps - 1) * 3 * n + 3 * n + (n + nc) + (nc + 2 * n))
    return matrix, vectors


def run(name, ks, cycles, reps, trace_k, out):
    import torch
    from saamge_amd import capi, problems
    h, n, prob = build(name, capi, problems, torch)
    kmax = max(list(ks) + [trace_k or 0])
    g = torch.Generator(device="cuda").manual_seed(7)
    B = torch.randn((kmax, n), dtype=torch.float64, device="cuda", generator=g)
    X = torch.zeros((kmax, n), dtype=torch.float64, device="cuda")
    Xs = torch.zeros((kmax, n), dtype=torch.float64, device="cuda")

    def block(k):
        h.vcycle_block(B.data_ptr(), X.data_ptr(), k=k, ldb=n, ldx=n)

    def singles(k):
        for j in range(k):
            h.vcycle(B[j].data_ptr(), Xs[j].data_ptr())
    if trace_k:
        block(trace_k)
        torch.cuda.synchronize()
        for _ in range(cycles):
            block(trace_k)
        torch.cuda.synchronize()
        h.close()
        return
    fmt = h.level_format(0)
    out("== %s: n = %d, levels %d, fine level entries pair/offset/plain %s, dictionary pairs %d" %
        (name, n, h.num_levels, "/".join(str(fmt["entries"][c]) for c in ("pair_coded", "offset_coded", "plain")), fmt["dictionary_pairs"]))

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(cycles):
            fn(k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / cycles
    for k in ks:
        block(k)
        singles(k)
        torch.cuda.synchronize()
        assert torch.equal(X[:k], Xs[:k]), "block and single V-cycles differ"
        tb = [timed(block, k) for _ in range(reps)]
        ts = [timed(singles, k) for _ in range(reps)]
        matrix, vectors = cycle_bytes(h, k)
        bound = (matrix + vectors) / COPY_RATE
        out("   k = %d  per column: block %s us (best %.1f)   single %s us (best %.1f)   block / single %.2f" %
            (k, ", ".join("%.1f" % (1e6 * t / k) for t in tb), 1e6 * min(tb) / k, ", ".join("%.1f" % (1e6 * t / k) for t in ts),
             1e6 * min(ts) / k, min(tb) / min(ts)))
        out("          bytes of one block cycle: matrix %.1f MB + vectors %.1f MB = %.1f us at 6.29 TB/s (%.1f us per column); block cycle x %.2f of it"
            % (matrix / 1e6, vectors / 1e6, 1e6 * bound, 1e6 * bound / k, min(tb) / bound))
    h.close()
    del prob


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", action="append", choices=WORKLOADS)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace-k", type=int, default=0)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None

    def out(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    for name in args.workload or WORKLOADS:
        run(name, args.ks, args.cycles, args.reps, args.trace_k, out)


if __name__ == "__main__":
    main()
