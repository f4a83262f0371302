#!/usr/bin/env python
"""Time of the eigensolver (Hierarchy.lobpcg) on the benchmark's operators, and where an iteration goes.

Workloads:
    poisson128        3-D Poisson 128^3 Q1 (BASELINE config 2, two levels), nev = nb = 8, tol = 1e-8, M = I
    poisson128_mass   the same with the Q1 mass assembled on the device (element_mass, then Operator)
    elasticity_q2_32  3-D elasticity, Q2 hexes at 32^3 (three levels), nev = 6, nb = 8, M = I

Protocol: one warm-up solve, `--reps` timed ones (all listed), a host clock closed by a synchronise.  One more solve runs
under the library's kernel profile (every kernel then ends in an event wait, so that run is not timed) and gives the split
into V-cycles, operator products (A and M), Gram products, combinations and residuals.  Each block kernel is listed beside
the larger of two bounds: its bytes -- computed here from the shapes -- over the copy rate DESIGN.md section 4.15 measured
(6.29 TB/s), and its flops over the fp64 peak of the matrix cores (78.6 TFLOP/s).

    python tools/lobpcg_time.py [--workload NAME ...] [--reps 3] [--no-profile] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
FP64_PEAK = 78.6e12
TOL = 1e-8


def build(name, capi, problems, torch):
    """-> (hierarchy, n, M as three device addresses or None, nev, nb, things to keep alive)"""
    if name.startswith("poisson128"):
        prob = problems.poisson3d_device(128, blk=(8, 8, 4), coarse_blk=[], device="cuda")
        params = capi.default_params(num_coarsenings=1, theta=0.003, nu_relax=3)
        nev, nb, nde = 8, 8, 8
    else:
        prob = problems.elasticity3d_q2_device(32, blk=(4, 4, 4), coarse_blk=[(2, 2, 2)], device="cuda")
        params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3)
        nev, nb, nde = 6, 8, 81
    h = capi.Hierarchy(prob.rowptr, prob.col, prob.val, prob.n, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions,
                       prob.nparts, params, prob.NE_, getattr(prob, "nde_", nde), stream=torch.cuda.current_stream().cuda_stream)
    M, keep = None, [prob]
    if name == "poisson128_mass":
        coords = torch.as_tensor(problems.grid_coords(128)).cuda()
        mass = capi.element_mass(coords, prob.elem_to_dof, torch.ones(prob.NE_, dtype=torch.float64, device="cuda"), device=True)
        op = capi.Operator(prob.n, prob.elem_to_dof, mass, prob.bdr, nde=8, NE=prob.NE_)
        rp, cp, vp, _ = op.arrays()
        M, keep = (rp, cp, vp), keep + [op, mass, coords]
    return h, int(prob.n), M, nev, nb, keep


def block_bounds(n, nb, with_mass):
    """per launch: kernel -> (bytes, flops) from the shapes: the buffers are 3 nb columns wide, the combination writes 2 nb"""
    w = 3 * nb
    blocks = 3 if with_mass else 2
    gram_full = (8.0 * n * 2 * w, 2.0 * n * w * w)
    gram_sym = (8.0 * n * w, 1.0 * n * w * (w + 1))
    # two Gram products per iteration: S^T (A S) always full, S^T (M S) full with a mass and symmetric (T == S) without
    second = gram_full if with_mass else gram_sym
    return {"bv_gram": (0.5 * (gram_full[0] + second[0]), 0.5 * (gram_full[1] + second[1])),
            "bv_combine": (8.0 * n * blocks * (w + 2 * nb), 2.0 * n * blocks * w * 2 * nb),
            "bv_residual": (8.0 * n * nb * 3, 6.0 * n * nb)}


def run(name, reps, profile, out):
    import torch
    from saamge_amd import capi, problems
    h, n, M, nev, nb, keep = build(name, capi, problems, torch)

    def solve():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = h.lobpcg(nev, nb, M=M, tol=TOL, max_iter=200, seed=1)
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0
    (lam, X, res, iters, conv, hist), warm = solve()
    times = [solve()[1] for _ in range(reps)]
    out("== %s: n = %d, nev = %d, nb = %d, M = %s" % (name, n, nev, nb, "Q1 mass (device)" if M else "I"))
    out("   iterations %d, converged %d, lambda_1 = %.6e, lambda_nev = %.6e, max rho = %.2e" % (iters, conv, lam[0], lam[-1], res.max()))
    out("   warm-up %.1f ms; timed: %s ms" % (1e3 * warm, ", ".join("%.1f" % (1e3 * t) for t in times)))
    best = min(times)
    out("   best %.1f ms = %.2f ms per iteration (%d iterations + the start)" % (1e3 * best, 1e3 * best / (iters + 1), iters))
    if profile:
        capi.profile(True)
        capi.profile_reset()
        h.lobpcg(nev, nb, M=M, tol=TOL, max_iter=200, seed=1)
        stats = capi.profile_stats()
        capi.profile(False)
        capi.profile_reset()
        groups = {"V-cycles": 0.0, "A / M products": 0.0, "bv_gram": 0.0, "bv_combine": 0.0, "bv_residual": 0.0}
        per = {}
        for k in stats:
            key = k["name"] if k["name"] in groups else ("A / M products" if k["name"] == "spmv@%d" % n else "V-cycles")
            groups[key] += k["ms"]
            per[k["name"]] = k
        total = sum(groups.values())
        out("   kernel profile of one solve (sum of kernel times %.1f ms):" % total)
        for key, ms in groups.items():
            out("     %-16s %9.2f ms  %5.1f %%" % (key, ms, 100.0 * ms / total))
        algebra = groups["bv_gram"] + groups["bv_combine"] + groups["bv_residual"]
        out("     block algebra %.1f %% of the kernel time, V-cycles %.1f %%" % (100 * algebra / total, 100 * groups["V-cycles"] / total))
        out("   block kernels per launch against max(bytes / 6.29 TB/s, flops / 78.6 TFLOP/s):")
        for kname, (by, fl) in block_bounds(n, nb, M is not None).items():
            k = per[kname]
            t = 1e-3 * k["ms"] / k["launches"]
            tb, tf = by / COPY_RATE, fl / FP64_PEAK
            out("     %-12s %5d launches  %8.1f us   bound %7.1f us (%s: %.0f MB, %.2f GFLOP)   x %.2f of the bound"
                % (kname, k["launches"], 1e6 * t, 1e6 * max(tb, tf), "bytes" if tb >= tf else "flops", by / 1e6, fl / 1e9,
                   t / max(tb, tf)))
    h.close()
    del keep


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", action="append", choices=["poisson128", "poisson128_mass", "elasticity_q2_32"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None

    def out(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    for name in args.workload or ["poisson128", "poisson128_mass", "elasticity_q2_32"]:
        run(name, args.reps, not args.no_profile, out)


if __name__ == "__main__":
    main()
