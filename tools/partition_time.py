"""Times the device partitioner: element graph, level-0 and level-1 partition, peak device memory and the size distribution
of the parts, on Q1 hex grids (vertex and face adjacency) and on the half-prism mesh of poisson3d_mixed_problem.  Host
clock closed by a synchronise, one warm-up, `--reps` repetitions (all listed).  Prints one JSON line per case.

    python tools/partition_time.py [--hex 128,256] [--mixed 64] [--epa 256,64] [--reps 3] [--seeding {0,1}] [--growth {0,1}]
                                   [--refine R]

--seeding 1 times the spaced seeding; the line then carries, per level, the radius chosen, the independent-set rounds and
the seeds before and after the top-up (saamge_amd_partition_seeding_info; zeros for --seeding 0).  --growth 1 times the
balanced growth; the line carries the mode and, per level, the balanced rounds, the nodes labelled under a quota, the parts
open at the release and the nodes labelled after it (saamge_amd_partition_growth_info; zeros for --growth 0).

--refine R (default 0: off) times the boundary refinement pass with at most R rounds on the partition of each level as the
other options made it (saamge_amd_partition_refine with that level's caps, parts numbered again): the line then carries, per
level, the rounds that moved nodes, the nodes moved, the edge cut before and after and the time of the pass alone.  Both
levels are those of the unrefined partitions, so the lines of --refine 0 and --refine R describe the same graphs.

graph_ms is the time of partition_mesh with one coarsening minus the level-0 partition timed alone (it includes the
quotient graph of level 0).  For the hex grids, box_setup_ms is the time of a 3-level hierarchy setup of the Poisson problem
on the same grid with box partitions (8 x 8 x 4, twice), timed the same way and printed last: what the partitioner's
time stands next to.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def hex_e2d_device(n):
    import torch
    nv = n + 1
    e = torch.arange(n * n * n, device="cuda", dtype=torch.int64)
    ex, ey, ez = e % n, (e // n) % n, e // (n * n)
    v0 = (ez * nv + ey) * nv + ex
    offs = [0, 1, nv + 1, nv, nv * nv, nv * nv + 1, nv * nv + nv + 1, nv * nv + nv]
    return torch.stack([v0 + o for o in offs], dim=1).to(torch.int32).contiguous(), nv ** 3


def main():
    import torch
    from saamge_amd import capi, problems, partition_model as pm

    ap = argparse.ArgumentParser()
    ap.add_argument("--hex", default="128,256")
    ap.add_argument("--mixed", default="64")
    ap.add_argument("--epa", default="256,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seeding", type=int, choices=(0, 1), default=0)
    ap.add_argument("--growth", type=int, choices=(0, 1), default=0)
    ap.add_argument("--refine", type=int, default=0)
    a = ap.parse_args()
    epa = [int(x) for x in a.epa.split(",")]
    cases = []
    for n in [int(x) for x in a.hex.split(",") if x]:
        e2d, ND = hex_e2d_device(n)
        cases += [("hex%d_vertex" % n, e2d, None, ND, 1), ("hex%d_face" % n, e2d, None, ND, 4)]
    for n in [int(x) for x in a.mixed.split(",") if x]:
        mp = problems.poisson3d_mixed_problem(n, (2, 2, 2), wedges="half")
        dev = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32)).cuda()
        cases.append(("mixed%d_vertex" % n, dev(mp.elem_to_dof), dev(mp.elem_ptr), mp.ND, 1))

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), r

    def box_setup_ms(n):
        hexp = problems.poisson3d_device(n, blk=(8, 8, 4), coarse_blk=[(8, 8, 4)], device="cuda")
        def setup():
            params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3)
            h = capi.Hierarchy(hexp.rowptr, hexp.col, hexp.val, hexp.n, hexp.elem_to_dof, hexp.elmat, hexp.bdr,
                               hexp.partitions, hexp.nparts, params, hexp.NE_, 8,
                               stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            h.close()
        timed(setup)
        return [round(timed(setup)[0], 2) for _ in range(a.reps)]

    def edge_cut(g, part):
        xadj, adj = g
        src = torch.repeat_interleave(torch.arange(part.numel(), device="cuda"), xadj[1:] - xadj[:-1])
        return int((part[src] != part[adj.long()]).sum().item()) // 2

    def refine_level(n, g, part, nparts, e):
        """The pass on a copy of `part`, one warm-up: rounds, nodes moved, cut before and after, the times."""
        max_size, min_size = pm.resolve_sizes(e)
        out = dict(cut_before=edge_cut(g, part))
        ms_ = []
        for _ in range(a.reps + 1):
            work = part.clone()
            t, (_, info) = timed(lambda: capi.partition_refine(n, g[0], g[1], nparts, work, a.refine, max_size, min_size,
                                                               renumber=True))
            ms_.append(round(t, 2))
        out.update(rounds=info["rounds"], moved=info["moved"], converged=info["converged"], cut_after=edge_cut(g, work),
                   refine_ms=ms_[1:])
        assert out["cut_before"] - out["cut_after"] == info["gain"]
        return out

    for name, e2d, eptr, ND, ms in cases:
        mesh1 = lambda: capi.partition_mesh(e2d, ND, epa[:1], elem_ptr=eptr, min_shared=ms, seeding=a.seeding, growth=a.growth)
        _, P = timed(mesh1)                         # warm-up; its graphs feed the per-level timings
        g0, g1 = P.graph(0, device=True), P.graph(1, device=True)
        n0, n1 = P.n_elem[0], P.nparts[0]
        part0 = P.part(0)
        P.close()
        d0 = torch.empty(n0, dtype=torch.int32, device="cuda")
        d1 = torch.empty(n1, dtype=torch.int32, device="cuda")
        lev0 = lambda: capi.partition_graph(n0, g0[0], g0[1], epa[0], part=d0, seeding=a.seeding, growth=a.growth)[1]
        lev1 = lambda: capi.partition_graph(n1, g1[0], g1[1], epa[1], part=d1, seeding=a.seeding, growth=a.growth)[1]
        timed(lev0), timed(lev1)
        t_mesh, t0, t1 = [], [], []
        capi.memory_stats(reset_peak=True)
        for _ in range(a.reps):
            t, P = timed(mesh1)
            P.close()
            t_mesh.append(t)
            t0.append(timed(lev0)[0])
            info0 = capi.partition_seeding_info()
            ginfo0 = capi.partition_growth_info()
            t, np1 = timed(lev1)
            info1 = capi.partition_seeding_info()
            ginfo1 = capi.partition_growth_info()
            t1.append(t)
        peak = capi.memory_stats()[1]
        r = lambda v: [round(x, 2) for x in v]
        extra = {}
        if a.refine > 0:
            timed(lev0)
            extra = {"refine": a.refine, "refine_level0": refine_level(n0, g0, d0, n1, epa[0]),
                     "refine_level1": refine_level(n1, g1, d1, int(np1), epa[1])}
        print(json.dumps(dict({
            "case": name, "seeding": a.seeding, "seeding_level0": info0, "seeding_level1": info1,
            "growth": a.growth, "growth_level0": ginfo0, "growth_level1": ginfo1, "elements": n0, "graph_entries": int(g0[1].numel()), "elems_per_agg": epa,
            "nparts": [n1, int(np1)], "mesh_one_level_ms": r(t_mesh), "level0_ms": r(t0), "level1_ms": r(t1),
            "graph_ms": r([m - l for m, l in zip(t_mesh, t0)]), "peak_device_bytes": int(peak),
            "size_over_epa_level0": pm.size_stats(part0, n1, epa[0]),
            "size_over_epa_level1": pm.size_stats(d1.cpu().numpy(), int(np1), epa[1])}, **extra)), flush=True)
        del g0, g1, d0, d1
    # last, so that the hierarchies do not enter the partitioner's peak memory
    for n in [int(x) for x in a.hex.split(",") if x]:
        print(json.dumps({"case": "hex%d_box_setup" % n, "box_setup_ms": box_setup_ms(n)}), flush=True)


if __name__ == "__main__":
    main()
