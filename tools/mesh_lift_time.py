"""Times the lift of an order-1 mesh to order 2 on the device (saamge_amd_mesh_lift_order2), the whole call with coordinates and
with the face table built inside, on meshes built on the device: Q1 hex grids, the Kuhn tetrahedra of a grid, a quadrilateral
grid.  Host clock closed by a synchronise, one warm-up, `--reps` repetitions (all listed).  Prints one JSON line per case.

    python tools/mesh_lift_time.py [--hex 128,256] [--tets 64] [--quads 2048] [--reps 3] [--host-tets 64]

Beside each lift, measured in the same run on the same mesh: face_table_build (the lift of a mesh with hexahedra contains one),
the lift with that table handed in, and graph_ms of the partitioner's element graph with min_shared = the node count of the
type's faces, computed the way tools/mesh_faces_time.py computes it; and the peak of the library's device bytes during a lift.
--host-tets N: the host time of problems.p2_simplex_nodes on the Kuhn tetrahedra of N^3, once, in the line of that case."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mesh_faces_time import EPA, hex_device, tets_device      # noqa: E402


def quads_device(n):
    """(elem_to_vertex (n^2, 4) int32, NV) of the n x n grid of counter-clockwise quadrilaterals, on the GPU"""
    import torch
    nv = n + 1
    e = torch.arange(n * n, device="cuda", dtype=torch.int64)
    v0 = (e // n) * nv + e % n
    return torch.stack([v0, v0 + 1, v0 + nv + 1, v0 + nv], dim=1).to(torch.int32).contiguous(), nv * nv


def grid_coords_device(n, dim):
    import torch
    nv = n + 1
    k = torch.arange(nv ** dim, device="cuda", dtype=torch.int64)
    cols = [((k // nv ** d) % nv).to(torch.float64) / n for d in range(dim)]
    return torch.stack(cols, dim=1).contiguous()


def main():
    import torch
    from saamge_amd import capi, problems

    ap = argparse.ArgumentParser()
    ap.add_argument("--hex", default="128,256")
    ap.add_argument("--tets", default="64")
    ap.add_argument("--quads", default="2048")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-tets", default="64")
    a = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",") if x]
    cases = []      # (name, dim, n, elem_to_vertex, NV, min_shared)
    for n in ints(a.hex):
        cases.append(("hex%d" % n, 3, n) + hex_device(n) + (4,))
    for n in ints(a.tets):
        cases.append(("tets%d" % n, 3, n) + tets_device(n) + (3,))
    for n in ints(a.quads):
        cases.append(("quads%d" % n, 2, n) + quads_device(n) + (2,))

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), r

    r = lambda v: [round(x, 2) for x in v]
    for name, dim, n, e2v, NV, ms in cases:
        X = grid_coords_device(n, dim)
        lift = lambda faces=None: capi.MeshLift(X, e2v, faces=faces)
        _, L = timed(lift)                           # warm-up
        info = L.info
        L.free()
        t_lift = []
        capi.memory_stats(reset_peak=True)
        for _ in range(a.reps):
            t, L = timed(lift)
            t_lift.append(t)
            peak = capi.memory_stats()[1]
            L.free()
        build = lambda: capi.FaceTable(NV, dim, e2v)
        _, T = timed(build)
        T.free()
        t_build, t_given = [], []
        for _ in range(a.reps):
            t, T = timed(build)
            t_build.append(t)
            t, L = timed(lambda: lift(T))
            t_given.append(t)
            L.free()
            T.free()
        # the yardstick: the partitioner's element graph, as tools/mesh_faces_time.py times it
        mesh1 = lambda: capi.partition_mesh(e2v, NV, [EPA], min_shared=ms)
        _, P = timed(mesh1)
        g0 = P.graph(0, device=True)
        n0 = P.n_elem[0]
        P.close()
        d0 = torch.empty(n0, dtype=torch.int32, device="cuda")
        lev0 = lambda: capi.partition_graph(n0, g0[0], g0[1], EPA, part=d0)[1]
        timed(lev0)
        t_mesh, t0 = [], []
        for _ in range(a.reps):
            t, P = timed(mesh1)
            P.close()
            t_mesh.append(t)
            t0.append(timed(lev0)[0])
        line = {"case": name, "elements": n0, "vertices": NV, "info": info, "mesh_lift_ms": r(t_lift),
                "face_table_build_ms": r(t_build), "mesh_lift_given_faces_ms": r(t_given), "peak_device_bytes": int(peak),
                "min_shared": ms, "partitioner_graph_ms": r([m - l for m, l in zip(t_mesh, t0)])}
        if name.startswith("tets") and n in ints(a.host_tets):
            hX, hv = X.cpu().numpy(), e2v.cpu().numpy()
            t = time.perf_counter()
            X2, _ = problems.p2_simplex_nodes(hX, hv)
            line["host_p2_simplex_nodes_ms"] = round(1e3 * (time.perf_counter() - t), 1)
            assert X2.shape[0] == info[0]
        print(json.dumps(line), flush=True)
        del g0, d0, X


if __name__ == "__main__":
    main()
