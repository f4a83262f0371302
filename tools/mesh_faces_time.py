"""Times the face table on the device (saamge_amd_face_table_build) and the essential-dof flags of all boundary faces
(saamge_amd_face_dofs) on meshes built on the device: Q1 hex grids, their Kuhn split into tetrahedra, the half-prism mesh of
poisson3d_mixed_problem and 27-node hexes.  Host clock closed by a synchronise, one warm-up, `--reps` repetitions (all listed).
Prints one JSON line per case.

    python tools/mesh_faces_time.py [--hex 128,256] [--tets 64] [--mixed 64] [--hex27 64] [--reps 3] [--host 128]

Beside each time, measured in the same run: graph_ms of the partitioner's element graph on the same mesh with min_shared = the
node count of the type's faces, computed the way tools/partition_time.py computes it (partition_mesh with one coarsening minus
the level-0 partition timed alone; it includes the quotient graph of level 0).  --host N: the host time of the numpy routine
problems.boundary_faces on the hex grid N^3, printed last as a line of its own (the routine needs tens of GB at 256^3)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPA = 256
KUHN = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)]


def hex_device(n):
    """(elem_to_vertex (NE, 8) int32, NV) of the n^3 grid, on the GPU"""
    import torch
    nv = n + 1
    e = torch.arange(n * n * n, device="cuda", dtype=torch.int64)
    ex, ey, ez = e % n, (e // n) % n, e // (n * n)
    v0 = (ez * nv + ey) * nv + ex
    offs = [0, 1, nv + 1, nv, nv * nv, nv * nv + 1, nv * nv + nv + 1, nv * nv + nv]
    return torch.stack([v0 + o for o in offs], dim=1).to(torch.int32).contiguous(), nv ** 3


def tets_device(n):
    """problems.hex_to_tets(n) on the GPU: (6 n^3, 4) int32"""
    import torch
    nv = n + 1
    e = torch.arange(n * n * n, device="cuda", dtype=torch.int64)
    base = torch.stack([e % n, (e // n) % n, e // (n * n)], dim=1)
    vid = lambda p: (p[:, 2] * nv + p[:, 1]) * nv + p[:, 0]
    tets = []
    for k, perm in enumerate(KUHN):
        corner = torch.zeros(3, dtype=torch.int64, device="cuda")
        v = [vid(base)]
        for axis in perm:
            corner[axis] = 1
            v.append(vid(base + corner[None, :]))
        if k >= 3:
            v[2], v[3] = v[3], v[2]
        tets.append(torch.stack(v, dim=1))
    return torch.stack(tets, dim=1).reshape(-1, 4).to(torch.int32).contiguous(), nv ** 3


def hex27_device(n):
    """problems.q2_hex_nodes((n, n, n)) on the GPU: (n^3, 27) int32, lexicographic nodes of the (2 n + 1)^3 grid"""
    import torch
    nv = 2 * n + 1
    e = torch.arange(n * n * n, device="cuda", dtype=torch.int64)
    ex, ey, ez = e % n, (e // n) % n, e // (n * n)
    cols = [((2 * ez + iz) * nv + 2 * ey + iy) * nv + 2 * ex + ix for iz in range(3) for iy in range(3) for ix in range(3)]
    return torch.stack(cols, dim=1).to(torch.int32).contiguous(), nv ** 3


def main():
    import torch
    from saamge_amd import capi, problems

    ap = argparse.ArgumentParser()
    ap.add_argument("--hex", default="128,256")
    ap.add_argument("--tets", default="64")
    ap.add_argument("--mixed", default="64")
    ap.add_argument("--hex27", default="64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host", default="128")
    a = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",") if x]
    cases = []      # (name, dim, elem_to_vertex, elem_ptr, NV, min_shared)
    for n in ints(a.hex):
        cases.append(("hex%d" % n, 3) + hex_device(n)[:1] + (None, (n + 1) ** 3, 4))
    for n in ints(a.tets):
        cases.append(("tets%d" % n, 3) + tets_device(n)[:1] + (None, (n + 1) ** 3, 3))
    for n in ints(a.mixed):
        mp = problems.poisson3d_mixed_problem(n, (2, 2, 2), wedges="half")
        dev = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32)).cuda()
        cases.append(("mixed%d" % n, 3, dev(mp.elem_to_dof), dev(mp.elem_ptr), mp.ND, 3))
    for n in ints(a.hex27):
        cases.append(("hex27_%d" % n, 3) + hex27_device(n)[:1] + (None, (2 * n + 1) ** 3, 9))

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), r

    r = lambda v: [round(x, 2) for x in v]
    for name, dim, e2v, eptr, NV, ms in cases:
        build = lambda: capi.FaceTable(NV, dim, e2v, elem_ptr=eptr)
        _, T = timed(build)                          # warm-up
        info, NB = T.info, T.NB
        flags = torch.zeros(NV, dtype=torch.int8, device="cuda")
        dofs = lambda: capi.face_dofs(NV, dim, e2v, T.pointer("bdr_elem"), T.pointer("bdr_local"), flags, elem_ptr=eptr)
        timed(dofs)
        t_dofs = [timed(dofs)[0] for _ in range(a.reps)]
        dofs_info = dofs()
        T.free()
        t_build = []
        capi.memory_stats(reset_peak=True)
        for _ in range(a.reps):
            t, T = timed(build)
            t_build.append(t)
            peak = capi.memory_stats()[1]
            T.free()
        # the yardstick: the partitioner's element graph, as tools/partition_time.py times it
        mesh1 = lambda: capi.partition_mesh(e2v, NV, [EPA], elem_ptr=eptr, min_shared=ms)
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
        print(json.dumps({
            "case": name, "elements": n0, "vertices": NV, "info": info, "boundary_faces": NB, "face_table_build_ms": r(t_build),
            "face_dofs_ms": r(t_dofs), "face_dofs_info": dofs_info, "peak_device_bytes": int(peak), "min_shared": ms,
            "partitioner_graph_entries": int(g0[1].numel()), "partitioner_graph_ms": r([m - l for m, l in zip(t_mesh, t0)])}),
            flush=True)
        del g0, d0, flags
    for n in ints(a.host):
        e2v = hex_device(n)[0].cpu().numpy()
        t = time.perf_counter()
        fe, _ = problems.boundary_faces(3, e2v)
        print(json.dumps({"case": "hex%d_host_boundary_faces" % n, "boundary_faces": int(len(fe)),
                          "host_ms": round(1e3 * (time.perf_counter() - t), 1)}), flush=True)


if __name__ == "__main__":
    main()
