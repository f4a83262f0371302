"""Times the uniform refinement of an order-1 mesh on the device (saamge_amd_mesh_refine), the whole call with coordinates, with
and without the interpolations, on meshes built on the device.  Each target is a size the lift was measured at
(tools/mesh_lift_time.py): Q1 hexahedra 64^3 -> 128^3 (one level) and -> 256^3 (two levels), the Kuhn tetrahedra of 32^3 -> the
64^3 split, quadrilaterals 1024^2 -> 2048^2.  Host clock closed by a synchronise, one warm-up, `--reps` repetitions (all
listed), the peak of the library's device bytes from saamge_amd_memory_stats.  Prints one JSON line per case.

    python tools/mesh_refine_time.py [--hex 64:1,64:2] [--tets 32:1] [--quads 1024:1] [--reps 3]

Yardsticks, in the same run: saamge_amd_mesh_lift_order2 on the mesh of every level the call lifts (a refinement step contains
that lift; `contained_lifts_ms` is their sum) and saamge_amd_face_table_build on the refined mesh.  `beyond_lift_ms` is the
call without interpolations minus the contained lifts: the children kernels and the hand-over between levels;
`interp_ms` the call with interpolations minus the call without.  The bounds are the bytes the children kernel (the child
lists and offsets written, the lifted node lists and their offsets read) and the interpolation kernel (rowptr, col and val
written) have to move, at COPY_TBPS -- the copy rate measured on the card, not the 8 TB/s of its data sheet."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mesh_faces_time import hex_device, tets_device      # noqa: E402
from mesh_lift_time import grid_coords_device, quads_device      # noqa: E402

COPY_TBPS = 6.29


def main():
    import torch
    from saamge_amd import capi

    ap = argparse.ArgumentParser()
    ap.add_argument("--hex", default="64:1,64:2")
    ap.add_argument("--tets", default="32:1")
    ap.add_argument("--quads", default="1024:1")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    pairs = lambda s: [tuple(int(v) for v in x.split(":")) for x in s.split(",") if x]
    cases = []      # (name, dim, n, levels, elem_to_vertex, NV)
    for n, lv in pairs(a.hex):
        cases.append(("hex%d_x%d" % (n, lv), 3, n, lv) + hex_device(n))
    for n, lv in pairs(a.tets):
        cases.append(("tets%d_x%d" % (n, lv), 3, n, lv) + tets_device(n))
    for n, lv in pairs(a.quads):
        cases.append(("quads%d_x%d" % (n, lv), 2, n, lv) + quads_device(n))

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), r

    def series(fn, keep=False):
        """one warm-up, then the repetitions; every handle is freed, the last one returned with keep"""
        _, h = timed(fn)
        h.free()
        capi.memory_stats(reset_peak=True)
        ts, peak = [], 0
        for k in range(a.reps):
            t, h = timed(fn)
            ts.append(t)
            peak = capi.memory_stats()[1]
            if not (keep and k == a.reps - 1):
                h.free()
        return ts, int(peak), h

    r = lambda v: [round(x, 2) for x in v]
    for name, dim, n, levels, e2v, NV in cases:
        X = grid_coords_device(n, dim)
        nd = int(e2v.shape[1])
        t_plain, peak_plain, R = series(lambda: capi.MeshRefine(X, e2v, levels=levels), keep=True)
        t_interp, peak_interp, _ = series(lambda: capi.MeshRefine(X, e2v, levels=levels, want_interp=True))
        info = R.info
        counts = [R.level_info(j) for j in range(levels + 1)]
        # the face table of the refined mesh
        rows = R.pointer("elem_to_vertex", shape=(R.NE, nd))
        t_faces, _, _ = series(lambda: capi.FaceTable(R.NV, dim, rows))
        R.free()
        # the lift of every level the call lifts: level 0 is the input, the later ones come from a shorter refinement
        t_lifts = []
        for j in range(levels):
            S = capi.MeshRefine(X, e2v, levels=j) if j else None
            Xj = S.pointer("coords") if S else X
            ej = S.pointer("elem_to_vertex", shape=(S.NE, nd)) if S else e2v
            t_lifts.append(series(lambda: capi.MeshLift(Xj, ej))[0])
            if S:
                S.free()
        contained = [sum(t[k] for t in t_lifts) for k in range(a.reps)]
        nc = 4 if dim == 2 else 8
        lifted_nd = {(2, 3): 6, (2, 4): 9, (3, 4): 10, (3, 8): 27}[(dim, nd)]
        child_bytes = sum(4 * (nc * c[2] + nc * c[1] + 1) + 4 * (lifted_nd * c[1] + c[1] + 1) for c in counts[:-1])
        nnz = [c[0] + 2 * c[3] + 4 * c[4] + (4 if dim == 2 else 8) * c[5] for c in counts[:-1]]
        interp_bytes = sum(4 * (counts[j + 1][0] + 1) + 12 * nnz[j] for j in range(levels))
        line = {"case": name, "levels": levels, "elements": int(e2v.shape[0]), "vertices": NV, "info": info,
                "level_counts": counts, "mesh_refine_ms": r(t_plain), "mesh_refine_interp_ms": r(t_interp),
                "mesh_lift_ms_per_level": [r(t) for t in t_lifts], "contained_lifts_ms": r(contained),
                "beyond_lift_ms": r([p - c for p, c in zip(t_plain, contained)]),
                "interp_ms": r([i - p for i, p in zip(t_interp, t_plain)]),
                "children_bound_ms": round(child_bytes / (COPY_TBPS * 1e9), 3),
                "interp_bound_ms": round(interp_bytes / (COPY_TBPS * 1e9), 3),
                "face_table_build_refined_ms": r(t_faces), "peak_device_bytes": peak_plain,
                "peak_device_bytes_interp": peak_interp}
        print(json.dumps(line), flush=True)
        del X


if __name__ == "__main__":
    main()
