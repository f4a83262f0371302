"""Times the element matrices computed on the device (saamge_amd_element_matrices) on device inputs: Q1 diffusion on n^3
hexes with a scalar coefficient per element and Q1 hex elasticity, against their HBM lower bound (the output written once
at --hbm-gbs; the inputs, listed as input_bytes, add 13 % for diffusion and 2 % for elasticity and are not in the bound),
beside the path this replaces: the element matrices generated on the host as problems.py does (one closed-form box matrix
scaled per element) and uploaded.  Host clock closed by a synchronise, one
warm-up, `--reps` repetitions (all listed).  One JSON line per case.

    python tools/elmat_time.py [--hex 128,256] [--elasticity 64] [--q2-hex 64,128] [--q2-elasticity 32,64] [--quad9 2048]
                               [--reps 3] [--host-reps 3] [--hbm-gbs 8000] [--fp64-gops 39300] [--no-host] [--no-mass]
                               [--rhs 256] [--boundary] [--p2-simplex] [--p2-tet 64] [--p2-tri 2048] [--points] [--point-coef]
                               [--boundary-points]

Beside every stiffness case, on the same mesh and in the same run (--no-mass: not): the mass matrices of the same layout
(saamge_amd_element_mass; vdim 1 beside diffusion, dim beside elasticity), written (`<case>:mass`) and added to the stiffness
matrices (`<case>:mass_accumulate`; its bound reads the target once and writes it once), and the load vectors of a nodal source
(`<case>:loads`; saamge_amd_element_loads), each with `stiffness_fraction_of_bound`, the yardstick.  --rhs n: the right-hand
side of Q1 diffusion on n^3 hexes assembled from its element vectors (saamge_amd_operator_assemble_rhs) against reading them
once.

--boundary: only the boundary forms (saamge_amd_boundary_mass / _loads) on ALL boundary faces of Q1 hexes 128^3 and 256^3, Q2
hexes 64^3 (vdim 1 and 3) and 9-node quadrilaterals 2048^2, same protocol (device inputs, jittered, host clock round the whole
call, one warm-up, --reps repetitions); the yardstick of a case is `element_mass` with `add_to` on the same mesh in the same run
(`mass_accumulate_ms`): the boundary call touches about 6 / n of the elements and should land below it.

--p2-simplex: only the order-2 simplices -- 10-node tetrahedra from the Kuhn split of the --p2-tet^3 grid and 6-node triangles
from the diagonal split of the --p2-tri^2 grid, their nodes the (2 n + 1)^dim half-grid with every node moved by 0.1 of the node
spacing -- under the same protocol: diffusion, elasticity, mass (vdim 1 and dim, written), loads, and the boundary mass and loads
on all boundary faces; after each, the same form on the 27-node hexes / 9-node quadrilaterals of the same grid in the same run,
the yardstick (`yardstick_fraction_of_bound`, or `yardstick_ms` for the boundary forms).

--points: only the data at quadrature points (saamge_amd_element_points, _eval with and without the gradient, _loads_points,
_errors with both columns; vdim 1) on Q1 hexes 128^3 and 256^3, Q2 hexes 64^3 and the 10-node tetrahedra of the 64^3 split, same
protocol; `bound_bytes` is what the call must move -- coordinates, vertex lists, nodal and point inputs read once, outputs
written once -- and `hbm_bound_ms` that at --hbm-gbs; after them saamge_amd_element_loads on the same mesh in the same run.

--point-coef: only the element matrices with coefficients at the points (saamge_amd_element_matrices_points: diffusion with a
symmetric tensor per point, elasticity; saamge_amd_element_mass_points written and accumulated, vdim 1) on Q1 hexes 128^3, Q2
hexes 64^3 and the 10-node tetrahedra of the 64^3 split, same protocol; directly after each, in the same run, the call it
parallels with per-element coefficients (saamge_amd_element_matrices / _mass), the yardstick.  `bound_bytes` is what the call
must move (coordinates, vertex lists and coefficients read once, the matrices written once -- read and written for
accumulate), `hbm_bound_ms` that at --hbm-gbs, `expected_extra_ms` the coefficient bytes the new call reads beyond its
yardstick at that rate, `ratio` new / yardstick (best of the repetitions) and `point_ratio` the points of the mass rule over the
points of the yardstick's rule.

--boundary-points: only the boundary data at the face points (saamge_amd_boundary_points, _eval with and without the gradient,
_mass_points, _loads_points; vdim 1) on ALL boundary faces of Q1 hexes 128^3, Q2 hexes 64^3 and the 10-node tetrahedra of the 64^3
split, same protocol; `bound_bytes` is what the call must move (face lists and offsets, the coordinates and ids of the nodes it
reads, point data read once, outputs written once, matrices and vectors read and written) and `hbm_bound_ms` that at --hbm-gbs;
beside the two forms, in the same run, the per-face call of --boundary they parallel (`per_face_call_ms`, `ratio`).  The calls
run a host clock round many small launches (one list and one or two passes per local face): the time is the call's, not a kernel's,
and that of points and eval covers the two library calls their Python wrappers make (a checks-only call for NFQ, then the call).

The vertices are jittered by 0.2 mesh widths, so no two elements are alike.  A case that does not fit is reported as skipped
with the error.

The order-2 cases (27-node hexes on n^3 elements, 9-node quadrilaterals on n^2; every node moved by 0.1 of the node spacing,
so the elements are curved) also list `ops_per_element`: the unfused floating-point operations the definition
(saamge_amd/elmat_model.py) spends on one element, counted from its formulas (arithmetic, not a measurement), and
`compute_bound_ms`, that count at --fp64-gops (the fp64 vector rate with a fused multiply-add counted once: the kernel may
not fuse).
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
    ap.add_argument("--elasticity", default="64")
    ap.add_argument("--q2-hex", default="64,128")
    ap.add_argument("--q2-elasticity", default="32,64")
    ap.add_argument("--quad9", default="2048")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=None)
    ap.add_argument("--fp64-gops", type=float, default=39300.0)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-mass", action="store_true")
    ap.add_argument("--rhs", default="")
    ap.add_argument("--boundary", action="store_true")
    ap.add_argument("--p2-simplex", action="store_true")
    ap.add_argument("--points", action="store_true")
    ap.add_argument("--point-coef", action="store_true")
    ap.add_argument("--boundary-points", action="store_true")
    ap.add_argument("--p2-tet", type=int, default=64)
    ap.add_argument("--p2-tri", type=int, default=2048)
    a = ap.parse_args()
    ints = lambda v: [int(x) for x in v.split(",") if x]
    stream = lambda: torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), r

    def mesh(n):
        """jittered grid_coords(n) and the hex vertex lists, made on the device"""
        nv = n + 1
        ax = torch.arange(nv, device=dev, dtype=torch.float64) / n
        X = torch.stack([ax.view(1, 1, -1).expand(nv, nv, nv).reshape(-1), ax.view(1, -1, 1).expand(nv, nv, nv).reshape(-1),
                         ax.view(-1, 1, 1).expand(nv, nv, nv).reshape(-1)], dim=1)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        X = (X + (2.0 * torch.rand(X.shape, generator=g, device=dev, dtype=torch.float64) - 1.0) * (0.2 / n)).contiguous()
        ez = torch.arange(n, device=dev).view(-1, 1, 1)
        ey = torch.arange(n, device=dev).view(1, -1, 1)
        ex = torch.arange(n, device=dev).view(1, 1, -1)
        e2v = torch.stack([(((ez + c) * nv + (ey + b)) * nv + (ex + a_)).reshape(-1) for (a_, b, c) in problems._HEX_LOC],
                          dim=1).to(torch.int32).contiguous()
        return X, e2v, g

    def mesh_q2(n, dim):
        """the (2 n + 1)^dim node grid with every node moved by 0.1 of the node spacing, and the node lists: the hex
        lexicographic, the quadrilateral in MFEM's H1 order"""
        gn = 2 * n + 1
        ax = torch.arange(gn, device=dev, dtype=torch.float64) / (2 * n)
        shape = (gn,) * dim
        X = torch.stack([ax.view([-1 if k == dim - 1 - d else 1 for k in range(dim)]).expand(shape).reshape(-1)
                         for d in range(dim)], dim=1)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        X = (X + (2.0 * torch.rand(X.shape, generator=g, device=dev, dtype=torch.float64) - 1.0) * (0.1 / (2 * n))).contiguous()
        if dim == 3:
            ez = torch.arange(n, device=dev).view(-1, 1, 1)
            ey = torch.arange(n, device=dev).view(1, -1, 1)
            ex = torch.arange(n, device=dev).view(1, 1, -1)
            lists = [(((2 * ez + c) * gn + (2 * ey + b)) * gn + (2 * ex + a_)).reshape(-1) for (a_, b, c) in problems.Q2_HEX_LOC]
        else:
            ey = torch.arange(n, device=dev).view(-1, 1)
            ex = torch.arange(n, device=dev).view(1, -1)
            lists = [((2 * ey + b) * gn + (2 * ex + a_)).reshape(-1) for (a_, b) in problems.Q2_QUAD_LOC]
        return X, torch.stack(lists, dim=1).to(torch.int32).contiguous(), g

    def ops_per_element(dim, nd, kind):
        """unfused operations of the definition for one element: per point the Jacobian, cofactors, determinant and the one
        division, per (point, node) G_a (and F_a), per (point, node pair a <= b) the entry's term and its addition"""
        nq, pairs, dot = nd, nd * (nd + 1) // 2, 2 * dim - 1
        point = dim * dim * (2 * nd - 1) + (33 if dim == 3 else 6)
        node = dim * dot * (1 if kind else 2)
        pair = dot + 1 + 3 * dim * dim + 3 * dim * dim + dim if kind else dot + 2
        return nq * (point + nd * node + pairs * pair)

    def grid_boundary(n, dim):
        """(face_elem, face_local) of all boundary faces of the n^dim grid (element (ez * n + ey) * n + ex), on the device; the
        local faces of elmat_model.FACE_NODES: hexahedron z = 0, y = 0, x = 1, y = 1, x = 0, z = 1; quadrilateral y = 0, x = 1,
        y = 1, x = 0"""
        idx = torch.arange(n ** dim, device=dev, dtype=torch.int32)
        ex, ey, ez = idx % n, (idx // n) % n, idx // (n * n)
        sides = [ez == 0, ey == 0, ex == n - 1, ey == n - 1, ex == 0, ez == n - 1] if dim == 3 else \
                [ey == 0, ex == n - 1, ey == n - 1, ex == 0]
        fe = torch.cat([idx[m] for m in sides])
        fl = torch.cat([torch.full((int(m.sum()),), k, device=dev, dtype=torch.int32) for k, m in enumerate(sides)])
        return fe.contiguous(), fl.contiguous()

    def mesh_p2(n, dim):
        """The order-2 simplex split of the n^dim grid on the nodes of mesh_q2 (node (z * gn + y) * gn + x of the half-grid): 6
        tetrahedra per cell (problems.hex_to_tets) or 2 triangles (problems.quads_to_tris), a midside node at the sum of its two
        vertices' grid positions.  Returns X, the node lists, the generator and the nodes' half-grid positions (NE, nodes, dim)."""
        from saamge_amd import elmat_model
        X, _, g = mesh_q2(n, dim)
        gn = 2 * n + 1
        idx = torch.arange(n ** dim, device=dev)
        base = torch.stack([idx % n, (idx // n) % n] + ([idx // (n * n)] if dim == 3 else []), dim=1)      # (cells, dim): x, y(, z)
        if dim == 3:
            corners = []
            for k, perm in enumerate(problems._KUHN):
                c, v = [0, 0, 0], [[0, 0, 0]]
                for axis in perm:
                    c[axis] = 1
                    v.append(list(c))
                if k >= 3:
                    v[2], v[3] = v[3], v[2]
                corners.append(v)
        else:
            corners = [[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]]
        corners = torch.tensor(corners, device=dev)                                    # (simplices per cell, dim + 1, dim)
        V = base[:, None, None, :] + corners[None, :, :, :]                            # (cells, per cell, dim + 1, dim)
        V = V.reshape(-1, dim + 1, dim)
        mids = [V[:, i] + V[:, j] for (i, j) in elmat_model.P2_EDGES[dim]]
        P = torch.cat([2 * V, torch.stack(mids, dim=1)], dim=1)                        # half-grid positions of all nodes
        ids = P[..., 0] + gn * P[..., 1] + (gn * gn * P[..., 2] if dim == 3 else 0)
        return X, ids.to(torch.int32).contiguous(), g, P

    def simplex_boundary(P, n, dim):
        """(face_elem, face_local) of the faces of the split whose vertices all lie on one side of the box"""
        from saamge_amd import elmat_model
        fe, fl = [], []
        ne = torch.arange(P.shape[0], device=dev, dtype=torch.int32)
        for lf, nodes in enumerate(elmat_model.FACE_NODES[(dim, P.shape[1])]):
            Q = P[:, list(nodes)]
            on = ((Q == 0).all(dim=1) | (Q == 2 * n).all(dim=1)).any(dim=1)
            fe.append(ne[on])
            fl.append(torch.full((int(on.sum()),), lf, device=dev, dtype=torch.int32))
        return torch.cat(fe).contiguous(), torch.cat(fl).contiguous()

    if a.p2_simplex:
        def reps(call):
            timed(call)                            # warm-up
            return [round(timed(call)[0], 3) for _ in range(a.reps)]
        for dim, n in ((3, a.p2_tet), (2, a.p2_tri)):
            seen = {}
            for fam in ("q2", "p2"):               # the yardstick first
                try:
                    if fam == "p2":
                        X, e2n, g, P = mesh_p2(n, dim)
                        fe, fl = simplex_boundary(P, n, dim)
                        P = None
                    else:
                        X, e2n, g = mesh_q2(n, dim)
                        fe, fl = grid_boundary(n, dim)
                    NE, nd, NF = int(e2n.shape[0]), int(e2n.shape[1]), int(fe.numel())
                    name = {27: "hex27", 9: "quad9", 10: "tet10", 6: "tri6"}[nd] + "_%d" % n
                    c1 = 0.5 + 1.5 * torch.rand(NE, generator=g, device=dev, dtype=torch.float64)
                    c2 = 0.5 + 1.5 * torch.rand((NE, 2), generator=g, device=dev, dtype=torch.float64)
                    alpha = 0.5 + 1.5 * torch.rand(NF, generator=g, device=dev, dtype=torch.float64)
                    src = torch.rand((X.shape[0], dim), generator=g, device=dev, dtype=torch.float64)
                    src1 = src[:, 0].contiguous()
                    out = torch.zeros(NE * (nd * dim) ** 2, dtype=torch.float64, device=dev)
                    vec = torch.zeros(NE * nd * dim, dtype=torch.float64, device=dev)
                    o1, v1 = out[:NE * nd * nd], vec[:NE * nd]
                    st = stream
                    forms = [("diffusion", 8 * o1.numel(), lambda: capi.element_matrices(X, e2n, 0, c1, device=True, out=o1, stream=st())),
                             ("elasticity", 8 * out.numel(), lambda: capi.element_matrices(X, e2n, 1, c2, device=True, out=out, stream=st())),
                             ("mass_vdim1", 8 * o1.numel(), lambda: capi.element_mass(X, e2n, c1, out=o1, stream=st())),
                             ("mass_vdim%d" % dim, 8 * out.numel(), lambda: capi.element_mass(X, e2n, c1, vdim=dim, out=out, stream=st())),
                             ("loads_vdim1", 8 * v1.numel(), lambda: capi.element_loads(X, e2n, src1, coef=c1, out=v1, stream=st())),
                             ("loads_vdim%d" % dim, 8 * vec.numel(), lambda: capi.element_loads(X, e2n, src, vdim=dim, coef=c1, out=vec, stream=st()))]
                    for tag, nbytes, call in forms:
                        t = reps(call)
                        b_ms = 1e3 * nbytes / (a.hbm_gbs * 1e9)
                        rec = {"case": "%s:%s" % (name, tag), "elements": NE, "bound_bytes": int(nbytes), "device_ms": t,
                               "hbm_bound_ms": round(b_ms, 4), "fraction_of_bound": round(b_ms / min(t), 4)}
                        if fam == "q2":
                            seen[tag] = rec["fraction_of_bound"]
                        else:
                            rec["yardstick_fraction_of_bound"] = seen.get(tag)
                        print(json.dumps(rec), flush=True)
                    for tag, call in [("boundary_mass", lambda: capi.boundary_mass(X, e2n, fe, fl, alpha, add_to=o1, stream=st())),
                                      ("boundary_loads", lambda: capi.boundary_loads(X, e2n, fe, fl, src1, coef=alpha, add_to=v1, stream=st()))]:
                        t = reps(call)
                        rec = {"case": "%s:%s" % (name, tag), "elements": NE, "faces": NF, "device_ms": t}
                        if fam == "q2":
                            seen[tag] = min(t)
                        else:
                            rec["yardstick_ms"] = seen.get(tag)
                        print(json.dumps(rec), flush=True)
                except (RuntimeError, MemoryError) as e:
                    print(json.dumps({"case": "%s %dD n = %d" % (fam, dim, n), "skipped": str(e)[:200]}), flush=True)
                X = e2n = out = vec = o1 = v1 = fe = fl = alpha = src = src1 = c1 = c2 = None
                torch.cuda.empty_cache()
                capi.release_cached_memory()
        return

    if a.points:
        def reps(call):
            timed(call)                            # warm-up
            return [round(timed(call)[0], 3) for _ in range(a.reps)]
        for name, n, nd in [("hex128", 128, 8), ("hex256", 256, 8), ("q2_hex64", 64, 27), ("tet10_64", 64, 10)]:
            try:
                X, e2v, g = mesh(n) if nd == 8 else (mesh_q2(n, 3) if nd == 27 else mesh_p2(n, 3)[:3])
                NE, NV = int(e2v.shape[0]), int(X.shape[0])
                NQ = capi.element_points(X, e2v, sizes_only=True)[5]
                u = torch.rand(NV, generator=g, device=dev, dtype=torch.float64)
                fq = torch.rand(NQ, generator=g, device=dev, dtype=torch.float64)
                exg = torch.rand((NQ, 1, 3), generator=g, device=dev, dtype=torch.float64)
                qp = torch.zeros(NE + 1, dtype=torch.int64, device=dev)
                xq = torch.zeros(NQ * 3, dtype=torch.float64, device=dev)
                gq = torch.zeros(NQ * 3, dtype=torch.float64, device=dev)
                wdet, uq = torch.zeros(NQ, dtype=torch.float64, device=dev), torch.zeros(NQ, dtype=torch.float64, device=dev)
                vec = torch.zeros(NE * nd, dtype=torch.float64, device=dev)
                err = torch.zeros(NE * 2, dtype=torch.float64, device=dev)
                st = stream
                mesh_bytes = 8 * X.numel() + 4 * e2v.numel()      # read once by every call
                calls = [("points", mesh_bytes + 8 * (NE + 1) + 8 * 4 * NQ,
                          lambda: capi.element_points(X, e2v, out={"qp_ptr": qp, "xq": xq, "wdet": wdet}, stream=st())),
                         ("eval", mesh_bytes + 8 * NV + 8 * 4 * NQ,
                          lambda: capi.element_eval(X, e2v, u, out={"uq": uq, "gradq": gq}, stream=st())),
                         ("eval_values_only", mesh_bytes + 8 * NV + 8 * NQ,
                          lambda: capi.element_eval(X, e2v, u, want=("uq",), out={"uq": uq}, stream=st())),
                         ("loads_points", mesh_bytes + 8 * NQ + 8 * vec.numel(),
                          lambda: capi.element_loads_points(X, e2v, fq, out=vec, stream=st())),
                         ("errors", mesh_bytes + 8 * NV + 8 * 4 * NQ + 8 * err.numel(),
                          lambda: capi.element_errors(X, e2v, u, fq, exg, out=err, stream=st())),
                         ("loads (nodal, the yardstick)", mesh_bytes + 8 * NV + 8 * vec.numel(),
                          lambda: capi.element_loads(X, e2v, u, out=vec, stream=st()))]
                for tag, nbytes, call in calls:
                    t = reps(call)
                    b_ms = 1e3 * nbytes / (a.hbm_gbs * 1e9)
                    print(json.dumps({"case": "points:%s:%s" % (name, tag), "elements": NE, "points": NQ, "bound_bytes": int(nbytes),
                                      "device_ms": t, "hbm_bound_ms": round(b_ms, 4), "fraction_of_bound": round(b_ms / min(t), 4)}),
                          flush=True)
            except (RuntimeError, MemoryError) as e:
                print(json.dumps({"case": "points:" + name, "skipped": str(e)[:200]}), flush=True)
            X = e2v = u = fq = exg = qp = xq = gq = wdet = uq = vec = err = None
            torch.cuda.empty_cache()
            capi.release_cached_memory()
        return

    if a.point_coef:
        def reps(call):
            timed(call)                            # warm-up
            return [round(timed(call)[0], 3) for _ in range(a.reps)]
        for name, n, nd, stiff_points in [("hex128", 128, 8, 8), ("q2_hex64", 64, 27, 27), ("tet10_64", 64, 10, 4)]:
            try:
                X, e2v, g = mesh(n) if nd == 8 else (mesh_q2(n, 3) if nd == 27 else mesh_p2(n, 3)[:3])
                NE = int(e2v.shape[0])
                NQ = capi.element_points(X, e2v, sizes_only=True)[5]
                nq = NQ // NE

                def coefs(rows):
                    """(symmetric tensor, lambda / mu, scalar) with `rows` rows: the diagonal in [0.5, 2), off it in [-0.2, 0.2]"""
                    k = 0.5 + 1.5 * torch.rand((rows, 6), generator=g, device=dev, dtype=torch.float64)
                    k[:, 3:] = (k[:, 3:] - 1.25) * (0.4 / 1.5)
                    return k, 0.5 + 1.5 * torch.rand((rows, 2), generator=g, device=dev, dtype=torch.float64), k[:, 0].contiguous()
                kq, lq, sq = coefs(NQ)
                ke, le, se = coefs(NE)
                out = torch.zeros(NE * (nd * 3) ** 2, dtype=torch.float64, device=dev)
                o1 = out[:NE * nd * nd]
                st = stream
                mesh_bytes = 8 * X.numel() + 4 * e2v.numel()
                pairs = [
                    ("diffusion_sym", 8 * o1.numel(), 6,
                     lambda: capi.element_matrices_points(X, e2v, 0, kq, device=True, out=o1, stream=st()),
                     lambda: capi.element_matrices(X, e2v, 0, ke, device=True, out=o1, stream=st())),
                    ("elasticity", 8 * out.numel(), 2,
                     lambda: capi.element_matrices_points(X, e2v, 1, lq, device=True, out=out, stream=st()),
                     lambda: capi.element_matrices(X, e2v, 1, le, device=True, out=out, stream=st())),
                    ("mass", 8 * o1.numel(), 1,
                     lambda: capi.element_mass_points(X, e2v, sq, out=o1, stream=st()),
                     lambda: capi.element_mass(X, e2v, se, out=o1, stream=st())),
                    ("mass_accumulate", 16 * o1.numel(), 1,
                     lambda: capi.element_mass_points(X, e2v, sq, add_to=o1, stream=st()),
                     lambda: capi.element_mass(X, e2v, se, add_to=o1, stream=st())),
                ]
                for tag, out_bytes, ncoef, new, old in pairs:
                    t_new, t_old = reps(new), reps(old)
                    b_new, b_old = mesh_bytes + out_bytes + 8 * ncoef * NQ, mesh_bytes + out_bytes + 8 * ncoef * NE
                    ms = lambda b: round(1e3 * b / (a.hbm_gbs * 1e9), 4)
                    print(json.dumps({"case": "point_coef:%s:%s" % (name, tag), "elements": NE, "points": NQ, "device_ms": t_new,
                                      "bound_bytes": int(b_new), "hbm_bound_ms": ms(b_new),
                                      "fraction_of_bound": round(ms(b_new) / min(t_new), 4),
                                      "yardstick_ms": t_old, "yardstick_bound_bytes": int(b_old), "yardstick_hbm_bound_ms": ms(b_old),
                                      "yardstick_fraction_of_bound": round(ms(b_old) / min(t_old), 4),
                                      "expected_extra_ms": ms(b_new - b_old), "measured_extra_ms": round(min(t_new) - min(t_old), 3),
                                      "ratio": round(min(t_new) / min(t_old), 3),
                                      "point_ratio": 1.0 if tag.startswith("mass") else round(nq / stiff_points, 3)}), flush=True)
            except (RuntimeError, MemoryError) as e:
                print(json.dumps({"case": "point_coef:" + name, "skipped": str(e)[:200]}), flush=True)
            X = e2v = kq = lq = sq = ke = le = se = out = o1 = None
            torch.cuda.empty_cache()
            capi.release_cached_memory()
        return

    if a.boundary_points:
        def reps(call):
            timed(call)                            # warm-up
            return [round(timed(call)[0], 3) for _ in range(a.reps)]
        for name, n, nd in [("hex128", 128, 8), ("q2_hex64", 64, 27), ("tet10_64", 64, 10)]:
            try:
                if nd == 10:
                    X, e2v, g, P = mesh_p2(n, 3)
                    fe, fl = simplex_boundary(P, n, 3)
                    P = None
                else:
                    X, e2v, g = mesh(n) if nd == 8 else mesh_q2(n, 3)
                    fe, fl = grid_boundary(n, 3)
                NE, NF = int(e2v.shape[0]), int(fe.numel())
                info = capi.boundary_points(X, e2v, fe, fl, sizes_only=True)
                NFQ, fn = info[5], {8: 4, 27: 9, 10: 6}[nd]
                alpha = 0.5 + 1.5 * torch.rand(NF, generator=g, device=dev, dtype=torch.float64)
                alphaq = 0.5 + 1.5 * torch.rand(NFQ, generator=g, device=dev, dtype=torch.float64)
                u = torch.rand(X.shape[0], generator=g, device=dev, dtype=torch.float64)
                gq = torch.rand(NFQ, generator=g, device=dev, dtype=torch.float64)
                out = torch.zeros(NE * nd * nd, dtype=torch.float64, device=dev)
                vec = torch.zeros(NE * nd, dtype=torch.float64, device=dev)
                pts = {"fp_ptr": torch.zeros(NF + 1, dtype=torch.int64, device=dev), "xq": torch.zeros(NFQ * 3, dtype=torch.float64, device=dev),
                       "wmeas": torch.zeros(NFQ, dtype=torch.float64, device=dev), "normal": torch.zeros(NFQ * 3, dtype=torch.float64, device=dev)}
                ev = {"uq": torch.zeros(NFQ, dtype=torch.float64, device=dev), "gradq": torch.zeros(NFQ * 3, dtype=torch.float64, device=dev)}
                st = stream
                # what a call must move: the face lists and the offsets (4 + 4 + 8 bytes per face), the coordinates of the nodes
                # it reads and their vertex ids (the face's nodes; eval with the gradient: all nodes of the owning element, with
                # u), point inputs read once, outputs written once (the matrices and vectors: read and written)
                lists, face_nodes, elem_nodes = 16 * NF, NF * fn * (24 + 4), NF * nd * (24 + 8 + 4)
                calls = [
                    ("points", lists + face_nodes + 8 * NFQ * 7 + 8 * NF, None,
                     lambda: capi.boundary_points(X, e2v, fe, fl, out=pts, stream=st())),
                    ("eval", lists + face_nodes + NF * fn * 8 + elem_nodes + 8 * NFQ * 4, None,
                     lambda: capi.boundary_eval(X, e2v, fe, fl, u, out=ev, stream=st())),
                    ("eval_trace_only", lists + face_nodes + NF * fn * 8 + 8 * NFQ, None,
                     lambda: capi.boundary_eval(X, e2v, fe, fl, u, want=("uq",), out={"uq": ev["uq"]}, stream=st())),
                    ("mass_points", lists + face_nodes + 8 * NFQ + 16 * NF * fn * fn,
                     lambda: capi.boundary_mass(X, e2v, fe, fl, alpha, add_to=out, stream=st()),
                     lambda: capi.boundary_mass_points(X, e2v, fe, fl, alphaq, add_to=out, stream=st())),
                    ("loads_points", lists + face_nodes + 8 * NF + 8 * NFQ + 16 * NF * fn,
                     lambda: capi.boundary_loads(X, e2v, fe, fl, u, coef=alpha, add_to=vec, stream=st()),
                     lambda: capi.boundary_loads_points(X, e2v, fe, fl, gq, coef=alpha, add_to=vec, stream=st())),
                ]
                for tag, nbytes, old, new in calls:
                    t = reps(new)
                    b_ms = 1e3 * nbytes / (a.hbm_gbs * 1e9)
                    rec = {"case": "boundary_points:%s:%s" % (name, tag), "elements": NE, "faces": NF, "face_points": NFQ,
                           "device_ms": t, "bound_bytes": int(nbytes), "hbm_bound_ms": round(b_ms, 5),
                           "fraction_of_bound": round(b_ms / min(t), 5)}
                    if old:
                        rec["per_face_call_ms"] = reps(old)
                        rec["ratio"] = round(min(t) / min(rec["per_face_call_ms"]), 3)
                    print(json.dumps(rec), flush=True)
            except (RuntimeError, MemoryError) as e:
                print(json.dumps({"case": "boundary_points:" + name, "skipped": str(e)[:200]}), flush=True)
            X = e2v = fe = fl = alpha = alphaq = u = gq = out = vec = pts = ev = None
            torch.cuda.empty_cache()
            capi.release_cached_memory()
        return

    if a.boundary:
        for name, n, dim, nd, vdim in [("hex128", 128, 3, 8, 1), ("hex256", 256, 3, 8, 1), ("q2_hex64", 64, 3, 27, 1),
                                       ("q2_hex64_vdim3", 64, 3, 27, 3), ("quad9_2048", 2048, 2, 9, 1)]:
            try:
                X, e2v, g = mesh(n) if nd == 8 else mesh_q2(n, dim)
                NE, size = n ** dim, nd * vdim
                fe, fl = grid_boundary(n, dim)
                NF = int(fe.numel())
                alpha = 0.5 + 1.5 * torch.rand(NF, generator=g, device=dev, dtype=torch.float64)
                sigma = 0.5 + 1.5 * torch.rand(NE, generator=g, device=dev, dtype=torch.float64)
                gn = torch.rand((X.shape[0], vdim), generator=g, device=dev, dtype=torch.float64)
                out = torch.zeros(NE * size * size, dtype=torch.float64, device=dev)
                vec = torch.zeros(NE * size, dtype=torch.float64, device=dev)
                info = capi.boundary_mass(X, e2v, fe, fl, alpha, vdim=vdim, sizes_only=True)
                rec = {"case": "boundary:" + name, "elements": NE, "faces": NF, "vdim": vdim, "elements_touched": info[7],
                       "mass_additions": info[5]}
                for tag, call in [("mass_accumulate_ms", lambda: capi.element_mass(X, e2v, sigma, vdim=vdim, add_to=out, stream=stream())),
                                  ("boundary_mass_ms", lambda: capi.boundary_mass(X, e2v, fe, fl, alpha, vdim=vdim, add_to=out, stream=stream())),
                                  ("boundary_loads_ms", lambda: capi.boundary_loads(X, e2v, fe, fl, gn, vdim=vdim, coef=alpha, add_to=vec,
                                                                                    stream=stream()))]:
                    timed(call)                    # warm-up
                    rec[tag] = [round(timed(call)[0], 3) for _ in range(a.reps)]
                rec["boundary_mass_over_yardstick"] = round(min(rec["boundary_mass_ms"]) / min(rec["mass_accumulate_ms"]), 4)
                rec["boundary_loads_over_yardstick"] = round(min(rec["boundary_loads_ms"]) / min(rec["mass_accumulate_ms"]), 4)
                print(json.dumps(rec), flush=True)
            except (RuntimeError, MemoryError) as e:
                print(json.dumps({"case": "boundary:" + name, "skipped": str(e)[:200]}), flush=True)
            X = e2v = out = vec = fe = fl = alpha = sigma = gn = None
            torch.cuda.empty_cache()
            capi.release_cached_memory()
        return

    host_reps = a.reps if a.host_reps is None else a.host_reps
    cases = [("hex_diffusion%d" % n, n, 0, 3, 8) for n in ints(a.hex)] + \
            [("hex_elasticity%d" % n, n, 1, 3, 8) for n in ints(a.elasticity)] + \
            [("q2_hex_diffusion%d" % n, n, 0, 3, 27) for n in ints(a.q2_hex)] + \
            [("q2_hex_elasticity%d" % n, n, 1, 3, 27) for n in ints(a.q2_elasticity)] + \
            [("quad9_diffusion%d" % n, n, 0, 2, 9) for n in ints(a.quad9)]
    for name, n, kind, dim, nd in cases:
        try:
            X, e2v, g = mesh(n) if nd == 8 else mesh_q2(n, dim)
            NE = n ** dim
            size = nd * (dim if kind else 1)
            coef = 0.5 + 1.5 * torch.rand((NE, 2) if kind else (NE,), generator=g, device=dev, dtype=torch.float64)
            out = torch.zeros(NE * size * size, dtype=torch.float64, device=dev)
            run = lambda: capi.element_matrices(X, e2v, kind, coef, device=True, out=out, stream=stream())
            timed(run)                             # warm-up
            t_dev = [timed(run)[0] for _ in range(a.reps)]
            out_bytes = 8 * out.numel()
            in_bytes = 8 * X.numel() + 4 * e2v.numel() + 8 * coef.numel()
            bound_ms = 1e3 * out_bytes / (a.hbm_gbs * 1e9)
            rec = {"case": name, "elements": NE, "matrix_size": size, "output_bytes": int(out_bytes), "input_bytes": int(in_bytes),
                   "device_ms": [round(x, 3) for x in t_dev], "hbm_bound_ms": round(bound_ms, 3),
                   "fraction_of_bound": round(bound_ms / min(t_dev), 3)}
            if nd != 8:
                rec["ops_per_element"] = ops_per_element(dim, nd, kind)
                rec["compute_bound_ms"] = round(1e3 * NE * rec["ops_per_element"] / (a.fp64_gops * 1e9), 3)
            if not a.no_host:
                # what a driver without this call does: the matrices on the host (here the cheapest generator there is, one
                # box matrix scaled per element -- an integrator call per element costs more), then the upload
                h = (1.0 / n,) * 3
                if nd == 8:
                    Kref = problems.hex_elasticity_matrix(h) if kind else problems.hex_element_matrix(h)
                elif nd == 27:
                    Kref = problems.hex_elasticity_matrix_tensor(h, 2) if kind else problems.hex_diffusion_matrix_tensor(h, 2)
                else:
                    Kref = problems.quad_mesh_problem(1, 1, order=2, coef=1.0).elmat[0]      # (the square's: it scales with h^0)
                c = coef.reshape(NE, -1)[:, 0].cpu().numpy()
                t_gen, t_up = [], []
                for _ in range(host_reps):
                    t = time.perf_counter()
                    host = np.ascontiguousarray(c[:, None, None] * Kref[None, :, :])
                    t_gen.append(1e3 * (time.perf_counter() - t))
                    t_up.append(timed(lambda: out.view(NE, size, size).copy_(torch.from_numpy(host)))[0])
                    host = None
                rec["host_generate_ms"] = [round(x, 1) for x in t_gen]
                rec["upload_ms"] = [round(x, 1) for x in t_up]
            print(json.dumps(rec), flush=True)
            if not a.no_mass:
                vdim = dim if kind else 1
                sigma = coef.reshape(NE, -1)[:, 0].contiguous()
                src = torch.rand((X.shape[0], vdim), generator=g, device=dev, dtype=torch.float64)
                vec = torch.zeros(NE * size, dtype=torch.float64, device=dev)
                calls = [("mass", out_bytes, lambda: capi.element_mass(X, e2v, sigma, vdim=vdim, out=out, stream=stream())),
                         ("mass_accumulate", 2 * out_bytes, lambda: capi.element_mass(X, e2v, sigma, vdim=vdim, add_to=out, stream=stream())),
                         ("loads", 8 * vec.numel(), lambda: capi.element_loads(X, e2v, src, vdim=vdim, coef=sigma, out=vec, stream=stream()))]
                for tag, nbytes, call in calls:
                    timed(call)                    # warm-up
                    t = [timed(call)[0] for _ in range(a.reps)]
                    b_ms = 1e3 * nbytes / (a.hbm_gbs * 1e9)
                    print(json.dumps({"case": name + ":" + tag, "elements": NE, "vdim": vdim, "bound_bytes": int(nbytes),
                                      "device_ms": [round(x, 3) for x in t], "hbm_bound_ms": round(b_ms, 4),
                                      "fraction_of_bound": round(b_ms / min(t), 4),
                                      "stiffness_fraction_of_bound": rec["fraction_of_bound"]}), flush=True)
                src = vec = None
            if kind == 0 and nd == 8 and n in ints(a.rhs):
                vec = capi.element_loads(X, e2v, torch.ones(X.shape[0], dtype=torch.float64, device=dev), device=True)
                op = capi.Operator(X.shape[0], e2v, out, None)
                try:
                    b = torch.zeros(X.shape[0], dtype=torch.float64, device=dev)
                    timed(lambda: op.assemble_rhs(vec, b=b))
                    t = [timed(lambda: op.assemble_rhs(vec, b=b))[0] for _ in range(a.reps)]
                    b_ms = 1e3 * 8 * vec.numel() / (a.hbm_gbs * 1e9)
                    print(json.dumps({"case": "assemble_rhs%d" % n, "dofs": int(X.shape[0]), "elvec_bytes": int(8 * vec.numel()),
                                      "device_ms": [round(x, 3) for x in t], "hbm_bound_ms": round(b_ms, 4),
                                      "fraction_of_bound": round(b_ms / min(t), 4)}), flush=True)
                finally:
                    op.close()
                vec = b = None
        except (RuntimeError, MemoryError) as e:
            print(json.dumps({"case": name, "skipped": str(e)[:200]}), flush=True)
        X = e2v = coef = out = None
        torch.cuda.empty_cache()
        capi.release_cached_memory()


if __name__ == "__main__":
    main()
