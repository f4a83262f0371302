"""Times the element matrices computed on the device (saamge_amd_element_matrices) on device inputs: Q1 diffusion on n^3
hexes with a scalar coefficient per element and Q1 hex elasticity, against their HBM lower bound (the output written once
at --hbm-gbs; the inputs, listed as input_bytes, add 13 % for diffusion and 2 % for elasticity and are not in the bound),
beside the path this replaces: the element matrices generated on the host as problems.py does (one closed-form box matrix
scaled per element) and uploaded.  Host clock closed by a synchronise, one
warm-up, `--reps` repetitions (all listed).  One JSON line per case.

    python tools/elmat_time.py [--hex 128,256] [--elasticity 64] [--reps 3] [--hbm-gbs 8000] [--no-host]

The vertices are jittered by 0.2 mesh widths, so no two elements are alike.  A case that does not fit is reported as skipped
with the error.
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--no-host", action="store_true")
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

    cases = [("hex_diffusion%d" % n, n, 0) for n in ints(a.hex)] + [("hex_elasticity%d" % n, n, 1) for n in ints(a.elasticity)]
    for name, n, kind in cases:
        try:
            X, e2v, g = mesh(n)
            NE = n ** 3
            size = 24 if kind else 8
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
            if not a.no_host:
                # what a driver without this call does: the matrices on the host (here the cheapest generator there is, one
                # box matrix scaled per element -- an integrator call per element costs more), then the upload
                h = (1.0 / n,) * 3
                Kref = problems.hex_elasticity_matrix(h) if kind else problems.hex_element_matrix(h)
                c = coef.reshape(NE, -1)[:, 0].cpu().numpy()
                t_gen, t_up = [], []
                for _ in range(a.reps):
                    t = time.perf_counter()
                    host = np.ascontiguousarray(c[:, None, None] * Kref[None, :, :])
                    t_gen.append(1e3 * (time.perf_counter() - t))
                    t_up.append(timed(lambda: out.view(NE, size, size).copy_(torch.from_numpy(host)))[0])
                    host = None
                rec["host_generate_ms"] = [round(x, 1) for x in t_gen]
                rec["upload_ms"] = [round(x, 1) for x in t_up]
            print(json.dumps(rec), flush=True)
        except (RuntimeError, MemoryError) as e:
            print(json.dumps({"case": name, "skipped": str(e)[:200]}), flush=True)
        X = e2v = coef = out = None
        torch.cuda.empty_cache()
        capi.release_cached_memory()


if __name__ == "__main__":
    main()
