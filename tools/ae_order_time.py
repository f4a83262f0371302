"""Setup time with saamge_amd_options.ae_order 0 and 1 on meshes whose global numbering scatters the dofs of an agglomerate.

poisson3d_device at n^3 (default 64 and 128; 8 x 8 x 4 agglomerates, two coarsenings), its dofs renumbered on the device by
  random       a fixed random permutation,
  refinement   coarse vertices first: the vertices whose coordinates are all multiples of n / 2 first, then those of n / 4,
               ..., of 2, the rest; lexicographic inside a class (an approximation of what uniform refinement does),
  none         the generator's lexicographic numbering (nothing to gain: the price of the option).
ae_order 0 and 1 alternate in one process after a warm-up of both; host clock closed by a synchronise, `--reps` repetitions
(all listed).  Then, with the kernel profile on, one setup per value for the time of the ordering kernel
(ae_level_order; with ae_order 0 it only measures the band) beside the sum over all profiled kernels.  One JSON line per case.

    python tools/ae_order_time.py [--n 64,128] [--numberings random,refinement,none] [--reps 3] [--levels 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def renumber(p, perm):
    """the problem with dof i renamed perm[i]: operator (rows sorted by column), elements, flags, right-hand side"""
    import torch
    n = p.n
    rowptr = p.rowptr.long()
    counts = rowptr[1:] - rowptr[:-1]
    rows = torch.repeat_interleave(torch.arange(n, device=perm.device), counts)
    key = perm[rows] * n + perm[p.col.long()]
    order = torch.argsort(key)
    q = type(p)(**p.__dict__)
    q.col = (key[order] % n).to(torch.int32).contiguous()
    q.val = p.val[order].contiguous()
    nc = torch.zeros(n, dtype=torch.int64, device=perm.device)
    nc[perm] = counts
    rp = torch.zeros(n + 1, dtype=torch.int64, device=perm.device)
    rp[1:] = torch.cumsum(nc, 0)
    q.rowptr = rp.to(p.rowptr.dtype).contiguous()
    q.elem_to_dof = perm[p.elem_to_dof.long()].to(torch.int32).contiguous()
    q.bdr = torch.empty_like(p.bdr)
    q.bdr[perm] = p.bdr
    q.b = torch.empty_like(p.b)
    q.b[perm] = p.b
    return q


def numbering(kind, n, device):
    import torch
    nv = n + 1
    ND = nv ** 3
    if kind == "random":
        g = torch.Generator(device="cpu")
        g.manual_seed(20240607)
        return torch.randperm(ND, generator=g).to(device)
    iz = torch.arange(nv, device=device).view(-1, 1, 1)
    iy = torch.arange(nv, device=device).view(1, -1, 1)
    ix = torch.arange(nv, device=device).view(1, 1, -1)
    cls = torch.zeros((nv, nv, nv), dtype=torch.int64, device=device)
    m = 2
    while m <= n // 2:
        cls += ((ix % m == 0) & (iy % m == 0) & (iz % m == 0)).long()
        m *= 2
    lex = torch.arange(ND, device=device)
    order = torch.argsort((cls.max() - cls).reshape(-1) * ND + lex)       # coarsest class first, lexicographic inside
    perm = torch.empty(ND, dtype=torch.int64, device=device)
    perm[order] = lex
    return perm


def main():
    import torch
    from saamge_amd import capi, problems

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="64,128")
    ap.add_argument("--numberings", default="random,refinement,none")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--levels", type=int, default=3)
    a = ap.parse_args()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    nco = a.levels - 1

    def setup(p, ae_order, keep=False):
        params = capi.default_params(num_coarsenings=nco, theta=0.003, nu_relax=3)
        params.options.ae_order = ae_order
        torch.cuda.synchronize()
        t = time.perf_counter()
        h = capi.Hierarchy(p.rowptr, p.col, p.val, p.n, p.elem_to_dof, p.elmat, p.bdr, p.partitions, p.nparts, params, p.NE_,
                           8, stream=stream())
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t)
        if keep:
            return ms, h
        h.close()
        return ms, None

    for n in [int(x) for x in a.n.split(",") if x]:
        base = problems.poisson3d_device(n, blk=(8, 8, 4), coarse_blk=[(8, 8, 4)] * (nco - 1), device="cuda")
        for kind in [k for k in a.numberings.split(",") if k]:
            p = base if kind == "none" else renumber(base, numbering(kind, n, base.b.device))
            for o in (0, 1):
                setup(p, o)                                        # warm-up
            ms = {0: [], 1: []}
            for _ in range(a.reps):
                for o in (0, 1):
                    ms[o].append(round(setup(p, o)[0], 2))
            rec = {"n": n, "numbering": kind, "rows": p.n, "levels": a.levels, "setup_ms_ae_order_0": ms[0], "setup_ms_ae_order_1": ms[1]}
            for o in (0, 1):
                capi.profile(True)
                capi.profile_reset()
                _, h = setup(p, o, keep=True)
                st = {s["name"]: s for s in capi.profile_stats()}
                capi.profile(False)
                rec["order_info_ae_order_%d" % o] = [h.level_order_info(l) for l in range(nco)]
                rec["agglomerates"] = [h.level_info(l)["nparts"] for l in range(nco)]
                x = torch.zeros_like(p.b)
                _, it, conv, _ = h.pcg(p.b, x, rel_tol=1e-8, max_iter=200)
                rec["pcg_iterations_ae_order_%d" % o] = int(it) if conv else -int(it)
                h.close()
                rec["kernel_ms_ae_order_%d" % o] = {k: round(st[k]["ms"], 3) for k in ("ae_level_order",) if k in st}
                rec["profiled_kernels_ms_ae_order_%d" % o] = round(sum(s["ms"] for s in st.values()), 2)
            print(json.dumps(rec), flush=True)
            if kind != "none":
                del p
            torch.cuda.empty_cache()
            capi.release_cached_memory()


if __name__ == "__main__":
    main()
