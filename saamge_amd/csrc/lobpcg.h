// Lowest eigenpairs of (A, M): LOBPCG preconditioned by the hierarchy's V-cycle (lobpcg.hip), the device driver of
// saamge_amd/lobpcg_model.py.
#pragma once
#include "hierarchy.h"

namespace saamge_amd {

struct LobpcgOptions {
    int nev = 1, nb = 1;        // wanted pairs and block size, 1 <= nev <= nb <= 16
    double tol = 1e-8;
    int max_iter = 100;
    bool constrain_essential = true;
    unsigned seed = 0;
};

// A = the level-0 operator of H, B = its V-cycle, M = a CSR matrix on the device or null (the identity).  x0: n x nb on the
// device or null (the hashed start block); evecs: n x nev on the device.  evals, res (nev), hist ((max_iter + 1) x nev,
// row-major, may be null) on the host.  The arguments are the caller's to check (capi.hip).
void lobpcg_solve(Hierarchy &H, const DCsr *M, const LobpcgOptions &o, const double *x0, double *evals, double *evecs,
                  double *res, int *iters, int *converged, double *hist);

}  // namespace saamge_amd
