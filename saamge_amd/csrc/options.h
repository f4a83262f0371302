#pragma once

namespace saamge_amd {

// Options of the library (saamge_amd_options, include/saamge_amd.h).  A hierarchy carries the copy it was built with
// (Params::opt) for its whole life; the entry points without a hierarchy take the default of saamge_amd_set_options.
// What is left of the ~50 environment switches of rounds 1-3: the variants that were measured without gain are gone, the
// ones tests need to reach a code path (or a caller may want) are fields here.  Environment variables that remain:
// SAAMGE_AMD_TIMING, SAAMGE_AMD_SERIAL (diagnostics), SAAMGE_AMD_POOL_MAX_GB, SAAMGE_AMD_THREADS (resources).
struct Options {
    int eig_strict = 0;               // few-eigenpairs path: a fallback to the dense path is an error (tests of that path)
    int eig_certify = 1;              // the count #{lambda < theta} certified by the inertia of C - theta I
    int eig_min_n = 64;               // smallest agglomerate of a batch that takes the few-eigenpairs path
    int eig_force_fallback = 0;       // tests: every k-th matrix takes the per-matrix dense fallback
    int eig_dense_only = 0;           // saamge_amd_lower_eigens_batched: the dense path (a hierarchy: saamge_amd_params.eigensolver)
    int eig_dense_one_stage = 0;      // dense path: one-stage blocked Householder reduction instead of the two-stage one
    int eig_nullcheck = 1;            // known-null-vector shortcut (ss_nullcheck_kernel)
    int eig_keep_inertia_factor = 1;  // wide-band matrices with certified count 0 keep the factor of the inertia pass
    int band_assembly = 1;            // coarse-level agglomerate matrices assembled inside their band
    int eig_dedupe = 1;               // bitwise identical agglomerate matrices of a batch are solved once
    int eig_outer_panels = 8;         // 16-column panels per outer block of the wide-band factorisations (2: the right-looking two-panel walk)
    int overlap = 15;                 // bit 0 subspace iteration beside the next chunk, 1 halo exchange beside the interior rows, 2 Galerkin product beside the next level, 3 fine operator data beside the AE tables
    int sell = 31;                    // bit 0 coded slices at all, 1 pair coding, 2 short-chain kernel path, 3 operator-level dictionary, 4 node blocks, 5 (off) coded smoother diagonal, 6 (off) row patterns OFF
    int spmv_sell = 0;                // saamge_amd_spmv / spmv64 build and use the SELL copy
    int debug = 0;                    // bit 0 iteration traces of the few-eigenpairs path, 1 operator format census, 2 level tags in the kernel profile
    int host_heap_pad_mb = 256;       // > 0: glibc never trims its heap, serves blocks up to 32 MB from it and grows it in steps of this size (0: allocator left alone)
    int ae_order = 0;                 // local order of the agglomerate matrices: 0 rank / box order (ae_perm_kernel), 1 the level order of ae_order_model.py where it is narrower
};

}  // namespace saamge_amd
