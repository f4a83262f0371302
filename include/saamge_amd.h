/* saamge_amd -- C ABI of the MI355X-native SAAMGE hot path (setup + solve).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Every
 * entry point names the reference interface (LLNL/saamge, paths relative to amg/) it
 * replaces.  Array arguments may be HOST or DEVICE pointers unless stated otherwise:
 * device pointers are used in place (zero copy), host pointers are uploaded once.
 * All indices are 32-bit like the reference's hypre/MFEM `int`; all reals are fp64.
 *
 * Return value: 0 on success, non-zero on failure (the reference aborts through
 * SA_ASSERT -> MPI_Abort, inc/common.hpp:635-647; here the message is kept in
 * saamge_amd_last_error()).  Not thread-safe (neither is the reference: global
 * singletons, src/process.cpp:46-48); one hierarchy may be used from one thread at a time.
 */
#ifndef SAAMGE_AMD_H
#define SAAMGE_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define SAAMGE_AMD_MAX_LEVELS 8

/* agg_dof_status_t bit flags, inc/aggregates.hpp:102-105 */
#define SAAMGE_AMD_BETWEEN_AES 0x01
#define SAAMGE_AMD_ON_ESS_DOMAIN_BORDER 0x02
#define SAAMGE_AMD_ON_PROC_IFACE 0x04
#define SAAMGE_AMD_OWNED 0x08

typedef struct saamge_amd_hierarchy saamge_amd_hierarchy; /* == ml_data_t, inc/ml.hpp:118-120 */

/* Options of the library's own machinery (no counterpart in the reference): what is left of the environment switches of
 * rounds 1-3.  The variants that were measured without gain are gone; these remain because tests need them to reach a code
 * path or because a caller may want them.  PER HIERARCHY: params->options is what a hierarchy uses for its whole life
 * (setup, saamge_amd_update_operators, solves); building one neither reads nor alters the default, and hierarchies with
 * different options may coexist.  saamge_amd_set_options() sets the process-wide DEFAULT: what saamge_amd_get_options
 * returns (for callers who fill params->options from it) and what the entry points without a hierarchy use
 * (saamge_amd_spmv / spmv64, saamge_amd_lower_eigens_batched, saamge_amd_inertia_batched); it never reaches a hierarchy
 * that already exists.  Values out of range are refused (saamge_amd_last_error names the field).  Only host_heap_pad_mb
 * is a property of the process: the first hierarchy's value applies.  Environment variables that remain: SAAMGE_AMD_TIMING (phase
 * times on stderr), SAAMGE_AMD_SERIAL (no worker threads in the setup: counter passes), SAAMGE_AMD_POOL_MAX_GB (device
 * block cache, default 64), SAAMGE_AMD_THREADS (host threads of the host topology builds). */
typedef struct saamge_amd_options {
    int eig_strict;               /* 0.  1: a fallback of the few-eigenpairs path to the dense path is an ERROR */
    int eig_certify;              /* 1.  0: no inertia certificate (residual bounds only): kept to show what the certificate is for */
    int eig_min_n;                /* 64: smallest agglomerate of a batch that takes the few-eigenpairs path */
    int eig_force_fallback;       /* 0.  k > 0: every k-th matrix of a batch takes the per-matrix dense fallback (tests) */
    int eig_dense_only;           /* 0.  1: saamge_amd_lower_eigens_batched uses the dense path (a hierarchy: params.eigensolver) */
    int eig_dense_one_stage;      /* 0.  1: dense path by the one-stage blocked Householder reduction instead of the two-stage one */
    int eig_nullcheck;            /* 1: agglomerates whose one wanted pair is the known null vector skip the iteration */
    int eig_keep_inertia_factor;  /* 1: wide-band matrices with certified count 0 keep the factor of the inertia pass */
    int band_assembly;            /* 1: coarse-level agglomerate matrices are assembled, summed and scaled inside their band */
    int eig_dedupe;               /* 1: bitwise identical agglomerate matrices of a batch (structured meshes, piecewise constant
                                   * coefficients) are solved once, their eigenpairs copied to the other members of the class */
    int eig_outer_panels;         /* 8: 16-column panels per outer block of the wide-band factorisations (left-looking panels,
                                   * one rank-128 update of the trailing window on the matrix cores); 4: rank-64; 2: the
                                   * right-looking two-panel walk of rounds 2-3 */
    int overlap;                  /* 15: bit 0 subspace iteration of a chunk beside the next chunk's assembly, bit 1 halo exchange
                                   * beside the interior rows, bit 2 Galerkin product beside the next level's eigenproblems,
                                   * bit 3 the fine operator's SELL copy and smoother diagonal beside the AE tables */
    int sell;                     /* 31: SELL slice formats: bit 0 coded slices at all, bit 1 pair coding (values in the table),
                                   * bit 2 the short-chain kernel path, bit 3 operator-level dictionary, bit 4 3 x 3 node blocks,
                                   * bit 5 (off) the smoother's diagonal as byte codes where the rows of the operator repeat,
                                   * bit 6 (off) row patterns OFF: staged tiles stream every row's code words instead of one
                                   * byte per row naming one of the tile's few distinct code rows */
    int spmv_sell;                /* 0.  1: saamge_amd_spmv / spmv64 build and use the SELL copy (tests of the SELL kernels) */
    int debug;                    /* 0: bit 0 iteration traces of the few-eigenpairs path, bit 1 operator format census on stderr,
                                   * bit 2 level tags in the kernel profile */
    int host_heap_pad_mb;         /* 256: the first hierarchy of the process asks glibc (mallopt) never to trim its heap, to serve
                                   * blocks up to 32 MB from it and to grow it in steps of this many MiB.  The setup's host tables
                                   * (some tens of MB per hierarchy, some of them copied to and from the device as pageable
                                   * memory) otherwise go back to the kernel with every hierarchy; unmapping pages the GPU driver
                                   * has registered stalled the process's queues for ~20 ms at the start of the next setup in
                                   * half of the processes (measured: DESIGN.md section 7.0).  0: the allocator is left alone. */
    int ae_order;                 /* 0: the agglomerate matrices of the few-eigenpairs path are ordered by the rank of the global dof
                                   * number (a lexicographic box: shortest extent fastest).  1: per agglomerate, where that order's
                                   * structural half bandwidth exceeds 51 and the agglomerate has at most 4096 rows, the level order
                                   * (Cuthill-McKee from a pseudo-peripheral root, two sweeps; the rule: saamge_amd/ae_order_model.py,
                                   * DESIGN.md section 4.8) is computed and taken if it is narrower -- for global numberings that
                                   * scatter an agglomerate's dofs (refined or generated meshes).  See saamge_amd_level_order_info. */
} saamge_amd_options;
void saamge_amd_options_default(saamge_amd_options *o);
void saamge_amd_set_options(const saamge_amd_options *o);
void saamge_amd_get_options(saamge_amd_options *o);

/* == MultilevelParameters, inc/ml.hpp:59-114 (+ the hidden defaults of src/ml.cpp:64-67) */
typedef struct saamge_amd_params {
    int num_coarsenings;                      /* levels - 1 */
    double theta[SAAMGE_AMD_MAX_LEVELS];      /* spectral tolerance per coarsening */
    int nu_relax[SAAMGE_AMD_MAX_LEVELS];      /* smoother: SAS polynomial of degree 3 nu + 1 */
    int nu_pro[SAAMGE_AMD_MAX_LEVELS];        /* prolongator smoothing degree (interp_smooth, src/interp.cpp:172-229); 0 = tentative */
    int avoid_ess_bdr_dofs;                   /* src/ml.cpp:64, always true in the reference */
    int testmesh;                             /* mltest fixture: ones-vector on AE 0, src/interp.cpp:510-524 */
    int coarse_solver;                        /* 0 auto (explicit dense inverse up to 8192 rows, else inner PCG); 1 direct = the reference's
                                               * coarse_direct (src/tg.cpp:990-996): dense inverse up to 16384 rows, beyond that block-
                                               * tridiagonal elimination over a level structure of the operator's graph; 2 inner PCG;
                                               * 3 block-tridiagonal elimination whatever the size */
    double coarse_rtol;                       /* inner PCG tolerance on (B r, r), un-squared */
    int coarse_max_iter;
    long long workspace_bytes;                /* dense AE matrices are processed in chunks of this size (default 32 GiB) */
    int keep_debug;                           /* keep eigenpairs / singular values for inspection */
    /* Multi-GPU, one process per GPU (reference: MPI ranks, src/process.cpp).  Every rank passes
     * the SAME global problem; the AEs of each level are split into `world` contiguous ranges,
     * a rank solves the local spectral problems (src/interp.cpp:387-556) of its range only and
     * the eigenvectors are all-gathered in place through `allgather` (buf is a device pointer;
     * rank r owns bytes [byte_off[r], byte_off[r+1]); return 0 on success).  The bench/tests
     * implement it with torch.distributed (nccl = RCCL on ROCm, gloo for rehearsals). */
    int rank, world;
    int (*allgather)(void *ctx, void *buf_dev, const long long *byte_off);
    void *allgather_ctx;
    /* Row-partitioned solve (reference: HypreParMatrix::Mult's halo exchange in every operator
     * application of src/tg.cpp:91-132, MPI_Allreduce of the inner products of
     * src/mfem_addons.cpp:106-248).  When both callbacks are set, levels with at least
     * dist_min_local_rows rows per rank are applied by contiguous row blocks: before each SpMV
     * the interface entries of the input vector travel through `alltoallv` (device buffers; the
     * part for / from rank r is [byte_off[r], byte_off[r+1]) ), inner products and the restricted
     * residual are summed with `allreduce_sum`, coarse corrections and the final solution come
     * back through `allgather`.  Smaller levels and the coarsest solve stay replicated.  Both
     * callbacks receive allgather_ctx.  comm_stream_ordered != 0 promises that the callbacks
     * enqueue their work on the hierarchy's stream (RCCL through torch.distributed on the same
     * stream), so the library does not synchronise the stream around them. */
    int (*allreduce_sum)(void *ctx, double *buf_dev, long long count);
    int (*alltoallv)(void *ctx, const void *send_dev, const long long *send_byte_off, void *recv_dev,
                     const long long *recv_byte_off);
    long long dist_min_local_rows;            /* default 262144 */
    int comm_stream_ordered;
    /* MultilevelParameters::use_correct_nullspace (inc/ml.hpp, default true in the reference's
     * drivers): one more two-grid level under the coarsest spectral operator, interp = scaling_P
     * (src/contrib.cpp:655-668, src/interp.cpp:842-909), SAS smoother nu = 3 (CorrectNullspace,
     * src/solve.cpp:52-164, src/ml.cpp:225-236).  Its own coarse solve (one BoomerAMG V-cycle in
     * the reference) is this library's coarsest solver.  Default 0. */
    int correct_nullspace;
    /* ContribTent::ExtendWithPolynomials / ExtendWithRBMs (src/contrib.cpp:302-436): extra modes
     * given per fine dof -- constants, coordinates, rigid-body modes: the caller evaluates them --
     * are restricted to every MIS and appended after the spectral columns before the SVD (finest
     * level only, like the reference).  n x num_extra_modes, column-major, host or device. */
    const double *extra_modes;
    int num_extra_modes;
    /* Element-free mode (tg_produce_data_algebraic / ExtractSubMatrices, src/tg.cpp:579-672,
     * :862-886): elements are the dofs, partitions[0] maps DOFS to (non-overlapping) AEs, the AE
     * matrices are principal submatrices of A made rowsum-free; pass NE = n, nde = 1,
     * elem_to_dof = elmat = bdr_dofs = NULL.  1 = ExtractSubMatrices; 2 = WindowSubMatrices
     * (src/tg.cpp:741-858, `use_window`): A_TT + A_TX E, outside neighbours replaced by the
     * row-weighted average of the inside ones. */
    int algebraic;
    /* MultilevelParameters::smooth_drop_tol (inc/ml.hpp:93-113; interp_smooth -> AltThreshold,
     * src/interp.cpp:89-229): entries of the SMOOTHED prolongator (nu_pro > 0) with
     * |value| <= tol are dropped before R = P^T and Ac = RAP.  0 = keep everything. */
    double smooth_drop_tol;
    /* MultilevelParameters::do_aggregates (inc/ml.hpp; src/ml.cpp:149): on the LAST coarsening the
     * minimal intersection sets are replaced by one aggregate per AE; dofs shared by several AEs
     * are distributed greedily by strength of connection (agg_construct_aggregate_mises,
     * src/aggregates.cpp:324-487; Arbitrator::suggest, src/arbitrator.cpp:93-204).  Lower
     * operator complexity on the coarsest level. */
    int do_aggregates;
    /* Local eigensolver (Eigensolver::SolveDirect -> dsygvx, src/spectral.cpp:124-237,
     * src/xpacks.cpp:222-314).  0 (default): few-eigenpairs path -- banded Cholesky + shift-invert
     * subspace iteration, the count #{lambda <= theta} certified by the inertia of C - theta I,
     * any batch that fails certification redone by the dense path; 1: dense path only (dsygvx's
     * own algorithm: reduction to tridiagonal form, Sturm counts, inverse iteration). */
    int eigensolver;
    /* Few-eigenpairs path: a Ritz pair is accepted when the bound of its residual || C x - lambda x || (C scaled to
     * lambda_max <= 1, like the reference's generalised problem, src/spectral.cpp:134) is at most eig_tol.  Default 1e-12:
     * an invariant subspace is then determined to eig_tol / gap (the reference's dsygvx delivers eps / gap), i.e. to
     * ~1e-8 for the 7e-5 gaps of BASELINE config 4 (theta = 1e-4).  Measured there (tests/test_gpu_baseline_sizes.py, the
     * well-posed config-4 golden): 1e-12, 1e-13 and 1e-14 give the same level dimensions, the same counts and the same PCG
     * history to 3 digits of its 6e-8 deviation from the oracle's -- that deviation comes from the singular vectors of the
     * smallest kept singular values, not from the eigenvectors.  Allowed: 1e-15 ... 1e-8. */
    double eig_tol;
    saamge_amd_options options;               /* what this hierarchy uses for its whole life (see saamge_amd_options) */
} saamge_amd_params;

void saamge_amd_params_default(saamge_amd_params *p);

/* ---- native collectives: RCCL over xGMI, one process per GPU (csrc/comm.hip) --------------------------------
 * Rank 0 draws a unique id and ships it to the other ranks by any means (MPI_Bcast, a file, torch.distributed's
 * store); every rank then creates its communicator on the stream its hierarchy will run on and installs it in
 * the parameters: rank, world and the three collectives are filled in, comm_stream_ordered = 1.  The stream MUST be
 * the one later given to saamge_amd_ml_produce_data (the collectives are ordered with the hierarchy's kernels only
 * there): a mismatch is an error of saamge_amd_ml_produce_data.  The allgather / allreduce_sum / alltoallv callbacks
 * remain the plug for MPI host codes. */
typedef struct saamge_amd_comm saamge_amd_comm;
int saamge_amd_comm_unique_id(char id[128]);
int saamge_amd_comm_create(int rank, int world, const char id[128], void *stream, saamge_amd_comm **out);
void saamge_amd_comm_destroy(saamge_amd_comm *c);
int saamge_amd_params_set_comm(saamge_amd_params *p, saamge_amd_comm *c);
/* one all-reduce, all-gather and all-to-all of known data, checked: 0 = the communicator works */
int saamge_amd_comm_selftest(saamge_amd_comm *c);
const char *saamge_amd_comm_last_error(void);
/* hipMemcpy(hipMemcpyDefault) helper for all-gather callbacks written outside C (host or device
 * pointers on either side) */
int saamge_amd_memcpy(void *dst, const void *src, long long bytes);
const char *saamge_amd_last_error(void);

/* ml_produce_data (inc/ml.hpp:192-194, src/ml.cpp:379-472) on raw arrays:
 *   A            n x n CSR, essential rows/cols eliminated with the diagonal kept
 *                (== HypreParMatrix Ag / SparseMatrix Al of test/mltest/mltest.cpp:619-621)
 *   elem_to_dof  NE x nde, elmat NE x nde x nde row-major raw element matrices
 *                (== ElementMatrixProvider::GetMatrix, inc/elmat.hpp:53-78)
 *   bdr_dofs     n flags (== fem_find_bdr_dofs, src/fem.cpp:87-140); may be NULL
 *   partitions   partitions[k][e] = AE of level-k element e (level-k elements are the
 *                level-(k-1) AEs); replaces METIS, exactly like the non-NULL
 *                `partitioning` argument of agg_create_partitioning_fine
 *                (inc/aggregates.hpp:385-390)
 *   nparts       nparts[k] = number of AEs of coarsening k
 *   stream       hipStream_t to run on (NULL = default stream)                          */
int saamge_amd_ml_produce_data(int n, const int *rowptr, const int *col, const double *val,
                               int NE, int nde, const int *elem_to_dof, const double *elmat,
                               const signed char *bdr_dofs, const int *const *partitions,
                               const int *nparts, const saamge_amd_params *params, void *stream,
                               saamge_amd_hierarchy **out);
/* The same with 64-bit row offsets, for an operator with more than 2^31 stored entries on one GPU (the
 * reference's HYPRE_Int is 32-bit and reaches such sizes only split over MPI ranks): Q2 elasticity on 96^3
 * elements has 4.2e9.  Column indices and dimensions stay 32-bit.  Inside the library every operator carries
 * 64-bit row offsets; the 32-bit entry widens its input on the device. */
int saamge_amd_ml_produce_data64(int n, const long long *rowptr, const int *col, const double *val,
                                 int NE, int nde, const int *elem_to_dof, const double *elmat,
                                 const signed char *bdr_dofs, const int *const *partitions,
                                 const int *nparts, const saamge_amd_params *params, void *stream,
                                 saamge_amd_hierarchy **out);
/* The same for a mesh whose elements have different numbers of dofs (hexes with prisms, tetrahedra or pyramids; a
 * variable-order space) -- the reference's elem_to_dof Table and ElementMatrixProvider::GetMatrix(e) of any size:
 *   elem_ptr     NE + 1 offsets, elem_ptr[0] = 0, at least one dof per element: element e has
 *                nd_e = elem_ptr[e+1] - elem_ptr[e] dofs
 *   elem_to_dof  elem_ptr[NE] dof ids, element e's at elem_ptr[e] ...
 *   elmat        the raw element matrices packed in element order: element e's nd_e x nd_e matrix, row-major, at
 *                sum_{f<e} nd_f^2 (a 64-bit offset)
 * Host or device pointers, as above; every other argument as in saamge_amd_ml_produce_data.  Malformed offsets
 * (elem_ptr[0] != 0, an empty element, decreasing offsets) and dofs out of range are refused (nonzero return,
 * saamge_amd_last_error) before anything reads through them.  Elements that all have the same size take exactly the
 * path of saamge_amd_ml_produce_data with that nde (the same hierarchy, bit for bit). */
int saamge_amd_ml_produce_data_mixed(int n, const int *rowptr, const int *col, const double *val,
                                     int NE, const int *elem_ptr, const int *elem_to_dof, const double *elmat,
                                     const signed char *bdr_dofs, const int *const *partitions,
                                     const int *nparts, const saamge_amd_params *params, void *stream,
                                     saamge_amd_hierarchy **out);
int saamge_amd_ml_produce_data_mixed64(int n, const long long *rowptr, const int *col, const double *val,
                                       int NE, const int *elem_ptr, const int *elem_to_dof, const double *elmat,
                                       const signed char *bdr_dofs, const int *const *partitions,
                                       const int *nparts, const saamge_amd_params *params, void *stream,
                                       saamge_amd_hierarchy **out);
/* ml_produce_data from PER-RANK inputs (one process per GPU; params->rank / world and the collectives set): what the
 * reference's multi-rank drivers pass (pmltest, amg/CMakeLists.txt:198-203; test/mltest/mltest.cpp:619-745):
 *   A            this rank's row block as a HypreParMatrix holds it -- hypre's ParCSR split (hypre_ParCSRMatrix: `diag` =
 *                the columns of the rank's own range with LOCAL indices, `offd` = the others, compressed, col_map_offd[c] =
 *                global column of offd column c; inc/SharedEntityCommunication.hpp:74-245 works on the same split).  Row
 *                blocks are contiguous and ordered by rank (row_starts, world + 1 entries, may be NULL); entries of a row
 *                may come in any order.
 *   elem_to_dof  NE_local x nde, GLOBAL (true) dof ids -- the reference's local dofs mapped through Dof_TrueDof;
 *   elmat        the matrices of the rank's OWN elements: they stay on this rank and are never exchanged;
 *   bdr_dofs     flags of the rank's own rows (A->nrows of them; may be NULL);
 *   partitions   partitions[0][e] = local agglomerate (0 .. nparts_local[0] - 1) of local element e; partitions[k], k > 0,
 *                maps the rank's level-(k-1) agglomerates to its level-k agglomerates: no agglomerate straddles ranks
 *                (the reference's invariant, src/aggregates.cpp:1340-1443).
 * Global numbering = rank order (rank 0's elements / agglomerates first).  The hierarchy is identical to the one
 * saamge_amd_ml_produce_data builds from the assembled global problem.  A rank assembles, factors and coarsens the
 * agglomerates made of its own elements; round 4: the operator's rows and the integer topology are all-gathered inside
 * (DESIGN.md section 6 lists what is replicated), the element matrices are not.  Host or device pointers. */
typedef struct saamge_amd_parcsr {
    long long global_rows;              /* 0 = the sum of the ranks' rows */
    const long long *row_starts;        /* world + 1 entries, or NULL */
    int nrows;                          /* rows of this rank */
    const int *diag_i, *diag_j;         /* nrows x nrows */
    const double *diag_a;
    const int *offd_i, *offd_j;         /* nrows x num_cols_offd; offd_i may be NULL when num_cols_offd == 0 */
    const double *offd_a;
    int num_cols_offd;
    const long long *col_map_offd;
} saamge_amd_parcsr;
int saamge_amd_ml_produce_data_parcsr(const saamge_amd_parcsr *A, int NE_local, int nde, const int *elem_to_dof,
                                      const double *elmat, const signed char *bdr_dofs, const int *const *partitions,
                                      const int *nparts_local, const saamge_amd_params *params, void *stream,
                                      saamge_amd_hierarchy **out);
/* adapt_update_operators(A, ml_data, mlp, resmooth_interp = true), src/adapt.cpp:188-219: the
 * matrix values changed (same sparsity and topology): every interpolation is kept -- no local
 * eigenproblem is solved again --, smoother diagonals, smoothed prolongators (nu_pro > 0), all
 * Galerkin operators and the coarsest solver are rebuilt.  new_val: nnz(A) values in the order
 * given at setup (host or device); NULL if the caller changed its device array in place. */
int saamge_amd_update_operators(saamge_amd_hierarchy *h, const double *new_val);
/* tg_update_coarse_operator(A, tg_data, perform_solve_init, coarse_direct), inc/tg.hpp:610-612: the same update with
 * the coarsest solver chosen again -- coarse_solver with the meaning of the params field of that name: 1 = the
 * reference's coarse_direct = true, 2 = its CG on the coarsest operator; -1 keeps the kind in
 * place: the one the hierarchy was built with, or the one the last call with 1 or 2 chose. */
int saamge_amd_update_operators2(saamge_amd_hierarchy *h, const double *new_val, int coarse_solver);
/* ml_free_data, inc/ml.hpp:196 */
void saamge_amd_ml_free_data(saamge_amd_hierarchy *h);

/* VCycleSolver::Mult with iterative_mode = false (inc/solve.hpp:129-143,
 * src/solve.cpp:309-323 -> tg_cycle_atb src/tg.cpp:91-132): x = B b */
int saamge_amd_vcycle_mult(saamge_amd_hierarchy *h, const double *b, double *x);
/* VCycleSolver::Mult for either iterative_mode (src/solve.cpp:309-323): iterative_mode != 0 keeps the
 * caller's x as the start vector, x <- x + B (b - A x) (the cycle is a stationary linear iteration, so this
 * equals tg_cycle_atb started from x). */
int saamge_amd_vcycle(saamge_amd_hierarchy *h, const double *b, double *x, int iterative_mode);
/* tg_data_t::coarse_solver (inc/tg_data.hpp:71; assigned by callers, e.g. test/algebraic/algebraic.cpp:282-283;
 * invoked as coarse_solver.Mult(RESC, XC) with XC pre-zeroed, src/tg.cpp:110-126): replaces the library's
 * coarsest solve by a host callback, xc = solve(rc) on `n` = coarsest dimension host doubles; return 0 on
 * success.  NULL restores the built-in solver. */
typedef int (*saamge_amd_coarse_solve_fn)(void *ctx, int n, const double *rc_host, double *xc_host);
int saamge_amd_set_coarse_solver(saamge_amd_hierarchy *h, saamge_amd_coarse_solve_fn fn, void *ctx);
/* The smoother plug of the cycle: typedef void (*smpr_ft)(HypreParMatrix& A, const Vector& b, Vector& x, void *data)
 * (inc/smpr.hpp:59-60), selected per tg_data_t through the TG options pre_smoother / post_smoother (inc/tg.hpp:99-119,
 * copied at src/tg.cpp:411-414) and called by tg_cycle_atb as pre_smoother(A, b, x, data) ... post_smoother(A, b, x, data)
 * (src/tg.cpp:113,131) with the semantics x += M^-1 (b - A x).  Here: host callbacks on `n` = rows of the level's
 * operator; the library copies b and x to the host, calls, and copies x back (pre-smoothing of a cycle from a zero
 * start vector hands over x = 0).  NULL for either restores the built-in polynomial smoother (smpr_sym_poly) in that
 * place.  A level that is row-partitioned over several ranks refuses a plug (error at the cycle).  Return 0 on success. */
typedef int (*saamge_amd_smoother_fn)(void *ctx, int level, int n, const double *b_host, double *x_host);
int saamge_amd_set_smoother(saamge_amd_hierarchy *h, int level, saamge_amd_smoother_fn pre, saamge_amd_smoother_fn post,
                            void *ctx);
/* smpr_sym_poly on one level (inc/smpr.hpp:59-60, src/smpr.cpp:213-234): x += M^-1 (b - A x) */
int saamge_amd_smoother(saamge_amd_hierarchy *h, int level, const double *b, double *x);
/* Outer Krylov loop: MFEM CGSolver as driven by test/mltest/mltest.cpp:773-781
 * (squared_tol = 1: stop when (B r,r) < max(rel_tol^2 (B r0,r0), abs_tol^2)) or
 * kalchev_pcg, inc/mfem_addons.hpp:276 (squared_tol = 0).  hist (host, max_iter+1
 * doubles, may be NULL) receives (B r_k, r_k).  zero_guess != 0 starts from x = 0. */
int saamge_amd_pcg(saamge_amd_hierarchy *h, const double *b, double *x, double rel_tol,
                   double abs_tol, int max_iter, int squared_tol, int zero_guess, int *iters,
                   int *converged, double *hist);

/* ---- inspection (ml_print_dims / tg_data_t field access, src/ml.cpp:296-355) ---- */
int saamge_amd_num_levels(const saamge_amd_hierarchy *h); /* number of operators = coarsenings + 1 */
/* info[0]=rows(A_l) [1]=nnz(A_l) [2]=nparts [3]=num_mises [4]=coarse dim [5]=nnz(P) [6]=nnz(Ac)
 * [7]=total eigenvectors [8]=inner PCG iterations of the last coarsest solve
 * [12]=1 if the level is row-partitioned [13]=first own row [14]=own rows [15]=halo entries received */
int saamge_amd_level_info(const saamge_amd_hierarchy *h, int level, long long info[16]);
/* The coarsest solver IN USE (a direct request that could not be served -- a level set beyond the block limit, a
 * non-positive pivot -- ends in the inner PCG; this tells): info[0] = 1 explicit dense inverse, 2 inner PCG, 3 block-
 * tridiagonal elimination, 0 the caller's plug (saamge_amd_set_coarse_solver); [1] = rows of the coarsest operator;
 * [2] = blocks and [3] = rows of the largest block of the block-tridiagonal structure (kind 3, else 0); [4] = doubles held
 * in the explicit inverses (kind 1: n^2, kind 3: sum n_k^2); [5..7] = 0. */
int saamge_amd_coarse_solver_info(const saamge_amd_hierarchy *h, long long info[8]);
/* Storage formats of the level operator's SELL-64 copy (no reference counterpart: hypre keeps CSR): info[0..2] = slices
 * that are pair-coded / offset-coded / plain, [3..5] = their stored entries, [6] = 256-row tiles whose x-segments are
 * staged through LDS, [7] = bytes of matrix data one application streams in these formats, [8] = pairs of the operator-level
 * (offset, value) dictionary that replaces the plain slices' columns and values by 16-bit codes (0: none), [9] = 1 if the
 * lanes of a 3 x 3 node block share their gathers of x, [10] = rows outside regular node blocks, [11] = local eigenproblems this rank SOLVED on the level (its other
 * agglomerates are bitwise identical to one of those and received a copy: saamge_amd_options.eig_dedupe). */
int saamge_amd_level_format(const saamge_amd_hierarchy *h, int level, long long info[12]);
/* The local order of the level's agglomerate matrices (saamge_amd_options.ae_order), over the agglomerates whose matrices were
 * given a permutation (the few-eigenpairs path): info[0] = their number, [1] = those that took the level order, [2] = the
 * largest structural half bandwidth of the rank / box order, [3] = the largest of the order in use.  With ae_order = 0 the
 * setup measures nothing: this call then measures the rank / box order of those agglomerates ([1] = 0, [3] = [2]). */
int saamge_amd_level_order_info(const saamge_amd_hierarchy *h, int level, long long info[4]);
/* which: 0 A_l, 1 interp, 2 restr, 3 Ac (host output buffers sized from level_info) */
int saamge_amd_get_csr(const saamge_amd_hierarchy *h, int level, int which, int *rowptr, int *col,
                       double *val);       /* fails on an operator with more than 2^31 - 1 entries */
int saamge_amd_get_csr64(const saamge_amd_hierarchy *h, int level, int which, long long *rowptr, int *col,
                         double *val);
/* which: 0 AE_to_dof, 1 dof_to_AE, 2 mis_to_dof, 3 mis_to_AE, 4 AE_to_mis, 5 elem_to_dof.
 * Pass I = J = NULL to query sizes: *nrows, *nconn. */
int saamge_amd_get_table(const saamge_amd_hierarchy *h, int level, int which, int *nrows,
                         long long *nconn, int *I, int *J);
/* per-dof MIS id (n), per-MIS kept vectors / SVD columns (num_mises), agg_flags (n) */
int saamge_amd_get_mis(const saamge_amd_hierarchy *h, int level, int *mises, int *mis_k,
                       int *mis_ncols, signed char *agg_flags);
/* keep_debug only: eigenvector counts per AE (nparts), packed eigenvalues / eigenvectors
 * (AE i: n_i x m_i column-major, AEs concatenated); sizes via level_info[7] and tables. */
int saamge_amd_get_ae_eigens(const saamge_amd_hierarchy *h, int level, int *ae_m, double *evals,
                             double *evecs, double *ae_D);
/* keep_debug only: packed per-MIS singular values (sum of SVD input columns before dropping) and
 * tentative blocks (MIS m: r_m x k_m column-major, concatenated). */
int saamge_amd_get_mis_svd(const saamge_amd_hierarchy *h, int level, long long *sig_off,
                           double *sig, double *U);

/* ---- operator-level entry points (the same kernels, usable on their own) ---- */
/* y = A x, hypre ParCSRMatrixMatvec as used by src/tg.cpp:115 */
int saamge_amd_spmv(int nrows, int ncols, const int *rowptr, const int *col, const double *val,
                    const double *x, double *y);
int saamge_amd_spmv64(int nrows, int ncols, const long long *rowptr, const int *col, const double *val,
                      const double *x, double *y);
/* xpacks_calc_lower_eigens_dense batched (src/xpacks.cpp:222-314) for A x = lambda D x with
 * diagonal D: matrices packed column-major one after the other, D packed likewise.
 * Outputs (host): m[i]; evals at offset sum_{j<i} n_j; evecs at offset sum_{j<i} n_j^2
 * (first m[i] columns), D-orthonormal. */
int saamge_amd_lower_eigens_batched(int count, const int *n, const double *A, const double *D,
                                    double vl, double vu, int *m, double *evals, double *evecs);

/* The certificate of the few-eigenpairs path on its own: neg[i] = number of eigenvalues of
 * A_i x = lambda D_i x below vu, from the inertia of D^-1/2 A D^-1/2 - vu I (banded L S L^T without
 * pivoting; Sylvester) -- what dsygvx obtains from dstebz's Sturm counts (src/xpacks.cpp:226-268).
 * -1: a pivot was too small for the count to be trusted (the setup then takes the dense path).
 * Same packing as saamge_amd_lower_eigens_batched. */
int saamge_amd_inertia_batched(int count, const int *n, const double *A, const double *D, double vu,
                               int *neg);

/* ---- the general sparse products of the smoothed prolongator on their own (csrc/spgemm.hip; tests) ----
 * Host CSR arrays in (32-bit offsets; every row with distinct columns, in any order), the result on the host with every row
 * sorted by column.  Sizes: a call with Ccol = Cval = NULL returns the row offsets (nrows + 1) and *nnz only.
 * C = beta E + alpha diag(d) A B with A nrows x ninner, B ninner x ncols, E nrows x ncols or NULL, d (nrows) or NULL.  E given
 * as B's own three arrays (A square) is the same matrix on the device too.  The structure of C is the structural product
 * (entries that cancel stay).  *route: 0, 1, 2 = the hash-table product and the table tier (256, 2048, 8192 slots) that held
 * every row; 3 = the dense-B product; -1 = no kernel ran (no rows) or the product was refused. */
int saamge_amd_spgemm(int nrows, int ninner, int ncols, const int *Arow, const int *Acol, const double *Aval,
                      const int *Brow, const int *Bcol, const double *Bval, const int *Erow, const int *Ecol,
                      const double *Eval, const double *d, double alpha, double beta, int *Crow, long long *Cnnz,
                      int *Ccol, double *Cval, int *route);
/* ---- the local order of the agglomerate matrices on its own (csrc/assemble.hip; tests) ----
 * Host arrays.  A mesh (NE elements; elem_ptr NULL: nde dofs each, else NE + 1 offsets into elem_to_dof; dofs in [0, ND)) and an
 * element -> agglomerate map (values in [0, nparts), no agglomerate empty).  The relation tables are built as the setup builds
 * them.  Out: ae_ptr (nparts + 1) and *nconn always; with ae_to_dof and pos given (nconn entries each) the agglomerates' dofs
 * in table order, the position of each in its agglomerate's matrix, and per agglomerate bw0 (structural half bandwidth of the
 * rank / box order), bw (of the order in use) and choice (1: the level order).  mode: saamge_amd_options.ae_order (0: positions
 * of the rank / box order, choice 0; other values are refused).  Agglomerates of at most 8192 rows. */
int saamge_amd_ae_order(int ND, int NE, int nde, const int *elem_ptr, const int *elem_to_dof, const int *elem_to_ae,
                        int nparts, int mode, int *ae_ptr, long long *nconn, int *ae_to_dof, int *pos, int *bw0, int *bw,
                        int *choice);
/* ---- element matrices computed on the device (csrc/elmat.hip) ----
 * The standard order-1 and tensor-product order-2 element matrices from vertex coordinates, element -> vertex lists and per-element coefficients, written
 * in the packed layout saamge_amd_operator_assemble and saamge_amd_ml_produce_data* take (element e: size_e x size_e row-major
 * at sum_{f<e} size_f^2), so that the physics never exists on the host; saamge_amd/elmat_model.py defines every operation and
 * the device gives the same bits.  Types by (dim, nodes): (2, 3) P1 triangle, (2, 4) Q1 quadrilateral
 * (v00, v10, v11, v01), (3, 4) P1 tetrahedron, (3, 6) P1 x P1 wedge (bottom triangle, then top), (3, 8) Q1 hexahedron (MFEM's
 * vertex order); one quadrature rule per type, exact on affine images.
 * Order 2: (2, 9) Q2 quadrilateral, nodes in MFEM's H1 order (the vertices v00, v10, v11, v01, the edge midpoints bottom, right,
 * top, left, the centre), and (3, 27) Q2 hexahedron, nodes lexicographic (node (iz * 3 + iy) * 3 + ix).  The node order is an
 * input convention: the dof lists follow it, a caller with another order permutes its node lists and nothing else.  For these
 * coords holds ALL nodes (NV of them) and the lists hold 9 / 27 node ids; the geometry is isoparametric (the Jacobian runs over
 * all nodes, so an element may be curved; a straight-sided one has its extra nodes at the averages of its corners).  Rule: 3
 * Gauss points per axis, exact for both forms on parallelepipeds.  One list (elem_ptr) may hold elements of both orders.
 * Order-2 simplices: (2, 6) P2 triangle, nodes = the vertices 0, 1, 2, then the midpoints of the edges (0,1), (1,2), (2,0); and
 * (3, 10) P2 tetrahedron, nodes = the vertices 0 .. 3, then the midpoints of the edges (0,1), (0,2), (0,3), (1,2), (1,3), (2,3)
 * (believed to be MFEM's H1 order-2 orders; not verified against MFEM, this table is the definition).  Isoparametric like the
 * other order-2 types: coords holds all nodes, an element may be curved, a straight-sided one has its midside nodes at
 * 0.5 * (a + b).  Shape functions on the barycentric coordinates L: vertex i L_i (2 L_i - 1), edge (i, j) 4 L_i L_j.  Rules: the
 * 3-point degree-2 rule on the triangle, the 4-point degree-2 rule on the tetrahedron, exact for both forms on affine images.
 * kind 0 diffusion: ncoef = 1 (c I), dim (diagonal) or dim (dim + 1) / 2 (symmetric: xx, yy, zz, xy, yz, xz / xx, yy, xy), the
 * matrix nodes x nodes.  kind 1 elasticity (lambda div u div v + 2 mu eps(u):eps(v)): ncoef = 2 (lambda, mu), dof
 * dim * node + component, the matrix (dim nodes) x (dim nodes).
 * kind 0 diffusion, 1 elasticity; dim 2 or 3; elem_ptr NULL: nde vertices per element.
 * coords NV x dim row-major, coef NE x ncoef; elmat_out sized by the caller (sizes: call with elmat_out = NULL);
 * dof_ptr_out (NE + 1) / elem_to_dof_out: the dof lists the matrices are indexed by (kind 0: the vertex lists;
 * kind 1: dim * vertex + component), may be NULL.  Any pointer host or device, each on its own.
 * info[0..4] = triangles, quadrilaterals, tetrahedra, wedges, hexahedra; [5] = doubles written; [6] = first element
 * with a non-positive Jacobian (-1: none); [7] = order-2 elements (9-node quadrilaterals, 27-node hexahedra, 6-node triangles,
 * 10-node tetrahedra; [0..4] count the order-1 elements only).
 * Refused (nonzero return, saamge_amd_last_error names the argument or the first element; elmat_out is then not to be relied
 * on): dim, kind or ncoef out of range, NULL coords / elem_to_vertex / coef, malformed offsets, a vertex id outside [0, NV), an
 * element that lists a vertex twice, a node count that is no type of the dimension, an element whose Jacobian determinant is
 * not positive at a quadrature point.  The checks of the arguments alone run before anything touches the device. */
int saamge_amd_element_matrices(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                const int *elem_to_vertex, int kind, int ncoef, const double *coef, void *stream,
                                double *elmat_out, int *dof_ptr_out, int *elem_to_dof_out, long long info[8]);
/* ---- mass matrices and load vectors computed on the device (csrc/elmat.hip) ----
 * The zeroth-order forms on the types, node orders and isoparametric geometry of saamge_amd_element_matrices, so that the
 * right-hand side and sigma M + K never exist on the host either; saamge_amd/elmat_model.py (element_mass, element_loads)
 * defines every operation and the device gives the same bits.  The rule of a type is its rule above, except three points on the
 * triangle and four on the tetrahedron (exact for the P1 mass on affine simplices), and on the order-2 simplices a 6-point
 * degree-4 rule (6-node triangle) and a 14-point degree-5 rule (10-node tetrahedron), positive weights, interior points, exact
 * for the P2 mass on affine simplices -- so a curved element may be refused here at a point the stiffness rule does not have.
 * info[0..4] and [7] as above ([7] counts all four order-2 types).  vdim 1: one dof per node; vdim = dim: dof
 * dim * node + component, the layout of elasticity.  coef: NE doubles, c of (c u, v).
 * saamge_amd_element_mass: elmat_inout in the packed layout above (element e: size_e x size_e at sum_{f<e} size_f^2, size_e =
 * vdim * nodes); the components do not couple (an entry between two components is + 0.0).  accumulate != 0: the matrices are
 * ADDED to what elmat_inout holds, one addition per entry -- K + sigma M from the output of saamge_amd_element_matrices of
 * the same mesh and layout, with sigma in coef.  elmat_inout NULL (accumulate 0): the sizes only.
 * saamge_amd_element_loads: src NV x vdim, the source at the nodes; coef NULL: 1.  elvec_out packed, element e: size_e doubles at
 * sum_{f<e} size_f (NULL: the sizes only); saamge_amd_operator_assemble_rhs takes it.
 * Any pointer host or device, each on its own.  info as above, [5] = doubles written.
 * Refused, before anything touches the device: vdim not 1 or dim, NULL coef for the mass, NULL src, accumulate with NULL
 * elmat_inout; and everything saamge_amd_element_matrices refuses of the mesh, the first element with a non-positive Jacobian
 * determinant at a point of the mass rule in info[6]. */
int saamge_amd_element_mass(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                            const int *elem_to_vertex, int vdim, const double *coef, void *stream, int accumulate,
                            double *elmat_inout, long long info[8]);
int saamge_amd_element_loads(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                             const int *elem_to_vertex, int vdim, const double *coef, const double *src, void *stream,
                             double *elvec_out, long long info[8]);
/* ---- data at the points of the mass rule (csrc/elmat.hip) ----
 * The points of an element are those of its type's MASS rule (the rule saamge_amd_element_mass / _loads integrate with), in the
 * rule's order: point q of element e has the global index qp_ptr[e] + q, qp_ptr NE + 1 offsets of 64 bits, NQ = qp_ptr[NE].
 * saamge_amd/elmat_model.py (element_points, element_eval, element_loads_points, element_errors) defines every operation and
 * the device gives the same bits.  The shared arguments, the pointers (host or device, each on its own), the stream and
 * info[0..4], [7] as for saamge_amd_element_loads; info[5] = NQ, [6] = the first element with a non-positive determinant (-1:
 * none).  A refusal writes no output.
 * saamge_amd_element_points: qp_ptr_out (NE + 1), xq_out (NQ x dim) the physical coordinates x_q[i] = sum_a N_a(q) X[a][i], the
 * nodes ascending; wdet_out (NQ) weight_q * det J_q.  Any of the three may be NULL.
 * saamge_amd_element_eval: u NV x vdim at the nodes; uq_out (NQ x vdim) sum_a N_a u[a][i]; gradq_out (NQ x vdim x dim), entry
 * (i, j) the derivative of component i along x_j: r[i][k] = sum_a u[a][i] dN_a[k], then (sum_k r[i][k] C[j][k]) / det with the
 * cofactors C of the Jacobian, the division last.  Either output may be NULL.
 * saamge_amd_element_loads_points: fq NQ x vdim, the source AT THE POINTS; coef NE doubles or NULL: 1.  Entry (a, i) is the sum
 * over the points, ascending from 0.0, of (s fq[q][i]) N_a, s = (w det) coef[e]; elvec_out in the packed layout of
 * saamge_amd_element_loads (saamge_amd_operator_assemble_rhs takes it), NULL: the checks only.  A coefficient that varies inside
 * an element is folded into fq by the caller.
 * saamge_amd_element_errors: u NV x vdim, exq NQ x vdim and exgradq NQ x vdim x dim the exact values / gradients at the points
 * (either may be NULL); err_out NE x 2: column 0 sum_q wdet_q sum_i (uq_i - exq_i)^2, column 1 the same of the gradients over
 * (i, j); a column whose exact data is NULL is 0.0.  The entries are SQUARES of the element contributions: the caller sums
 * them and takes the root -- the library forms no total, so no order of execution enters a result.
 * Refused, in this order: vdim not 1 or dim, NULL coords / elem_to_vertex; everything saamge_amd_element_loads refuses of the
 * mesh; NULL u (eval, errors) or NULL fq (loads_points); the first element with a non-positive Jacobian determinant at a point
 * of the mass rule (info[6]).  The calls with optional outputs are not refused when all of them are NULL: the mesh and the
 * determinants are checked and info is filled. */
int saamge_amd_element_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                              const int *elem_to_vertex, void *stream, long long *qp_ptr_out, double *xq_out, double *wdet_out,
                              long long info[8]);
int saamge_amd_element_eval(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                            const int *elem_to_vertex, int vdim, const double *u, void *stream, double *uq_out, double *gradq_out,
                            long long info[8]);
int saamge_amd_element_loads_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                    const int *elem_to_vertex, int vdim, const double *coef, const double *fq, void *stream,
                                    double *elvec_out, long long info[8]);
int saamge_amd_element_errors(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                              const int *elem_to_vertex, int vdim, const double *u, const double *exq, const double *exgradq,
                              void *stream, double *err_out, long long info[8]);
/* ---- coefficients at the points: element matrices with k(x), sigma(x) given inside the elements (csrc/elmat.hip; DESIGN.md
 * section 4.9.6) ----
 * saamge_amd_element_matrices and saamge_amd_element_mass with a coefficient row per POINT in the place of one per element:
 * coefq has NQ rows, row qp_ptr[e] + q belongs to point q of element e -- the indexing of saamge_amd_element_points / _eval, so
 * that k(u_q) formed from the output of saamge_amd_element_eval goes in as it is.  saamge_amd/elmat_model.py
 * (element_matrices_points, element_mass_points) defines every operation and the device gives the same bits.
 * THE RULE of both calls is the type's MASS rule: the stiffness forms are integrated at the points of the mass rule here.  For
 * the quadrilateral, the hexahedron, the wedge and the 9-node / 27-node types that is the rule of saamge_amd_element_matrices
 * (equal coefficients at the points of an element give its bits); the triangle has 3 points here against 1 and the tetrahedron 4
 * against 1 (the tetrahedron still gives the same bits, the triangle agrees to rounding), the 6-node triangle 6 against 3 and the
 * 10-node tetrahedron 14 against 4: these agree to rounding with saamge_amd_element_matrices on affine elements and differ by the
 * quadrature on curved ones, and a CURVED 6-node triangle or 10-node tetrahedron can be refused here for a non-positive
 * determinant at a point saamge_amd_element_matrices does not have.
 * saamge_amd_element_matrices_points: coefq NQ x ncoef row-major; kind, ncoef, the outputs (elmat_out NULL: the sizes only; the
 * dof lists), info and the refusals are those of saamge_amd_element_matrices, with coefq in the place of coef.  Per point, kind
 * 0: F_a = K_q G_a with K_q from the point's row; kind 1: lambda_q, mu_q of the point's row.
 * saamge_amd_element_mass_points: coefq NQ doubles, s = (w det) coefq[qp_ptr[e] + q]; vdim, accumulate, elmat_inout, info and the
 * refusals are those of saamge_amd_element_mass -- K(u) + sigma(u) M by a call of each with accumulate.
 * Any pointer host or device, each on its own.  The checks of the arguments alone run before anything touches the device; the
 * first element with a non-positive determinant is reported in info[6] and the output is then not to be relied on. */
int saamge_amd_element_matrices_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                       const int *elem_to_vertex, int kind, int ncoef, const double *coefq /* NQ x ncoef */,
                                       void *stream, double *elmat_out, int *dof_ptr_out, int *elem_to_dof_out, long long info[8]);
int saamge_amd_element_mass_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                   const int *elem_to_vertex, int vdim, const double *coefq /* NQ */, void *stream, int accumulate,
                                   double *elmat_inout, long long info[8]);
/* ---- boundary forms computed on the device (csrc/elmat.hip) ----
 * The face mass (Robin: (c u, v) over faces) and the face loads (Neumann: (c g, v) over faces) of a list of NF faces, ADDED into
 * the packed matrices / vectors of the owning elements, so that the element matrices still sum to the operator and everything
 * downstream (saamge_amd_operator_assemble, _assemble_rhs, saamge_amd_ml_produce_data*) takes them unchanged;
 * saamge_amd/elmat_model.py (FACE_NODES, boundary_mass, boundary_loads) defines every operation and the device gives the same
 * bits.  Face f is the local face face_local[f] of element face_elem[f]; local faces by element type, as the element's local
 * node ids: triangle (0,1) (1,2) (2,0); quadrilateral (0,1) (1,2) (2,3) (3,0); 9-node quadrilateral (0,4,1) (1,5,2) (2,6,3)
 * (3,7,0); tetrahedron (1,2,3) (0,3,2) (0,1,3) (0,2,1); wedge (0,2,1) (3,4,5) (0,1,4,3) (1,2,5,4) (2,0,3,5); hexahedron (3,2,1,0)
 * (0,1,5,4) (1,2,6,5) (2,3,7,6) (3,0,4,7) (4,5,6,7); 27-node hexahedron: the same six faces with their 9 nodes; 6-node
 * triangle: the 3-node segments (0,3,1) (1,4,2) (2,5,0); 10-node tetrahedron: the tetrahedron's four faces as 6-node triangles
 * (three vertices, then the midpoints of (v0,v1), (v1,v2), (v2,v0)): (1,2,3,7,9,8) (0,3,2,6,9,5) (0,1,3,4,8,6) (0,2,1,5,7,4); a
 * 6-node triangular face has the shape functions of the 6-node triangle and its 6-point rule.  The call does
 * not know what a boundary is: interior faces are allowed.  coef: NF doubles, c per face.  The faces of one element are added
 * in ascending local face index, whatever the order of the list; entries that no listed face touches keep their bits.
 * saamge_amd_boundary_mass: elmat_inout holds the matrices of saamge_amd_element_matrices / _mass of the same mesh and vdim;
 * vdim = dim adds the face entry to ((a, i), (b, i)) of every component i.
 * saamge_amd_boundary_loads: g NV x vdim, the data at the nodes; coef NULL: 1; elvec_inout holds the vectors of
 * saamge_amd_element_loads.  Data that jumps across an edge: one call per side with its own g, the calls accumulate.
 * elmat_inout / elvec_inout NULL: the checks and info only.  Any pointer host or device, each on its own.  NF = 0: nothing.
 * info[0..4] = faces by type: 2-node segments, 3-node segments (whichever element type owns them), triangles (of 3 and of 6
 * nodes), 4-node quadrilaterals, 9-node quadrilaterals;
 * [5] = additions made (a double that two faces touch counts twice); [6] = first refused face (-1: none); [7] = distinct
 * elements touched.
 * Refused, before anything touches the device: vdim not 1 or dim, NF < 0, NULL face lists, NULL coef for the mass, NULL g;
 * then everything saamge_amd_element_mass refuses of the mesh; then the first face of the list with face_elem outside [0, NE) or
 * face_local outside the range of the element's type; then the first face whose (element, local face) the list holds more than
 * once; then the first face whose measure is not positive at a point of its rule. */
int saamge_amd_boundary_mass(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                             const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim,
                             const double *coef, void *stream, double *elmat_inout, long long info[8]);
int saamge_amd_boundary_loads(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                              const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim,
                              const double *coef, const double *g, void *stream, double *elvec_inout, long long info[8]);
/* ---- boundary data at the face points (csrc/elmat.hip) ----
 * What saamge_amd_element_points / _eval / _loads_points / _mass_points give inside the elements, on a list of faces: where the
 * face points are and the outward normal there, a nodal field and its whole gradient there, the Robin term with a coefficient
 * per point and the Neumann term of data given at the points -- so that a flux g = k grad u . n, a nonlinear alpha(u) or a
 * boundary flux is formed on the device.  saamge_amd/elmat_model.py (boundary_points, boundary_eval, boundary_mass_points,
 * boundary_loads_points) defines every operation and the device gives the same bits.  Everything not said here is as for the
 * boundary forms above: the face lists, the local faces, the rule of a face type, the pointers (host or device, each on its
 * own), the stream, info[0..4], [6], [7].
 * THE POINTS of face f of the list are those of its face type's rule, in the rule's order: point q of face f has the global
 * index fp_ptr[f] + q, fp_ptr NF + 1 offsets of 64 bits, NFQ = fp_ptr[NF].  The index follows the order of the LIST: a permuted
 * list permutes the point arrays by whole faces (and leaves the matrices and vectors as they are).
 * saamge_amd_boundary_points: fp_ptr_out (NF + 1); xq_out (NFQ x dim), x_q[i] = sum_c N_c(q) X[c][i] over the face nodes
 * ascending; wmeas_out (NFQ), w_q meas_q; normal_out (NFQ x dim), the unit normal that points out of the owning element: in 3D
 * (t_0 x t_1) / meas with the tangents t_j = sum_c X[c] dN_c[j], in 2D (t_y, -t_x) / meas, the division last.  Any of the four
 * may be NULL.  info[5] = NFQ.
 * saamge_amd_boundary_eval: u NV x vdim at the nodes.  uq_out (NFQ x vdim) is the trace through the face's own shape functions,
 * sum_c N_c u[c][i] over the face nodes.  gradq_out (NFQ x vdim x dim) is the WHOLE gradient of the owning element's field at the
 * face point, not its tangential part: the element's dN_a of all its nodes at the reference position of the face point, J, the
 * cofactors and (sum_k r[i][k] C[j][k]) / det as saamge_amd_element_eval.  Either output may be NULL; info[5] = NFQ.  The
 * element's determinant is checked at every face point whether or not gradq_out is given.
 * saamge_amd_boundary_mass_points: saamge_amd_boundary_mass with s = (w meas) coefq[fp_ptr[f] + q], coefq NFQ doubles; equal
 * values at the points of each face give the bits of saamge_amd_boundary_mass.  info[5] = additions made.
 * saamge_amd_boundary_loads_points: gq NFQ x vdim, the data AT THE POINTS; coef NF doubles or NULL: 1.  Face dof (a, i) gets the
 * sum over the points, ascending from 0.0, of (s gq[q][i]) N_a, s = (w meas) coef[f], added as saamge_amd_boundary_loads adds.
 * With gq = the uq_out of saamge_amd_boundary_eval of a nodal g the result has the bits of saamge_amd_boundary_loads(g).  Data
 * that jumps across an edge of a box (a flux through n) takes ONE call.
 * Refused, in this order: vdim not 1 or dim; NF < 0; NULL face lists, NULL coefq / gq / u -- before anything touches the device;
 * the mesh; the first face out of range; the first repeated (element, local face); the first face whose measure is not positive;
 * for saamge_amd_boundary_eval the first face (lowest index of the list) whose element has a non-positive determinant at a face
 * point.  A refusal writes no output: every face is checked before the first kernel that writes. */
int saamge_amd_boundary_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                               const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, void *stream,
                               long long *fp_ptr_out, double *xq_out, double *wmeas_out, double *normal_out, long long info[8]);
int saamge_amd_boundary_eval(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                             const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim,
                             const double *u, void *stream, double *uq_out, double *gradq_out, long long info[8]);
int saamge_amd_boundary_mass_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                    const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim,
                                    const double *coefq /* NFQ */, void *stream, double *elmat_inout, long long info[8]);
int saamge_amd_boundary_loads_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                     const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim,
                                     const double *coef /* NF or NULL */, const double *gq /* NFQ x vdim */, void *stream,
                                     double *elvec_inout, long long info[8]);
/* ---- the faces of a mesh found on the device (csrc/mesh_faces.hip) ----
 * Which element lies across each local face, and from that the boundary face list the boundary forms take, the element graph
 * through faces that saamge_amd_partition_graph takes, and the essential-dof flags that saamge_amd_operator_assemble and
 * saamge_amd_ml_produce_data* take: saamge_amd/mesh_model.py defines every integer and the device gives the same.  Element types
 * and local faces are those of the boundary forms above.  A SLOT is (element, local face), s = slot_ptr[e] + lf.  The CORNERS
 * of a face: in 2D its first and last node; of a triangular face (3 or 6 nodes) its first three nodes, of a quadrilateral face
 * (4 or 9 nodes) its first four.  Two slots match when their sorted corner vertex ids are equal (midside and centre nodes take no
 * part: a hexahedron and a 27-node hexahedron on the same four vertices are neighbours).  One slot alone is a boundary face; three
 * or more on one corner set make the mesh non-manifold, which is refused.
 * saamge_amd_face_table_build: nbr_elem[s] / nbr_local[s] the element and local face across slot s (-1, -1: boundary); bdr_elem /
 * bdr_local the NB boundary faces ascending by (element, local face); xadj (NE + 1) / adj (nnz): row e the distinct elements
 * across the faces of e, ascending, no self loop.  info[0] = slots, [1] = interior pairs, [2] = boundary faces ([0] = 2 [1] + [2]),
 * [3] = graph entries, [4] = interior pairs whose two faces differ in their node count, [5] = the most elements at one vertex,
 * [6] = -1 or the lowest element with a non-manifold face (then only [0], [5], [6] are filled), [7] = elements without a neighbour.
 * Any input a host or device pointer, each on its own.  NE = 0 is legal.  Refused, before anything touches the device: out NULL,
 * dim not 2 or 3, NV < 0, NE < 0, elem_to_vertex NULL, without elem_ptr an nde that is no type of the dimension or NE * nde
 * beyond 32 bits; then malformed offsets, a vertex id outside [0, NV) (before any kernel reads through the ids), a vertex listed
 * twice, the first element whose node count is no type of the dimension; then the non-manifold mesh.
 * saamge_amd_face_table_arrays: the device arrays, valid while the handle lives; any pointer may be NULL.
 * saamge_amd_face_table_get: blocking copies into host or device buffers; NULL: skipped; all NULL: the counts only.
 * saamge_amd_face_nodes: the global node ids of the NF listed faces in each face's own node order, midside nodes included:
 * face_ptr_out NF + 1 ints, face_nodes_out *count_out ints; outputs NULL: the count only.
 * saamge_amd_face_dofs: bdr_dofs_inout[vdim * a + i] |= flag for every node a of every listed face and every component i with
 * bit i of comp_mask set; vdim * NV bytes, read and written in place, other bytes and other bits keep their value.  vdim 1 or
 * dim; flag in 1 .. 127 (SAAMGE_AMD_ON_ESS_DOMAIN_BORDER); comp_mask in 1 .. 2^vdim - 1.  info[0] = faces, [1] = distinct nodes
 * touched, [2] = bytes whose value changed, [3] = -1 or the first refused face.
 * Both face-list calls refuse what saamge_amd_boundary_mass refuses of the mesh and of a face list (the first face out of range,
 * then the first face listed twice), nothing of the measure; NF = 0 writes nothing. */
typedef struct saamge_amd_face_table saamge_amd_face_table;
int saamge_amd_face_table_build(int NV, int dim, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex, void *stream,
                                saamge_amd_face_table **out, long long info[8]);
int saamge_amd_face_table_arrays(const saamge_amd_face_table *t, const long long **slot_ptr, const int **nbr_elem,
                                 const int **nbr_local, long long *NB, const int **bdr_elem, const int **bdr_local,
                                 const long long **xadj, const int **adj, long long *nnz);
int saamge_amd_face_table_get(const saamge_amd_face_table *t, long long *slot_ptr, int *nbr_elem, int *nbr_local, long long *NB,
                              int *bdr_elem, int *bdr_local, long long *xadj, int *adj, long long *nnz);
void saamge_amd_face_table_free(saamge_amd_face_table *t);
int saamge_amd_face_nodes(int NV, int dim, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex, int NF,
                          const int *face_elem, const int *face_local, void *stream, int *face_ptr_out, int *face_nodes_out,
                          long long *count_out);
int saamge_amd_face_dofs(int NV, int dim, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex, int NF,
                         const int *face_elem, const int *face_local, int vdim, unsigned comp_mask, int flag, void *stream,
                         signed char *bdr_dofs_inout, long long info[4]);
/* ---- an order-1 mesh lifted to order 2 on the device (csrc/mesh_lift.hip) ----
 * From an order-1 mesh to the order-2 mesh on the same elements, in the node orders saamge_amd_element_matrices takes: the
 * 3-node triangle becomes the 6-node, the 4-node quadrilateral the 9-node, the 4-node tetrahedron the 10-node, the 8-node
 * hexahedron the 27-node one; with elem_ptr one list may mix them.  saamge_amd/mesh_lift_model.py defines every integer and every
 * coordinate bit and the device gives the same.
 * Edges: the local edges of a type are the corner pairs (0,1) (1,2) (2,0) of a triangle, (0,1) (1,2) (2,3) (3,0) of a
 * quadrilateral, (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) of a tetrahedron and the 12 pairs of hexahedron corners that differ in one
 * reference coordinate.  An edge is the vertex pair a < b and a OWNS it: edge_ptr (NV + 1) counts the owned edges per vertex,
 * edge_hi (NEd) holds the b of each edge ascending within each owner, so edge k is the k-th pair in ascending (a, b) order.
 * Node ids: the vertices keep [0, NV), listed by an element or not; edge k is node NV + k; each distinct quadrilateral face of a
 * hexahedron is node NV + NEd + f, f the rank, in slot order, of its representative slot of the face table of the order-1 mesh
 * (the lower slot of an interior pair, the slot itself on the boundary), face_slot[f] that slot; the centre of the c-th
 * quadrilateral (2D) / hexahedron (3D) in element order is node NV + NEd + NFq + c.
 * Local order: triangle and tetrahedron: the vertices, then the edges in the order above; quadrilateral: the vertices, the edge
 * nodes, the centre; hexahedron: lexicographic (iz * 3 + iy) * 3 + ix -- a position without a 1 is a corner, with one 1 the edge
 * between its two corners, with two the local face of its four corners, (1, 1, 1) the centre.
 * Coordinates (coords NULL: none): vertices are copied; an edge node is 0.5 * (X[a] + X[b]); a face node
 * 0.25 * ((X[v0] + X[v1]) + (X[v2] + X[v3])) with v0 < v1 < v2 < v3 the face's vertex ids ascending; a quadrilateral's centre
 * 0.25 * ((c0 + c1) + (c2 + c3)) and a hexahedron's 0.125 * (((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7))) in the element's
 * local order.  Midside nodes of a curved boundary are the caller's to move in coords2.
 * info[0] = NV2 = NV + [1] + [2] + [3], [1] = NEd, [2] = NFq, [3] = centre nodes, [4] = entries of elem_to_node, [5] = the most
 * edges one vertex owns, [6] = -1 or the lowest refused element, [7] = vertices that no element lists.
 * faces: a handle of saamge_amd_face_table_build on the same order-1 mesh, used only where the mesh has a hexahedron; NULL: the
 * table is built inside and released before return.  Any input a host or device pointer, each on its own.  NE = 0 is legal.
 * Refused, before anything touches the device: out NULL, dim not 2 or 3, NV < 0, NE < 0, elem_to_vertex NULL, without elem_ptr an
 * nde that is no type of the dimension or lists beyond 32 bits, a face table of another number of elements; then what
 * saamge_amd_face_table_build refuses of the mesh (a vertex id outside [0, NV) before any kernel reads through the ids); then
 * the lowest element that is a wedge (there is no 18-node type) or of order 2 already; a face table whose slots are not those
 * of the mesh; a non-manifold mesh with a hexahedron; NV2 beyond 2^31 - 1.  A refusal writes no output and leaves *out untouched.
 * saamge_amd_mesh_lift_arrays: the device arrays (coords2 NV2 x dim or NULL, elem_ptr2 NE + 1, elem_to_node info[4], edge_ptr
 * NV + 1, edge_hi NEd, face_slot NFq), valid while the handle lives; any pointer may be NULL.
 * saamge_amd_mesh_lift_get: blocking copies into host or device buffers; NULL: skipped. */
typedef struct saamge_amd_mesh_lift saamge_amd_mesh_lift;
int saamge_amd_mesh_lift_order2(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                const int *elem_to_vertex, const saamge_amd_face_table *faces, void *stream,
                                saamge_amd_mesh_lift **out, long long info[8]);
int saamge_amd_mesh_lift_arrays(const saamge_amd_mesh_lift *m, int *NV2, const double **coords2, const int **elem_ptr2,
                                const int **elem_to_node, const long long **edge_ptr, const int **edge_hi,
                                const long long **face_slot);
int saamge_amd_mesh_lift_get(const saamge_amd_mesh_lift *m, int *NV2, double *coords2, int *elem_ptr2, int *elem_to_node,
                             long long *edge_ptr, int *edge_hi, long long *face_slot);
void saamge_amd_mesh_lift_free(saamge_amd_mesh_lift *m);
/* ---- an order-1 mesh refined uniformly on the device (csrc/mesh_refine.hip) ----
 * Every triangle and quadrilateral becomes 4, every tetrahedron and hexahedron 8 elements of its own type, `levels` times; with
 * elem_ptr one list may mix the types.  One step is the lift above plus the children: saamge_amd/mesh_refine_model.py defines
 * every integer and every coordinate bit and the device gives the same.
 * GUARANTEED element numbering: child k of element e is element nc * e + k of the next level, nc = 4 in 2D and 8 in 3D.  The
 * parent of element c is c / nc, its ancestor s levels up is c >> (2 s) in 2D and c >> (3 s) in 3D, and the descendants of one
 * element are a connected agglomerate: the nested partitions saamge_amd_ml_produce_data takes are arange(NE) >> (2 s | 3 s).
 * Vertex numbering: the vertex ids of level j + 1 are the node ids of the lift of level j -- the vertices of level j keep their
 * ids, then come its edges, the quadrilateral faces of its hexahedra, its centres -- and coords of level j + 1 is coords2 of that
 * lift, bit for bit (coords NULL: none).  New vertices on a curved boundary are the caller's to move.
 * Children, as indices into the parent's lifted local node list: triangle (0,3,5) (3,1,4) (5,4,2) (3,4,5); quadrilateral and
 * hexahedron: corner j of child k is the lifted node at reference position LOC[k] + LOC[j], so child k holds the parent's corner
 * k at its own position k; tetrahedron (0,4,5,6) (4,1,7,8) (5,7,2,9) (6,8,9,3) and the inner octahedron cut along m02 - m13:
 * (4,5,6,8) (7,5,4,8) (5,6,8,9) (8,7,5,9).  A child has a positive Jacobian determinant where its parent has one.
 * want_interp != 0 keeps P_0 .. P_{levels-1}: P_j is a CSR matrix (int rowptr, as saamge_amd_spmv, saamge_amd_spgemm and
 * saamge_amd_csr_transpose take it) with one row per vertex of level j + 1 and one column per vertex of level j, columns
 * ascending: (v, 1.0) for a kept vertex, (a, 0.5) (b, 0.5) for an edge, the four vertices of a face at 0.25, the four corners of
 * a quadrilateral at 0.25 or the eight of a hexahedron at 0.125 for a centre.
 * info[0] = NV of the result, [1] = its NE, [2] = entries of its elem_to_vertex, [3] = levels, [4] = total nnz of the kept P,
 * [5] = the most edges one vertex owns over all lifted levels, [6] = -1 or the lowest refused element, [7] = vertices that no
 * element lists.  Any input a host or device pointer, each on its own.  NE = 0 is legal.
 * Refused: out NULL, levels < 1, levels > 15; then per level what the lift refuses, in its order (at level 0 that is every
 * refusal of the caller's mesh; later the NV of the next level beyond 2^31 - 1), the vertex list of the next level beyond
 * 2^31 - 1 entries, with want_interp nnz of P_j beyond 2^31 - 1 -- each before that level is allocated.  A refusal leaves *out
 * untouched and info = {0, 0, 0, 0, 0, 0, -1 or the element, 0}.  The meshes of the levels between are not kept.
 * saamge_amd_mesh_refine_arrays: the device arrays of the result (coords NV x dim or NULL, elem_ptr NE + 1 -- always given --,
 * elem_to_vertex info[2]), valid while the handle lives; any pointer may be NULL.  saamge_amd_mesh_refine_get: blocking copies
 * into host or device buffers; NULL: skipped.
 * saamge_amd_mesh_refine_level_info, level in [0, levels]: info[0] = NV, [1] = NE, [2] = entries of the vertex list, [3] = NEd,
 * [4] = NFq, [5] = centres, [6] = the most edges one vertex owns, [7] = nnz of P_level (0: not kept); the last level was not
 * lifted, its [3] .. [7] are -1.
 * saamge_amd_mesh_refine_interp_arrays / _interp_get, level in [0, levels): P_level as device arrays (rowptr nrows + 1, col and
 * val nnz) / as blocking copies; refused without want_interp. */
typedef struct saamge_amd_refined_mesh saamge_amd_refined_mesh;
int saamge_amd_mesh_refine(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex,
                           int levels, int want_interp, void *stream, saamge_amd_refined_mesh **out, long long info[8]);
int saamge_amd_mesh_refine_arrays(const saamge_amd_refined_mesh *m, int *NV, int *NE, const double **coords, const int **elem_ptr,
                                  const int **elem_to_vertex);
int saamge_amd_mesh_refine_get(const saamge_amd_refined_mesh *m, int *NV, int *NE, double *coords, int *elem_ptr,
                               int *elem_to_vertex);
int saamge_amd_mesh_refine_level_info(const saamge_amd_refined_mesh *m, int level, long long info[8]);
int saamge_amd_mesh_refine_interp_arrays(const saamge_amd_refined_mesh *m, int level, int *nrows, int *ncols, long long *nnz,
                                         const int **rowptr, const int **col, const double **val);
int saamge_amd_mesh_refine_interp_get(const saamge_amd_refined_mesh *m, int level, int *nrows, int *ncols, long long *nnz,
                                      int *rowptr, int *col, double *val);
void saamge_amd_mesh_refine_free(saamge_amd_refined_mesh *m);
/* R = P^T (P nrows x ncols) */
int saamge_amd_csr_transpose(int nrows, int ncols, const int *rowptr, const int *col, const double *val, int *Rrow,
                             long long *Rnnz, int *Rcol, double *Rval);
/* C = the entries of A with |v| > tol, in their order (AltThreshold) */
int saamge_amd_csr_threshold(int nrows, int ncols, const int *rowptr, const int *col, const double *val, double tol,
                             int *Crow, long long *Cnnz, int *Ccol, double *Cval);

/* ---- device memory kept by the library between calls ----
 * Freed device blocks are cached and reused by later calls (hipMalloc / hipFree stall the host and, for
 * hipFree, the whole device); the eigensolver workspace is persistent.  saamge_amd_release_cached_memory()
 * returns all of it to the driver (call it with no hierarchy call in flight);
 * saamge_amd_cached_memory_bytes() reports the idle cached bytes (workspace not included).
 * Environment: SAAMGE_AMD_POOL_MAX_GB (default 64; 0 disables the cache). */
void saamge_amd_release_cached_memory(void);
long long saamge_amd_cached_memory_bytes(void);
/* device bytes the library holds right now (hierarchies, workspace in use; the caller's own arrays and the idle cache
 * are not counted) and their high-water mark since the last call with reset_peak != 0 */
void saamge_amd_memory_stats(long long *live_bytes, long long *peak_bytes, int reset_peak);
/* Requests of the library's cache of device blocks that went to the driver since the last reset: counts[0] = hipMalloc calls,
 * [1] = their bytes, [2] = hipFree of cached blocks, [3] = bytes idle in the cache now.  A steady-state setup makes none. */
void saamge_amd_pool_counts(long long counts[4], int reset);

/* ---- per-kernel timing for bench.py's roofline leg (HIP events around every launch) ---- */
void saamge_amd_profile_enable(int on);
void saamge_amd_profile_reset(void);
int saamge_amd_profile_count(void);
int saamge_amd_profile_get(int i, char *name, int name_len, double *ms, long long *launches,
                           double *bytes, double *flops);
/* The same, plus the bytes the launches had to move IN THE FORMAT THEY RAN (coded SELL slices + tables + vectors for the
 * SpMV family; equal to `bytes` elsewhere): the figure a roofline fraction is computed from.  The SpMV family is listed
 * per operator as "<name>@<rows>". */
int saamge_amd_profile_get2(int i, char *name, int name_len, double *ms, long long *launches, double *bytes, double *flops,
                            double *fmt_bytes);

/* ---- agglomerate partitions built on the device -----------------------------------------------------------------------
 * The entry points above take partitions[k] / nparts[k] from the caller.  These calls make them: deterministic, every part
 * connected, none empty, numbered by smallest member.  elems_per_agg is a target; the number of parts produced is returned.
 * The algorithm (seeded level-synchronous growth, recentring, size repair) is defined by saamge_amd/partition_model.py and
 * the device gives the same integers.  Arrays may be host or device pointers, each on its own, with
 * one exception: host columns (adj) need host offsets (xadj), which say how much to copy.  An element that lists a dof
 * twice is refused.  Parts above max_size are split in at most 32 rounds (enough for meshes by a wide margin; a hub with
 * thousands of leaves may keep a part above the cap).  A value of `seeding` other than 0 and 1 is refused before anything
 * is written; a zero-filled options struct asks for seeding 0. */
typedef struct saamge_amd_partition_options {
    int min_shared;      /* 1: dofs two elements share to be adjacent (1 vertex neighbours, 4 faces of Q1 hexes); mesh entry */
    int lloyd_iters;     /* 0: recentring passes */
    int max_size;        /* -1: 2 * elems_per_agg; 0: no cap */
    int min_size;        /* -1: elems_per_agg / 4; 0: small parts are left alone */
    unsigned seed;       /* 0 */
    int seeding;         /* 0: lowest priorities; 1: spaced, the greedy distance-r independent set, topped up to the target count */
} saamge_amd_partition_options;
void saamge_amd_partition_options_default(saamge_amd_partition_options *o);
/* What the spaced seeding did in the calling thread's last partition of one graph (saamge_amd_partition_graph, or the last
 * level of saamge_amd_partition_mesh): info[0] = the radius r, [1] = independent-set rounds over all radii tried and the
 * top-up, [2] = seeds of the independent set, [3] = seeds after the top-up.  All 0 after seeding = 0. */
void saamge_amd_partition_seeding_info(long long info[4]);
/* The options with `growth` as their last field.  saamge_amd_partition_options keeps its size (callers and tests hold it to
 * six ints), so the field lives in this struct, whose first six fields are those of saamge_amd_partition_options in the same
 * order, and the _v2 entry points below take it; the entry points without _v2 are these with growth = 0.  A value of
 * `seeding` or of `growth` other than 0 and 1 is refused before anything is written; a zero-filled struct asks for 0, 0. */
typedef struct saamge_amd_partition_options_v2 {
    int min_shared;
    int lloyd_iters;
    int max_size;
    int min_size;
    unsigned seed;
    int seeding;
    int growth;          /* 0: level-synchronous growth; 1: balanced, per round a part takes at most elems_per_agg - size of its
                            claimants (most neighbours in the part first), the rest is released to growth 0 when no open part
                            has a claimant; first growth and the regrowth after recentring, not the size repair */
} saamge_amd_partition_options_v2;
void saamge_amd_partition_options_v2_default(saamge_amd_partition_options_v2 *o);
/* The same for the balanced growth (with lloyd_iters > 0: the last growth): info[0] = balanced rounds, [1] = nodes labelled
 * under a quota, [2] = parts still open at the release, [3] = nodes labelled after the release ([2] = [3] = 0 when every
 * node was labelled under a quota).  All 0 after growth = 0. */
void saamge_amd_partition_growth_info(long long info[4]);

/* One level: a symmetric CSR graph (self-loops are ignored) -> part[n], *nparts_out.  o == NULL: the defaults.  Offsets that
 * do not ascend from 0, columns outside [0, n) and entries without their transpose are refused. */
int saamge_amd_partition_graph(int n, const long long *xadj, const int *adj, int elems_per_agg,
                               const saamge_amd_partition_options *o, void *stream, int *part, int *nparts_out);
int saamge_amd_partition_graph_v2(int n, const long long *xadj, const int *adj, int elems_per_agg,
                                  const saamge_amd_partition_options_v2 *o, void *stream, int *part, int *nparts_out);

/* All levels from the mesh.  elem_ptr == NULL: every element has nde dofs.  elems_per_agg has num_coarsenings entries.
 * Level k partitions graph k: graph 0 is the element graph, graph k + 1 the quotient graph of level k. */
typedef struct saamge_amd_partitioning saamge_amd_partitioning;
int saamge_amd_partition_mesh(int NE, int nde, const int *elem_ptr, const int *elem_to_dof, int ND, int num_coarsenings,
                              const int *elems_per_agg, const saamge_amd_partition_options *o, void *stream,
                              saamge_amd_partitioning **out);
int saamge_amd_partition_mesh_v2(int NE, int nde, const int *elem_ptr, const int *elem_to_dof, int ND, int num_coarsenings,
                                 const int *elems_per_agg, const saamge_amd_partition_options_v2 *o, void *stream,
                                 saamge_amd_partitioning **out);

/* Boundary refinement, off unless asked for: rounds in which nodes on a part's boundary move to the neighbouring part that
 * holds most of their neighbours, which lowers the edge cut and smooths the parts (partition_model.py, "refine"; DESIGN.md
 * section 4.5).  Parts stay connected, none is emptied, none grows beyond max_size (0: no cap) or shrinks below
 * max(min_size, 1) through the pass, and the part count stays.  Deterministic; `seed` orders equal gains as it does elsewhere.
 *
 * saamge_amd_partition_refine works on any partition of a symmetric CSR graph, the caller's own included: part (n labels in
 * [0, nparts), no part empty; host or device pointer, like xadj and adj each on its own) is read and written in place.
 * renumber = 1 numbers the parts by their smallest member afterwards, 0 keeps the caller's labels.  At most `rounds` rounds
 * move nodes.  info (may be NULL): [0] = rounds that moved nodes, [1] = nodes moved, [2] = the sum of their gains = cut edges
 * removed, [3] = 1 if the pass stopped because no node could move, else 0.  Refused before part is written: a malformed graph
 * (as saamge_amd_partition_graph), a label outside [0, nparts), an empty part, negative rounds / max_size / min_size, renumber
 * outside {0, 1}.  max_size and min_size are taken as given (no -1 defaults here). */
int saamge_amd_partition_refine(int n, const long long *xadj, const int *adj, int nparts, int *part, int rounds, int max_size,
                                int min_size, unsigned seed, int renumber, void *stream, long long info[4]);
/* saamge_amd_partition_mesh_v2 with the pass after each level's partition: refine_rounds[k] rounds at coarsening k, with that
 * level's caps (the defaults resolved) and seed from o; the parts are numbered again and the next graph is the quotient graph
 * of the refined parts.  refine_rounds == NULL or all zeros: saamge_amd_partition_mesh_v2, bit for bit. */
int saamge_amd_partition_mesh_refined(int NE, int nde, const int *elem_ptr, const int *elem_to_dof, int ND, int num_coarsenings,
                                      const int *elems_per_agg, const saamge_amd_partition_options_v2 *o, const int *refine_rounds,
                                      void *stream, saamge_amd_partitioning **out);
/* info as above for the calling thread's last refinement (saamge_amd_partition_refine, or the last refined level of
 * saamge_amd_partition_mesh_refined). */
void saamge_amd_partition_refine_info(long long info[4]);

/* Pointers that can be handed to saamge_amd_ml_produce_data* as partitions / nparts; they live as long as the handle.
 * on_host = 0: device arrays, 1: host copies. */
int saamge_amd_partitioning_arrays(const saamge_amd_partitioning *p, int on_host, const int *const **partitions,
                                   const int **nparts_host);
int saamge_amd_partitioning_get(const saamge_amd_partitioning *p, int level, int *part_host, int *n_elem, int *nparts);
/* graph `level` (0 .. num_coarsenings); NULL arrays: sizes only.  A getter: copies with a blocking hipMemcpy, on no stream. */
int saamge_amd_partitioning_graph(const saamge_amd_partitioning *p, int level, long long *xadj, int *adj, int *n,
                                  long long *nnz);
void saamge_amd_partitioning_free(saamge_amd_partitioning *p);

/* ---- the operator assembled on the device from the element matrices -----------------------------------------------------
 * The entry points above take the assembled, boundary-eliminated operator A from the caller.  These calls make it from the
 * inputs the hierarchy takes anyway.  Row i holds every dof that shares an element with i, ascending, entries of value zero
 * included; a value is the sum of the element terms in ascending element id; an off-diagonal entry in the row or column of
 * an essential dof (bdr_dofs[i] & SAAMGE_AMD_ON_ESS_DOMAIN_BORDER; bdr_dofs == NULL: none) is stored as 0.0, the diagonal
 * is kept.  saamge_amd/assemble_model.py defines the result and the device gives the same bits.
 * Arrays may be host or device pointers, each on its own.  Refused: elem_ptr[0] != 0, an empty element, a dof outside
 * [0, n), an element that lists a dof twice, a dof that lies in no element. */
typedef struct saamge_amd_operator saamge_amd_operator;
/* nde > 0 and elem_ptr == NULL: every element has nde dofs.  elem_ptr != NULL: offsets as in
 * saamge_amd_ml_produce_data_mixed, nde ignored.  elmat packed as in that entry. */
int  saamge_amd_operator_assemble(int n, int NE, int nde, const int *elem_ptr, const int *elem_to_dof,
                                  const double *elmat, const signed char *bdr_dofs, void *stream,
                                  saamge_amd_operator **out);
/* device arrays, valid as long as the handle lives; what saamge_amd_ml_produce_data64 / _mixed64 take as A */
int  saamge_amd_operator_arrays(const saamge_amd_operator *op, const long long **rowptr_dev, const int **col_dev,
                                const double **val_dev, long long *nnz);
/* host or device output buffers; all NULL: *nnz only.  A getter: blocking copy. */
int  saamge_amd_operator_get(const saamge_amd_operator *op, long long *rowptr, int *col, double *val, long long *nnz);
/* new element matrices, same mesh and flags: the numeric pass only, val_dev rewritten in place (on the stream of the
 * assembly; returns when it is done) */
int  saamge_amd_operator_update(saamge_amd_operator *op, const double *elmat);
/* b (n, in place) for essential values x_ess (n, read at essential dofs only); elmat = the matrices of the operator */
int  saamge_amd_operator_eliminate_rhs(const saamge_amd_operator *op, const double *elmat, const double *x_ess, double *b);
/* b (n, overwritten) from packed element vectors (element e: nd_e doubles at elem_ptr[e], the output of
 * saamge_amd_element_loads on the mesh of the operator): b_i the sum of the terms of dof i in ascending element id.  Essential
 * dofs are assembled like any other; saamge_amd_operator_eliminate_rhs overwrites them afterwards.  Host or device pointers. */
int  saamge_amd_operator_assemble_rhs(const saamge_amd_operator *op, const double *elvec, double *b);
void saamge_amd_operator_free(saamge_amd_operator *op);
/* Rows by the path they took: counts[0 .. 2] the symbolic pass (several rows per wavefront; one workgroup per row with the
 * candidates in LDS; through global memory), counts[3 .. 5] the numeric pass (the same three). */
int  saamge_amd_operator_path_counts(const saamge_amd_operator *op, long long counts[6]);
/* Tests: the largest candidate count (sum of the sizes of the elements of a row) of the first two paths for the assemblies
 * that follow, process-wide.  Defaults and upper limits 64 and 4096; a negative value: the default. */
int  saamge_amd_operator_set_path_limits(int short_candidates, int lds_candidates);

/* ---- lowest eigenpairs of A x = lambda M x: LOBPCG with soft locking, preconditioned by the V-cycle ----
 * The definition is saamge_amd/lobpcg_model.py; DESIGN.md section 4.18.  The library keeps essential dofs as decoupled
 * diagonal rows, each of them an eigenvector of the pencil with eigenvalue a_ii / m_ii that may lie among the lowest:
 * with constrain_essential the iteration runs in the subspace that is zero there (invariant under A, under an M whose
 * essential rows and columns are eliminated like A's, and under the V-cycle followed by the mask). */
typedef struct saamge_amd_lobpcg_options {
    int nev;                  /* wanted pairs, 1 .. 16 */
    int block;                /* nb, nev <= nb <= 16; 0: nev */
    double tol;               /* pair j accepted when ||A x - lambda M x||_2 <= tol * lambda * ||M x||_2; > 0 */
    int max_iter;             /* >= 0 */
    int constrain_essential;  /* 1: rows the hierarchy was set up with as essential (SAAMGE_AMD_ON_ESS_DOMAIN_BORDER in its
                                 level-0 agg_flags, what saamge_amd_get_mis returns) are held at zero in every vector */
    unsigned seed;            /* start block when x0 == NULL */
} saamge_amd_lobpcg_options;
void saamge_amd_lobpcg_options_default(saamge_amd_lobpcg_options *o);   /* 1, 0, 1e-8, 100, 1, 0 */
/* A = the hierarchy's level-0 operator, B = its V-cycle (plugs included).  M: n x n CSR, symmetric positive definite,
 * 64-bit row offsets (what saamge_amd_operator_arrays returns), NULL = identity.  x0: n x nb column-major or NULL.
 * evals (host, nev), evecs (n x nev column-major, M-orthonormal), res (host, nev: the rho_j), hist (host,
 * (max_iter + 1) x nev row-major, may be NULL; rows 0 .. *iters are written).  M, x0, evecs: host or device pointers, each
 * on its own.  res, iters, converged may be NULL.  *converged = 0 with a zero return: max_iter reached, or a breakdown (a
 * Gram matrix of the basis that is not safely positive definite, twice in a row); evals, evecs hold the best pairs so far.
 * Refused with a nonzero return, the argument named in saamge_amd_last_error, before any work memory is taken, any kernel
 * is launched or any output written (the hierarchy's flags and a device-resident M are read to be checked): a NULL h, o, evals or
 * evecs; nev, block, tol, max_iter out of range; 3 nb above the number of unconstrained rows; M offsets that do not start
 * at 0 or decrease, a column outside [0, n); a level 0 that is row-partitioned over several ranks.
 * Work memory: 9 nb n doubles (6 nb n without M) from the library's pool, returned before the call returns. */
int saamge_amd_lobpcg(saamge_amd_hierarchy *h, const long long *Mrowptr, const int *Mcol, const double *Mval,
                      const saamge_amd_lobpcg_options *o, const double *x0, double *evals, double *evecs,
                      double *res, int *iters, int *converged, double *hist);
/* The two block kernels on their own (tests), like saamge_amd_spgemm; host or device pointers, blocks column-major.
 * gram: G_host (p x q, column-major) = S^T T, 1 <= p, q <= 48, lds, ldt >= n; T == S (and ldt == lds, q == p) does half
 * the work; deterministic.  combine: Y (n x q) = S C (accumulate != 0: Y += S C), C_host p x q column-major; Y may be S
 * itself (the same pointer and leading dimension), any other overlap of the two is refused. */
int saamge_amd_blockvec_gram(int n, int p, const double *S, long long lds, int q, const double *T, long long ldt, double *G_host);
int saamge_amd_blockvec_combine(int n, int p, const double *S, long long lds, int q, const double *C_host, double *Y,
                                long long ldy, int accumulate);

/* ---- block solves: k columns per call ----
 * saamge_amd_spmv, _smoother, _vcycle and _pcg on k columns at once: the matrix data of every level is read once for the
 * columns of a launch (up to 8; more run in chunks) instead of once per column.  Blocks are column-major with a leading
 * dimension, host or device pointers exactly as the single-vector calls take them; rows past the row count are padding
 * and keep what they hold.  THE CONTRACT: column j of every output, iters[j], converged[j] and column j's history are bit
 * for bit what the single-vector call returns when it is given column j alone on the same hierarchy and options (the block
 * kernels keep every row's order of additions).  hist: k x (max_iter + 1), column j's history at hist + j (max_iter + 1),
 * entries 0 .. its own last step written and the rest left as they are; may be NULL, like converged.  A caller's smoother
 * or coarsest solver is called once per column; the dense and the block-tridiagonal coarsest solves run column by column.
 * Refused, each by name, before any HIP call and before anything is written: k < 1 or k > 64; a NULL block; a leading
 * dimension below the row count; X overlapping B (Y overlapping X for spmv_block); a row-partitioned hierarchy.
 * Work memory: the cycle's vectors for min(k, 8) columns, taken from the pool at the hierarchy's first block call, grown
 * only by a wider call, returned with the hierarchy (saamge_amd_memory_stats shows it). */
int saamge_amd_spmv_block(int nrows, int ncols, const int *rowptr, const int *col, const double *val, int k, const double *X,
                          long long ldx, double *Y, long long ldy);      /* honours spmv_sell like saamge_amd_spmv */
int saamge_amd_smoother_block(saamge_amd_hierarchy *h, int level, int k, const double *B, long long ldb, double *X, long long ldx);
int saamge_amd_vcycle_block(saamge_amd_hierarchy *h, int k, const double *B, long long ldb, double *X, long long ldx,
                            int iterative_mode);
int saamge_amd_pcg_block(saamge_amd_hierarchy *h, int k, const double *B, long long ldb, double *X, long long ldx, double rel_tol,
                         double abs_tol, int max_iter, int squared_tol, int zero_guess, int *iters, int *converged, double *hist);

#ifdef __cplusplus
}
#endif
#endif
