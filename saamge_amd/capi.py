"""ctypes binding of include/saamge_amd.h -- the test/bench harness side of the C ABI.

The product is ``libsaamge_amd.so`` (HIP, gfx950).  This module only marshals numpy
arrays / raw device pointers through the C ABI; it contains no numerics and no CPU
fallback: if the library is missing, import of the binding fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SAAMGE_AMD_LIB") or os.path.join(_HERE, "libsaamge_amd.so")

MAX_LEVELS = 8

# every symbol include/saamge_amd.h declares
SYMBOLS = [
    "saamge_amd_params_default", "saamge_amd_last_error", "saamge_amd_ml_produce_data",
    "saamge_amd_ml_free_data", "saamge_amd_vcycle_mult", "saamge_amd_smoother", "saamge_amd_pcg",
    "saamge_amd_num_levels", "saamge_amd_level_info", "saamge_amd_get_csr", "saamge_amd_get_table",
    "saamge_amd_get_mis", "saamge_amd_get_ae_eigens", "saamge_amd_get_mis_svd", "saamge_amd_spmv",
    "saamge_amd_lower_eigens_batched", "saamge_amd_profile_enable", "saamge_amd_profile_reset",
    "saamge_amd_profile_count", "saamge_amd_profile_get", "saamge_amd_memcpy",
    "saamge_amd_update_operators", "saamge_amd_inertia_batched", "saamge_amd_vcycle",
    "saamge_amd_set_coarse_solver", "saamge_amd_comm_unique_id", "saamge_amd_comm_create", "saamge_amd_comm_destroy",
    "saamge_amd_params_set_comm", "saamge_amd_comm_selftest", "saamge_amd_comm_last_error",
    "saamge_amd_release_cached_memory", "saamge_amd_cached_memory_bytes",
    "saamge_amd_ml_produce_data64", "saamge_amd_get_csr64", "saamge_amd_spmv64", "saamge_amd_set_smoother", "saamge_amd_profile_get2", "saamge_amd_level_format", "saamge_amd_update_operators2",
    "saamge_amd_ml_produce_data_parcsr", "saamge_amd_memory_stats", "saamge_amd_pool_counts",
    "saamge_amd_options_default", "saamge_amd_set_options", "saamge_amd_get_options",
    "saamge_amd_ml_produce_data_mixed", "saamge_amd_ml_produce_data_mixed64",
    "saamge_amd_partition_options_default", "saamge_amd_partition_seeding_info", "saamge_amd_partition_growth_info", "saamge_amd_partition_options_v2_default",
    "saamge_amd_partition_graph_v2", "saamge_amd_partition_mesh_v2", "saamge_amd_partition_graph", "saamge_amd_partition_mesh",
    "saamge_amd_partition_refine", "saamge_amd_partition_mesh_refined", "saamge_amd_partition_refine_info",
    "saamge_amd_partitioning_arrays", "saamge_amd_partitioning_get", "saamge_amd_partitioning_graph",
    "saamge_amd_partitioning_free", "saamge_amd_coarse_solver_info",
    "saamge_amd_spgemm", "saamge_amd_csr_transpose", "saamge_amd_csr_threshold",
    "saamge_amd_operator_assemble", "saamge_amd_operator_arrays", "saamge_amd_operator_get", "saamge_amd_operator_update",
    "saamge_amd_operator_eliminate_rhs", "saamge_amd_operator_free", "saamge_amd_operator_path_counts",
    "saamge_amd_operator_set_path_limits",
    "saamge_amd_level_order_info", "saamge_amd_ae_order", "saamge_amd_element_matrices",
    "saamge_amd_element_mass", "saamge_amd_element_loads", "saamge_amd_operator_assemble_rhs",
    "saamge_amd_boundary_mass", "saamge_amd_boundary_loads",
    "saamge_amd_boundary_points", "saamge_amd_boundary_eval", "saamge_amd_boundary_mass_points", "saamge_amd_boundary_loads_points",
    "saamge_amd_element_points", "saamge_amd_element_eval", "saamge_amd_element_loads_points", "saamge_amd_element_errors",
    "saamge_amd_element_matrices_points", "saamge_amd_element_mass_points",
    "saamge_amd_face_table_build", "saamge_amd_face_table_arrays", "saamge_amd_face_table_get", "saamge_amd_face_table_free",
    "saamge_amd_face_nodes", "saamge_amd_face_dofs",
    "saamge_amd_mesh_lift_order2", "saamge_amd_mesh_lift_arrays", "saamge_amd_mesh_lift_get", "saamge_amd_mesh_lift_free",
    "saamge_amd_mesh_refine", "saamge_amd_mesh_refine_arrays", "saamge_amd_mesh_refine_get", "saamge_amd_mesh_refine_level_info",
    "saamge_amd_mesh_refine_interp_arrays", "saamge_amd_mesh_refine_interp_get", "saamge_amd_mesh_refine_free",
    "saamge_amd_lobpcg_options_default", "saamge_amd_lobpcg", "saamge_amd_blockvec_gram", "saamge_amd_blockvec_combine",
    "saamge_amd_spmv_block", "saamge_amd_smoother_block", "saamge_amd_vcycle_block", "saamge_amd_pcg_block",
]

ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong))
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_longlong)
COARSE_SOLVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double))
SMOOTHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double))
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong), C.c_void_p,
                           C.POINTER(C.c_longlong))


class Options(C.Structure):      # saamge_amd_options
    _fields_ = [(k, C.c_int) for k in ("eig_strict", "eig_certify", "eig_min_n", "eig_force_fallback", "eig_dense_only",
                                       "eig_dense_one_stage", "eig_nullcheck", "eig_keep_inertia_factor", "band_assembly",
                                       "eig_dedupe", "eig_outer_panels", "overlap", "sell", "spmv_sell", "debug", "host_heap_pad_mb",
                                       "ae_order")]


class Params(C.Structure):
    _fields_ = [
        ("num_coarsenings", C.c_int),
        ("theta", C.c_double * MAX_LEVELS),
        ("nu_relax", C.c_int * MAX_LEVELS),
        ("nu_pro", C.c_int * MAX_LEVELS),
        ("avoid_ess_bdr_dofs", C.c_int),
        ("testmesh", C.c_int),
        ("coarse_solver", C.c_int),
        ("coarse_rtol", C.c_double),
        ("coarse_max_iter", C.c_int),
        ("workspace_bytes", C.c_longlong),
        ("keep_debug", C.c_int),
        ("rank", C.c_int),
        ("world", C.c_int),
        ("allgather", ALLGATHER_FN),
        ("allgather_ctx", C.c_void_p),
        ("allreduce_sum", ALLREDUCE_FN),
        ("alltoallv", ALLTOALLV_FN),
        ("dist_min_local_rows", C.c_longlong),
        ("comm_stream_ordered", C.c_int),
        ("correct_nullspace", C.c_int),
        ("extra_modes", C.c_void_p),
        ("num_extra_modes", C.c_int),
        ("algebraic", C.c_int),
        ("smooth_drop_tol", C.c_double),
        ("do_aggregates", C.c_int),
        ("eigensolver", C.c_int),
        ("eig_tol", C.c_double),
        ("options", Options),
    ]


class ParCsr(C.Structure):      # saamge_amd_parcsr
    _fields_ = [("global_rows", C.c_longlong), ("row_starts", C.c_void_p), ("nrows", C.c_int),
                ("diag_i", C.c_void_p), ("diag_j", C.c_void_p), ("diag_a", C.c_void_p),
                ("offd_i", C.c_void_p), ("offd_j", C.c_void_p), ("offd_a", C.c_void_p),
                ("num_cols_offd", C.c_int), ("col_map_offd", C.c_void_p)]


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME
    as the system one this library links to); whichever is loaded first serves both.  If OUR
    library came first, torch would later bring in its own copy as a second runtime and find
    "No HIP GPUs are available".  So when torch is installed but not imported yet, map ITS
    runtime first: this library then binds to it, exactly as when torch is imported first."""
    import sys
    if "torch" in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        cand = os.path.join(libdir, "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass   # no torch / unusual layout: the system runtime is used


def load():
    """Load the HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("saamge_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; "
                           "g.build()'` (hipcc, gfx950); there is no CPU fallback" % LIB_PATH)
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    lib.saamge_amd_last_error.restype = C.c_char_p
    lib.saamge_amd_num_levels.restype = C.c_int
    _lib = lib
    # tests that run the library in a child process choose options through SAAMGE_AMD_TEST_OPTIONS="name=value,..." -- read
    # HERE, by the harness; the library itself has no such switch
    spec = os.environ.get("SAAMGE_AMD_TEST_OPTIONS")
    if spec:
        set_options(**{kv.split("=")[0].strip(): int(kv.split("=")[1]) for kv in spec.split(",") if kv.strip()})
    return lib


def _check(rc):
    if rc != 0:
        raise RuntimeError("saamge_amd: " + load().saamge_amd_last_error().decode())


def _ptr(a):
    """numpy array -> host pointer; int -> raw (device) pointer; None -> NULL."""
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, int):
        return C.c_void_p(a)
    if hasattr(a, "data_ptr"):  # torch tensor (device memory plumbing)
        return C.c_void_p(a.data_ptr())
    assert a.flags["C_CONTIGUOUS"]
    return C.c_void_p(a.ctypes.data)


class _Handle(object):
    """Owner of a handle of the library, `h`, until free() / close() or the end of a `with` block; _FREE names the C function
    that frees it."""
    _FREE = None
    h = None

    @classmethod
    def build(cls, *args, **kw):
        return cls(*args, **kw)

    def free(self):
        if self.h is not None and self.h.value:
            free = getattr(load(), self._FREE)
            free.restype = None
            free(self.h)
        self.h = None

    def close(self):
        self.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def default_params(num_coarsenings=1, theta=0.003, nu_relax=3, testmesh=False, keep_debug=False,
                   coarse_rtol=1e-14, workspace_bytes=None, dist_min_local_rows=None,
                   coarse_solver=None, nu_pro=0, correct_nullspace=False, extra_modes=None, algebraic=False,
                   smooth_drop_tol=0.0, do_aggregates=False, eigensolver=0, eig_tol=None):
    p = Params()
    load().saamge_amd_params_default(C.byref(p))
    p.options = get_options()          # (what set_options / SAAMGE_AMD_TEST_OPTIONS chose stays in force for this hierarchy)
    p.num_coarsenings = num_coarsenings
    for i in range(MAX_LEVELS):
        p.theta[i] = theta
        p.nu_relax[i] = nu_relax
        p.nu_pro[i] = nu_pro
    p.testmesh = int(testmesh)
    p.correct_nullspace = int(correct_nullspace)
    p.algebraic = 2 if algebraic == "window" else int(bool(algebraic))
    p.smooth_drop_tol = float(smooth_drop_tol)
    p.do_aggregates = int(do_aggregates)
    p.eigensolver = {"subspace": 0, "dense": 1}.get(eigensolver, eigensolver)
    p.keep_debug = int(keep_debug)
    if eig_tol is not None:
        p.eig_tol = float(eig_tol)
    p.coarse_rtol = coarse_rtol
    if workspace_bytes is not None:
        p.workspace_bytes = int(workspace_bytes)
    if dist_min_local_rows is not None:
        p.dist_min_local_rows = int(dist_min_local_rows)
    if extra_modes is not None:
        em = np.asfortranarray(np.asarray(extra_modes, dtype=np.float64))   # n x q, column-major
        em = em.reshape(em.shape[0], -1, order="F")
        p._extra_keep = em                                                   # keep alive with the params
        p.extra_modes = em.ctypes.data
        p.num_extra_modes = em.shape[1]
    if coarse_solver is not None:
        p.coarse_solver = int(coarse_solver)   # 0 auto, 1 dense Cholesky, 2 inner PCG
    return p


class Hierarchy(_Handle):
    """Owner of a saamge_amd_hierarchy (== ml_data_t).  Mirrors the reference call
    sequence: ml_produce_data -> VCycleSolver::Mult / CGSolver::Mult -> ml_free_data."""
    _FREE = "saamge_amd_ml_free_data"

    def _prepare_params(self, params, group, stream, dist_solve):
        """A private copy of the caller's params with the collectives of `group` installed."""
        lib = load()
        caller_params = params
        params = Params.from_buffer_copy(params)      # the caller's struct is never modified
        self._keep_params = caller_params             # (keeps extra_modes alive)
        if group is not None and group.world > 1 and getattr(group, "native", False):
            # the library's own RCCL collectives (csrc/comm.hip), enqueued on the hierarchy's stream
            rc = lib.saamge_amd_params_set_comm(C.byref(params), group.native_comm(stream))
            assert rc == 0
            if not dist_solve:
                params.allreduce_sum = ALLREDUCE_FN(0)
                params.alltoallv = ALLTOALLV_FN(0)
        elif group is not None and group.world > 1:
            # distributed setup: this rank solves the eigenproblems of its AE range only;
            # distributed solve: large levels are applied by row blocks with halo exchange
            self._cb = group.allgather_callback()
            params.rank = group.rank
            params.world = group.world
            params.allgather = self._cb
            if dist_solve:
                self._cb2 = group.solve_callbacks(stream)
                params.allreduce_sum, params.alltoallv = self._cb2
                params.comm_stream_ordered = int(group.stream_ordered(stream))
        return params

    def __init__(self, A_rowptr, A_col, A_val, n, elem_to_dof, elmat, bdr, partitions, nparts,
                 params, NE, nde, stream=0, group=None, dist_solve=True, elem_ptr=None):
        """elem_ptr (NE + 1 offsets; nde ignored): elements of different sizes -- flat elem_to_dof and the element
        matrices packed in element order (saamge_amd_ml_produce_data_mixed)."""
        lib = load()
        self._keep = (A_rowptr, A_col, A_val, elem_to_dof, elmat, bdr, partitions, elem_ptr)
        params = self._prepare_params(params, group, stream, dist_solve)
        parts = (C.c_void_p * len(partitions))(*[_ptr(p).value for p in partitions])
        npa = (C.c_int * len(nparts))(*[int(x) for x in nparts])
        h = C.c_void_p()
        # 64-bit row offsets (torch.int64 / np.int64): operators beyond 2^31 stored entries
        wide = str(getattr(A_rowptr, "dtype", "")).endswith("int64")
        if elem_ptr is not None:
            produce = lib.saamge_amd_ml_produce_data_mixed64 if wide else lib.saamge_amd_ml_produce_data_mixed
            _check(produce(
                C.c_int(n), _ptr(A_rowptr), _ptr(A_col), _ptr(A_val), C.c_int(NE), _ptr(elem_ptr),
                _ptr(elem_to_dof), _ptr(elmat), _ptr(bdr), parts, npa, C.byref(params),
                C.c_void_p(stream), C.byref(h)))
        else:
            produce = lib.saamge_amd_ml_produce_data64 if wide else lib.saamge_amd_ml_produce_data
            _check(produce(
                C.c_int(n), _ptr(A_rowptr), _ptr(A_col), _ptr(A_val), C.c_int(NE), C.c_int(nde),
                _ptr(elem_to_dof), _ptr(elmat), _ptr(bdr), parts, npa, C.byref(params),
                C.c_void_p(stream), C.byref(h)))
        self.h = h
        self.n = n
        self.testmesh = bool(params.testmesh)

    @classmethod
    def from_problem(cls, prob, params, stream=0, group=None, dist_solve=True):
        """Build from a saamge_amd.problems.Problem (host numpy arrays).  A problem that carries `elem_ptr` (elements of
        different sizes: flat elem_to_dof, packed elmat) goes through saamge_amd_ml_produce_data_mixed; its element
        arrays, bdr and partitions may be host arrays or device tensors."""
        if getattr(prob, "elem_ptr", None) is not None:
            return cls._from_mixed_problem(prob, params, stream, group, dist_solve)
        A = prob.A.tocsr()
        rowptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
        col = np.ascontiguousarray(A.indices, dtype=np.int32)
        val = np.ascontiguousarray(A.data, dtype=np.float64)
        e2d = np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32)
        elmat = np.ascontiguousarray(prob.elmat, dtype=np.float64)
        bdr = np.ascontiguousarray(prob.bdr, dtype=np.int8)
        parts = [np.ascontiguousarray(p, dtype=np.int32) for p in prob.partitions[:params.num_coarsenings]]
        nparts = [int(p.max()) + 1 for p in parts]
        return cls(rowptr, col, val, A.shape[0], e2d, elmat, bdr, parts, nparts, params,
                   e2d.shape[0], e2d.shape[1], stream, group, dist_solve)

    @classmethod
    def _from_mixed_problem(cls, prob, params, stream, group, dist_solve):
        def arr(a, dt):          # device tensors pass through, host arrays are made contiguous
            return a if hasattr(a, "data_ptr") else np.ascontiguousarray(a, dtype=dt)
        A = prob.A.tocsr()
        rowptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
        col = np.ascontiguousarray(A.indices, dtype=np.int32)
        val = np.ascontiguousarray(A.data, dtype=np.float64)
        eptr = arr(prob.elem_ptr, np.int32)
        e2d = arr(prob.elem_to_dof, np.int32)
        elmat = arr(prob.elmat, np.float64)
        bdr = arr(prob.bdr, np.int8) if prob.bdr is not None else None
        parts = [arr(p, np.int32) for p in prob.partitions[:params.num_coarsenings]]
        nparts = [int(p.max()) + 1 for p in parts]
        return cls(rowptr, col, val, A.shape[0], e2d, elmat, bdr, parts, nparts, params, len(eptr) - 1, 0,
                   stream, group, dist_solve, elem_ptr=eptr)

    @classmethod
    def from_partitioning(cls, prob, params, partitioning, on_host=False, stream=0):
        """from_problem with the partitions of a `Partitioning` (partition_mesh) in place of prob.partitions: its device
        arrays (on_host=False) or its host copies go to the entry point as they are."""
        A = prob.A.tocsr()
        rowptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
        col = np.ascontiguousarray(A.indices, dtype=np.int32)
        val = np.ascontiguousarray(A.data, dtype=np.float64)
        e2d = np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32)
        elmat = np.ascontiguousarray(prob.elmat, dtype=np.float64)
        bdr = np.ascontiguousarray(prob.bdr, dtype=np.int8) if prob.bdr is not None else None
        nc = params.num_coarsenings
        parts = partitioning.pointers(on_host)[:nc]
        nparts = partitioning.nparts[:nc]
        eptr = getattr(prob, "elem_ptr", None)
        if eptr is not None:
            eptr = np.ascontiguousarray(eptr, dtype=np.int32)
            h = cls(rowptr, col, val, A.shape[0], e2d, elmat, bdr, parts, nparts, params, len(eptr) - 1, 0, stream,
                    elem_ptr=eptr)
        else:
            h = cls(rowptr, col, val, A.shape[0], e2d, elmat, bdr, parts, nparts, params, e2d.shape[0], e2d.shape[1], stream)
        h._keep = h._keep + (partitioning,)
        return h

    @classmethod
    def from_operator(cls, prob, op, params, stream=0):
        """from_problem with the operator of an `Operator` in place of prob.A: its device arrays go to the 64-bit entry as
        they are (no copy), so the hierarchy keeps `op` alive; after op.update(), update_operators(None) takes the new
        values."""
        def arr(a, dt):
            return a if a is None or hasattr(a, "data_ptr") else np.ascontiguousarray(a, dtype=dt)
        rp, cp, vp, _ = op.arrays()
        rowptr, col, val = _DevicePointer(rp, "int64"), _DevicePointer(cp, "int32"), _DevicePointer(vp, "float64")
        e2d = arr(prob.elem_to_dof, np.int32)
        elmat = arr(prob.elmat, np.float64)
        bdr = arr(prob.bdr, np.int8)
        parts = [arr(p, np.int32) for p in prob.partitions[:params.num_coarsenings]]
        nparts = [int(p.max()) + 1 for p in parts]
        eptr = getattr(prob, "elem_ptr", None)
        if eptr is not None:
            eptr = arr(eptr, np.int32)
            h = cls(rowptr, col, val, op.n, e2d, elmat, bdr, parts, nparts, params, len(eptr) - 1, 0, stream, elem_ptr=eptr)
        else:
            h = cls(rowptr, col, val, op.n, e2d, elmat, bdr, parts, nparts, params, e2d.shape[0], e2d.shape[1], stream)
        h._keep = h._keep + (op,)
        return h

    @classmethod
    def from_parcsr(cls, piece, params, stream=0, group=None, dist_solve=True):
        """Build from PER-RANK inputs (saamge_amd_ml_produce_data_parcsr): `piece` = this rank's entry of
        problems.split_parcsr -- its row block as diag / offd / col_map_offd, its own elements (global dof ids), their
        matrices, the flags of its own rows and its local agglomerate partitions.  Host numpy arrays or device tensors."""
        self = cls.__new__(cls)
        lib = load()
        params = self._prepare_params(params, group, stream, dist_solve)
        nco = params.num_coarsenings
        A = ParCsr()
        A.global_rows = int(piece.get("global_rows", 0))
        rs = piece.get("row_starts")
        self._keep = [piece, rs]
        A.row_starts = _ptr(rs).value if rs is not None else None
        A.nrows = int(piece["nrows"])
        for k in ("diag_i", "diag_j", "diag_a", "offd_i", "offd_j", "offd_a", "col_map_offd"):
            setattr(A, k, _ptr(piece.get(k)).value)
        A.num_cols_offd = int(piece.get("num_cols_offd", 0))
        parts = (C.c_void_p * nco)(*[_ptr(p).value for p in piece["partitions"][:nco]])
        npa = (C.c_int * nco)(*[int(x) for x in piece["nparts"][:nco]])
        h = C.c_void_p()
        e2d = piece["elem_to_dof"]
        _check(lib.saamge_amd_ml_produce_data_parcsr(C.byref(A), C.c_int(int(e2d.shape[0])), C.c_int(int(e2d.shape[1])), _ptr(e2d),
                                                     _ptr(piece["elmat"]), _ptr(piece.get("bdr")), parts, npa, C.byref(params),
                                                     C.c_void_p(stream), C.byref(h)))
        self.h = h
        self.n = int(self.level_info(0)["n"])
        self.testmesh = False
        return self

    @classmethod
    def from_matrix(cls, A, dof_partition, params, coarse_partitions=(), stream=0, group=None):
        """Element-free (algebraic) mode: only the matrix and a map dof -> AE
        (tg_produce_data_algebraic, amg/src/tg.cpp:862-886).  `params.algebraic` must be set."""
        A = A.tocsr()
        A.sort_indices()
        rowptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
        col = np.ascontiguousarray(A.indices, dtype=np.int32)
        val = np.ascontiguousarray(A.data, dtype=np.float64)
        parts = [np.ascontiguousarray(p, dtype=np.int32) for p in (dof_partition,) + tuple(coarse_partitions)]
        nparts = [int(p.max()) + 1 for p in parts]
        return cls(rowptr, col, val, A.shape[0], None, None, None, parts, nparts, params, A.shape[0], 1,
                   stream, group)

    def update_operators(self, new_val=None, coarse_solver=None):
        """adapt_update_operators: new matrix values (same pattern), interpolations kept.  coarse_solver (1 dense
        inverse, 2 inner PCG, 0 auto): tg_update_coarse_operator's coarse_direct -- the coarsest solver is chosen again."""
        if new_val is not None:
            new_val = np.ascontiguousarray(new_val, dtype=np.float64) if not hasattr(new_val, "data_ptr") else new_val
        if coarse_solver is None:
            _check(load().saamge_amd_update_operators(self.h, _ptr(new_val)))
        else:
            _check(load().saamge_amd_update_operators2(self.h, _ptr(new_val), C.c_int(int(coarse_solver))))

    # ---- solve ----
    def vcycle(self, b, x=None):
        if x is None:
            x = np.zeros_like(b)
        _check(load().saamge_amd_vcycle_mult(self.h, _ptr(b), _ptr(x)))
        return x

    def vcycle_iterative(self, b, x):
        """VCycleSolver::Mult with iterative_mode = true: x <- x + B (b - A x)."""
        _check(load().saamge_amd_vcycle(self.h, _ptr(b), _ptr(x), C.c_int(1)))
        return x

    def set_coarse_solver(self, fn):
        """tg_data_t::coarse_solver plug: fn(rc: ndarray) -> xc: ndarray on the host, or None for the built-in solver."""
        if fn is None:
            self._coarse_cb = None
            _check(load().saamge_amd_set_coarse_solver(self.h, None, None))
            return

        def tramp(ctx, n, rc, xc):
            try:
                r = np.ctypeslib.as_array(rc, shape=(n,))
                out = np.ctypeslib.as_array(xc, shape=(n,))
                out[:] = fn(r.copy())
                return 0
            except Exception as e:
                import sys
                print("coarse solver callback failed: %r" % (e,), file=sys.stderr)
                return 1
        self._coarse_cb = COARSE_SOLVE_FN(tramp)
        _check(load().saamge_amd_set_coarse_solver(self.h, self._coarse_cb, None))

    def set_smoother(self, level, pre, post):
        """The smpr_ft plug (inc/smpr.hpp:59-60): pre / post = fn(level, b: ndarray, x: ndarray) -> new x with the semantics
        x += M^-1 (b - A x) on the host, or None for the built-in polynomial smoother in that place."""
        def wrap(fn):
            if fn is None:
                return SMOOTHER_FN()
            def tramp(ctx, lev, n, bp, xp):
                try:
                    bb = np.ctypeslib.as_array(bp, shape=(n,))
                    xx = np.ctypeslib.as_array(xp, shape=(n,))
                    xx[:] = fn(lev, bb.copy(), xx.copy())
                    return 0
                except Exception as e:
                    import sys
                    print("smoother callback failed: %r" % (e,), file=sys.stderr)
                    return 1
            return SMOOTHER_FN(tramp)
        if not hasattr(self, "_smoother_cbs"):
            self._smoother_cbs = {}
        self._smoother_cbs[level] = (wrap(pre), wrap(post))
        _check(load().saamge_amd_set_smoother(self.h, C.c_int(level), self._smoother_cbs[level][0],
                                              self._smoother_cbs[level][1], None))

    def smoother(self, level, b, x):
        _check(load().saamge_amd_smoother(self.h, C.c_int(level), _ptr(b), _ptr(x)))
        return x

    def pcg(self, b, x=None, rel_tol=1e-6, abs_tol=0.0, max_iter=1000, squared_tol=True,
            zero_guess=True):
        if x is None:
            x = np.zeros_like(b)
        it = C.c_int(0)
        conv = C.c_int(0)
        hist = np.zeros(max_iter + 2)
        _check(load().saamge_amd_pcg(self.h, _ptr(b), _ptr(x), C.c_double(rel_tol),
                                     C.c_double(abs_tol), C.c_int(max_iter), C.c_int(int(squared_tol)),
                                     C.c_int(int(zero_guess)), C.byref(it), C.byref(conv), _ptr(hist)))
        return x, it.value, bool(conv.value), hist[:it.value + 1].copy()

    # ---- block solves: k columns per call.  A block is column-major with a leading dimension: a C-contiguous numpy array of
    # shape (k, ld) whose row j is column j (ld >= n; the entries past n are padding and stay untouched), or a device
    # pointer / tensor with `ld` given.  Column j of every result is bit for bit the single-vector call on column j.
    @staticmethod
    def _ld(a, ld):
        return int(ld) if ld is not None else int(a.shape[1])

    def smoother_block(self, level, B, X, k=None, ldb=None, ldx=None):
        k = int(k if k is not None else B.shape[0])
        _check(load().saamge_amd_smoother_block(self.h, C.c_int(level), C.c_int(k), _ptr(B), C.c_longlong(self._ld(B, ldb)),
                                                _ptr(X), C.c_longlong(self._ld(X, ldx))))
        return X

    def vcycle_block(self, B, X, iterative_mode=False, k=None, ldb=None, ldx=None):
        k = int(k if k is not None else B.shape[0])
        _check(load().saamge_amd_vcycle_block(self.h, C.c_int(k), _ptr(B), C.c_longlong(self._ld(B, ldb)), _ptr(X),
                                              C.c_longlong(self._ld(X, ldx)), C.c_int(int(iterative_mode))))
        return X

    def pcg_block(self, B, X, rel_tol=1e-6, abs_tol=0.0, max_iter=1000, squared_tol=True, zero_guess=True, k=None, ldb=None,
                  ldx=None, hist=None, iters=None, converged=None):
        """-> X, iters (k,), converged (k,), hist (k, max_iter + 1): row j is column j's history, written up to its own last
        step (the rest keeps what `hist` held: NaN in a new array)."""
        k = int(k if k is not None else B.shape[0])
        iters = np.zeros(max(k, 1), dtype=np.int32) if iters is None else iters
        converged = np.zeros(max(k, 1), dtype=np.int32) if converged is None else converged
        if hist is None:
            hist = np.full((max(k, 1), max(max_iter, 0) + 1), np.nan)
        _check(load().saamge_amd_pcg_block(self.h, C.c_int(k), _ptr(B), C.c_longlong(self._ld(B, ldb)), _ptr(X),
                                           C.c_longlong(self._ld(X, ldx)), C.c_double(rel_tol), C.c_double(abs_tol),
                                           C.c_int(max_iter), C.c_int(int(squared_tol)), C.c_int(int(zero_guess)), _ptr(iters),
                                           _ptr(converged), _ptr(hist)))
        return X, iters, converged, hist

    def lobpcg(self, nev, block=0, M=None, x0=None, tol=1e-8, max_iter=100, constrain_essential=True, seed=0, evecs=None):
        """The lowest nev pairs of A x = lambda M x (saamge_amd_lobpcg; the definition: saamge_amd.lobpcg_model).  M: None,
        a scipy matrix, or (rowptr, col, val) with 64-bit offsets (numpy arrays or device pointers / tensors); x0: n x nb
        (numpy, any layout; or a device pointer / tensor holding it column-major); evecs: a device pointer / tensor for
        n x nev column-major, or None.  -> lam, X (n x nev; `evecs` itself when given), res, iters, converged, hist."""
        n = int(self.level_info(0)["n"])
        nb = block or nev
        o = LobpcgOptions()
        load().saamge_amd_lobpcg_options_default(C.byref(o))
        o.nev, o.block, o.tol, o.max_iter = int(nev), int(block), float(tol), int(max_iter)
        o.constrain_essential, o.seed = int(bool(constrain_essential)), int(seed)
        if M is None:
            m = (None, None, None)
        elif isinstance(M, tuple):
            m = M
        else:
            import scipy.sparse as sp
            M = sp.csr_matrix(M)
            m = (np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.int32),
                 np.ascontiguousarray(M.data, dtype=np.float64))
        if isinstance(x0, np.ndarray):
            assert x0.shape == (n, nb)
            x0 = np.ascontiguousarray(x0.T, dtype=np.float64)       # column-major n x nb
        lam, res = np.zeros(max(nev, 0)), np.zeros(max(nev, 0))
        X = np.zeros((max(nev, 0), n)) if evecs is None else evecs
        hist = np.zeros((max(max_iter, 0) + 1, max(nev, 0)))
        it, conv = C.c_int(0), C.c_int(0)
        _check(load().saamge_amd_lobpcg(self.h, _ptr(m[0]), _ptr(m[1]), _ptr(m[2]), C.byref(o), _ptr(x0), _ptr(lam), _ptr(X),
                                        _ptr(res), C.byref(it), C.byref(conv), _ptr(hist)))
        return lam, (X.T if evecs is None else evecs), res, it.value, int(conv.value), hist[:it.value + 1].copy()

    # ---- inspection ----
    @property
    def num_levels(self):
        return load().saamge_amd_num_levels(self.h)

    def level_info(self, level):
        info = (C.c_longlong * 16)()
        _check(load().saamge_amd_level_info(self.h, C.c_int(level), info))
        keys = ["n", "nnz", "nparts", "num_mises", "ncoarse", "nnzP", "nnzAc", "nvec",
                "coarse_iters", "evecs_size", "sig_size", "U_size", "row_partitioned", "row0",
                "own_rows", "halo_recv"]
        return dict(zip(keys, [int(v) for v in info[:len(keys)]]))

    def coarse_solver_info(self):
        """The coarsest solver in use: kind (1 dense inverse, 2 inner PCG, 3 block-tridiagonal, 0 the caller's plug), rows
        of the coarsest operator, blocks / largest block of the block-tridiagonal structure, doubles of explicit inverses."""
        info = (C.c_longlong * 8)()
        _check(load().saamge_amd_coarse_solver_info(self.h, info))
        keys = ["kind", "n", "nblk", "max_block", "inverse_doubles"]
        return dict(zip(keys, [int(v) for v in info[:len(keys)]]))

    def level_format(self, level):
        info = (C.c_longlong * 12)()
        _check(load().saamge_amd_level_format(self.h, C.c_int(level), info))
        v = [int(x) for x in info]
        return {"slices": {"pair_coded": v[0], "offset_coded": v[1], "plain": v[2]},
                "entries": {"pair_coded": v[3], "offset_coded": v[4], "plain": v[5]},
                "staged_tiles": v[6], "stream_bytes": v[7],
                "dictionary_pairs": v[8], "node_blocks": bool(v[9]), "irregular_rows": v[10],
                "eigenproblems_solved": v[11]}

    def level_order_info(self, level):
        """[agglomerates given a permutation, those that took the level order, largest bw0, largest bandwidth in use]"""
        info = (C.c_longlong * 4)()
        _check(load().saamge_amd_level_order_info(self.h, C.c_int(level), info))
        return [int(x) for x in info]

    def get_csr(self, level, which):
        import scipy.sparse as sp
        info = self.level_info(level)
        which_id = {"A": 0, "P": 1, "R": 2, "Ac": 3}[which]
        nrows, ncols, nnz = {
            "A": (info["n"], info["n"], info["nnz"]),
            "P": (info["n"], info["ncoarse"], info["nnzP"]),
            "R": (info["ncoarse"], info["n"], info["nnzP"]),
            "Ac": (info["ncoarse"], info["ncoarse"], info["nnzAc"]),
        }[which]
        rowptr = np.zeros(nrows + 1, dtype=np.int32)
        col = np.zeros(nnz, dtype=np.int32)
        val = np.zeros(nnz, dtype=np.float64)
        _check(load().saamge_amd_get_csr(self.h, C.c_int(level), C.c_int(which_id), _ptr(rowptr),
                                         _ptr(col), _ptr(val)))
        return sp.csr_matrix((val, col, rowptr), shape=(nrows, ncols))

    def get_table(self, level, name):
        wid = {"AE_to_dof": 0, "dof_to_AE": 1, "mis_to_dof": 2, "mis_to_AE": 3, "AE_to_mis": 4,
               "elem_to_dof": 5}[name]
        nrows = C.c_int(0)
        nconn = C.c_longlong(0)
        _check(load().saamge_amd_get_table(self.h, C.c_int(level), C.c_int(wid), C.byref(nrows),
                                           C.byref(nconn), None, None))
        I = np.zeros(nrows.value + 1, dtype=np.int32)
        J = np.zeros(nconn.value, dtype=np.int32)
        _check(load().saamge_amd_get_table(self.h, C.c_int(level), C.c_int(wid), None, None,
                                           _ptr(I), _ptr(J)))
        return I, J

    def get_mis(self, level):
        info = self.level_info(level)
        mises = np.zeros(info["n"], dtype=np.int32)
        k = np.zeros(info["num_mises"], dtype=np.int32)
        nc = np.zeros(info["num_mises"], dtype=np.int32)
        flags = np.zeros(info["n"], dtype=np.int8)
        _check(load().saamge_amd_get_mis(self.h, C.c_int(level), _ptr(mises), _ptr(k), _ptr(nc),
                                         _ptr(flags)))
        return mises, k, nc, flags

    def get_ae_eigens(self, level):
        """Returns (m, evals_list, evecs_list, D_list) per AE (needs keep_debug)."""
        info = self.level_info(level)
        I, _ = self.get_table(level, "AE_to_dof")
        sizes = np.diff(I)
        m = np.zeros(info["nparts"], dtype=np.int32)
        _check(load().saamge_amd_get_ae_eigens(self.h, C.c_int(level), _ptr(m), None, None, None))
        evecs = np.zeros(info["evecs_size"])
        evals = np.zeros(max(int(m.sum()), 1))
        D = np.zeros(int(sizes.sum()))
        _check(load().saamge_amd_get_ae_eigens(self.h, C.c_int(level), _ptr(m), _ptr(evals),
                                               _ptr(evecs), _ptr(D)))
        ev, X, Ds = [], [], []
        xo = eo = do = 0
        for i, n in enumerate(sizes):
            cnt = int(m[i])
            X.append(evecs[xo:xo + n * cnt].reshape(cnt, n).T.copy())
            xo += n * cnt
            Ds.append(D[do:do + n].copy())
            do += n
            # eigenvalues exist only for computed pairs (not for the mltest fixture's ones-vector)
            ne = cnt - 1 if (self.testmesh and level == 0 and i == 0) else cnt
            ev.append(evals[eo:eo + ne].copy())
            eo += ne
        return m, ev, X, Ds

    def get_mis_svd(self, level):
        info = self.level_info(level)
        nm = info["num_mises"]
        off = np.zeros(nm + 1, dtype=np.int64)
        sig = np.zeros(max(info["sig_size"], 1))
        U = np.zeros(max(info["U_size"], 1))
        _check(load().saamge_amd_get_mis_svd(self.h, C.c_int(level), _ptr(off), _ptr(sig), _ptr(U)))
        return off, sig, U


def spmv_raw(nrows, ncols, rowptr, col, val, x, y):
    """y = A x on raw arrays (numpy or torch; host or device); 64-bit row offsets when rowptr is int64."""
    wide = str(getattr(rowptr, "dtype", "")).endswith("int64")
    fn = load().saamge_amd_spmv64 if wide else load().saamge_amd_spmv
    _check(fn(C.c_int(nrows), C.c_int(ncols), _ptr(rowptr), _ptr(col), _ptr(val), _ptr(x), _ptr(y)))
    return y


def spmv(A, x):
    A = A.tocsr()
    y = np.zeros(A.shape[0])
    _check(load().saamge_amd_spmv(C.c_int(A.shape[0]), C.c_int(A.shape[1]),
                                  _ptr(np.ascontiguousarray(A.indptr, dtype=np.int32)),
                                  _ptr(np.ascontiguousarray(A.indices, dtype=np.int32)),
                                  _ptr(np.ascontiguousarray(A.data, dtype=np.float64)),
                                  _ptr(np.ascontiguousarray(x, dtype=np.float64)), _ptr(y)))
    return y


def spmv_block(A, X, Y, k=None, ldx=None, ldy=None):
    """Y[j] = A X[j] for the k columns of a block (saamge_amd_spmv_block; honours spmv_sell like spmv).  X: (k, ldx), Y: (k, ldy)
    C-contiguous numpy arrays (row j = column j of the column-major block), or device pointers with the leading dimensions."""
    A = A.tocsr()
    k = int(k if k is not None else X.shape[0])
    _check(load().saamge_amd_spmv_block(C.c_int(A.shape[0]), C.c_int(A.shape[1]),
                                        _ptr(np.ascontiguousarray(A.indptr, dtype=np.int32)),
                                        _ptr(np.ascontiguousarray(A.indices, dtype=np.int32)),
                                        _ptr(np.ascontiguousarray(A.data, dtype=np.float64)), C.c_int(k), _ptr(X),
                                        C.c_longlong(int(ldx) if ldx is not None else int(X.shape[1])), _ptr(Y),
                                        C.c_longlong(int(ldy) if ldy is not None else int(Y.shape[1]))))
    return Y


def lower_eigens_batched(mats, diags, vl, vu):
    """mats: list of symmetric (n_i, n_i) arrays; diags: list of positive (n_i,) arrays."""
    count = len(mats)
    n = np.array([m.shape[0] for m in mats], dtype=np.int32)
    A = np.concatenate([np.asfortranarray(m).ravel(order="F") for m in mats])
    D = np.concatenate([np.asarray(d, dtype=np.float64) for d in diags])
    m_out = np.zeros(count, dtype=np.int32)
    evals = np.zeros(int(n.sum()))
    evecs = np.zeros(int((n.astype(np.int64) ** 2).sum()))
    _check(load().saamge_amd_lower_eigens_batched(C.c_int(count), _ptr(n), _ptr(A), _ptr(D),
                                                  C.c_double(vl), C.c_double(vu), _ptr(m_out),
                                                  _ptr(evals), _ptr(evecs)))
    out = []
    vo = 0
    mo = 0
    for i in range(count):
        ni, mi = int(n[i]), int(m_out[i])
        out.append((evals[vo:vo + mi].copy(), evecs[mo:mo + ni * mi].reshape(mi, ni).T.copy()))
        vo += ni
        mo += ni * ni
    return out


def inertia_batched(mats, diags, vu):
    """Number of eigenvalues of A_i x = lambda D_i x below vu per matrix (-1: not certifiable)."""
    count = len(mats)
    n = np.array([m.shape[0] for m in mats], dtype=np.int32)
    A = np.concatenate([np.asfortranarray(m).ravel(order="F") for m in mats])
    D = np.concatenate([np.asarray(d, dtype=np.float64) for d in diags])
    neg = np.zeros(count, dtype=np.int32)
    _check(load().saamge_amd_inertia_batched(C.c_int(count), _ptr(n), _ptr(A), _ptr(D), C.c_double(vu), _ptr(neg)))
    return neg


# ---- the general sparse products on their own (csrc/spgemm.hip) ----
ROUTE_NONE, ROUTE_DENSE_B = -1, 3      # saamge_amd_spgemm's *route; 0, 1, 2: the hash path and its table tier


def _csr_arrays(M):
    """(indptr, indices, data) of a scipy CSR matrix AS STORED (no sorting, no summing: the order of a row is part of
    what the kernels are given)"""
    return (np.ascontiguousarray(M.indptr, dtype=np.int32), np.ascontiguousarray(M.indices, dtype=np.int32),
            np.ascontiguousarray(M.data, dtype=np.float64))


def _csr_result(shape, call):
    """call(rowptr, nnz_ref, col, val): first for the sizes, then for the entries"""
    import scipy.sparse as sp
    rowptr = np.zeros(shape[0] + 1, dtype=np.int32)
    nnz = C.c_longlong(0)
    call(rowptr, nnz, None, None)
    col = np.zeros(nnz.value, dtype=np.int32)
    val = np.zeros(nnz.value, dtype=np.float64)
    if nnz.value:
        call(rowptr, nnz, col, val)
    return sp.csr_matrix((val, col, rowptr), shape=shape)


def spgemm(A, B, E=None, d=None, alpha=1.0, beta=0.0):
    """(C, route): C = beta E + alpha diag(d) A B as a scipy CSR matrix and the route of saamge_amd_spgemm.  A, B, E: scipy
    CSR matrices, passed as stored; `E is B` passes B's arrays twice (one matrix on the device too)."""
    a, b = _csr_arrays(A), _csr_arrays(B)
    e = b if E is B else (_csr_arrays(E) if E is not None else (None, None, None))
    dd = None if d is None else np.ascontiguousarray(d, dtype=np.float64)
    route = C.c_int(ROUTE_NONE)

    def call(rowptr, nnz, col, val):
        _check(load().saamge_amd_spgemm(C.c_int(A.shape[0]), C.c_int(A.shape[1]), C.c_int(B.shape[1]), _ptr(a[0]), _ptr(a[1]),
                                        _ptr(a[2]), _ptr(b[0]), _ptr(b[1]), _ptr(b[2]), _ptr(e[0]), _ptr(e[1]), _ptr(e[2]),
                                        _ptr(dd), C.c_double(alpha), C.c_double(beta), _ptr(rowptr), C.byref(nnz), _ptr(col),
                                        _ptr(val), C.byref(route)))
    out = _csr_result((A.shape[0], B.shape[1]), call)
    return out, int(route.value)


def csr_transpose(P):
    p = _csr_arrays(P)

    def call(rowptr, nnz, col, val):
        _check(load().saamge_amd_csr_transpose(C.c_int(P.shape[0]), C.c_int(P.shape[1]), _ptr(p[0]), _ptr(p[1]), _ptr(p[2]),
                                               _ptr(rowptr), C.byref(nnz), _ptr(col), _ptr(val)))
    return _csr_result((P.shape[1], P.shape[0]), call)


def csr_threshold(A, tol):
    a = _csr_arrays(A)

    def call(rowptr, nnz, col, val):
        _check(load().saamge_amd_csr_threshold(C.c_int(A.shape[0]), C.c_int(A.shape[1]), _ptr(a[0]), _ptr(a[1]), _ptr(a[2]),
                                               C.c_double(tol), _ptr(rowptr), C.byref(nnz), _ptr(col), _ptr(val)))
    return _csr_result(A.shape, call)


def release_cached_memory():
    """Return the library's cached device blocks and the eigensolver workspace to the driver."""
    load().saamge_amd_release_cached_memory()


def cached_memory_bytes():
    lib = load()
    lib.saamge_amd_cached_memory_bytes.restype = C.c_longlong
    return int(lib.saamge_amd_cached_memory_bytes())


def ae_order(ND, elem_to_dof, elem_to_ae, nparts, mode, elem_ptr=None):
    """saamge_amd_ae_order: (ae_ptr, ae_to_dof, pos, bw0, bw, choice) as numpy int32 arrays.  elem_ptr None: elem_to_dof is
    (NE, nde); otherwise flat elem_to_dof with NE + 1 offsets."""
    e2d = np.ascontiguousarray(elem_to_dof, dtype=np.int32)
    part = np.ascontiguousarray(elem_to_ae, dtype=np.int32)
    ep = None if elem_ptr is None else np.ascontiguousarray(elem_ptr, dtype=np.int32)
    NE = len(part)
    nde = 0 if ep is not None else int(e2d.shape[1])
    ae_ptr = np.zeros(max(int(nparts), 0) + 1, np.int32)
    nconn = C.c_longlong(0)

    def call(j, pos, bw0, bw, choice):
        _check(load().saamge_amd_ae_order(C.c_int(ND), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2d), _ptr(part),
                                          C.c_int(nparts), C.c_int(mode), _ptr(ae_ptr), C.byref(nconn), _ptr(j), _ptr(pos),
                                          _ptr(bw0), _ptr(bw), _ptr(choice)))
    call(None, None, None, None, None)
    j, pos = np.zeros(nconn.value, np.int32), np.zeros(nconn.value, np.int32)
    bw0, bw, choice = (np.zeros(nparts, np.int32) for _ in range(3))
    call(j, pos, bw0, bw, choice)
    return ae_ptr, j, pos, bw0, bw, choice


ELEMENT_TYPES = ("triangles", "quadrilaterals", "tetrahedra", "wedges", "hexahedra")


def _element_matrices_call(coords, elem_to_vertex, kind, coef, elem_ptr, stream, elmat, dof_ptr, e2d,
                           fn="saamge_amd_element_matrices"):
    """One saamge_amd_element_matrices call on prepared arrays; returns info (8 integers).  A refusal raises RuntimeError with
    the library's message, and `.info` on it holds what the call had filled in by then (info[6]: the first element with a
    non-positive Jacobian).  fn: the call itself or saamge_amd_element_matrices_points, which has its arguments (coef: coefq)."""
    NV, dim = int(coords.shape[0]), int(coords.shape[1])
    NE = len(elem_ptr) - 1 if elem_ptr is not None else int(elem_to_vertex.shape[0])
    nde = 0 if elem_ptr is not None else int(elem_to_vertex.shape[1])
    ncoef = 1 if len(coef.shape) == 1 else int(coef.shape[1])
    info = (C.c_longlong * 8)()
    rc = getattr(load(), fn)(C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(elem_ptr),
                             _ptr(elem_to_vertex), C.c_int(int(kind)), C.c_int(ncoef), _ptr(coef),
                             C.c_void_p(stream), _ptr(elmat), _ptr(dof_ptr), _ptr(e2d), info)
    if rc != 0:
        err = RuntimeError("saamge_amd: " + load().saamge_amd_last_error().decode())
        err.info = [int(v) for v in info]
        raise err
    return [int(v) for v in info]


def _element_arrays(coords, elem_to_vertex, coef, elem_ptr):
    def arr(a, dt):          # device tensors pass through, host arrays are made contiguous
        return a if a is None or hasattr(a, "data_ptr") else np.ascontiguousarray(a, dtype=dt)
    return arr(coords, np.float64), arr(elem_to_vertex, np.int32), arr(coef, np.float64), arr(elem_ptr, np.int32)


def element_matrices_info(coords, elem_to_vertex, kind, coef, elem_ptr=None, stream=0):
    """The sizes-only call (elmat_out = NULL): info = [triangles, quadrilaterals, tetrahedra, wedges, hexahedra (the order-1
    elements), doubles the matrices take, -1, order-2 elements (9-node quadrilaterals, 27-node hexahedra, 6-node triangles,
    10-node tetrahedra)].  Nothing is
    written; the mesh and the Jacobians are checked all the same."""
    coords, e2v, coef, ep = _element_arrays(coords, elem_to_vertex, coef, elem_ptr)
    return _element_matrices_call(coords, e2v, kind, coef, ep, stream, None, None, None)


def element_matrices(coords, elem_to_vertex, kind, coef, elem_ptr=None, device=False, dofs=False, out=None, stream=0):
    """saamge_amd_element_matrices: the element matrices of a mesh from its vertex coordinates (NV x dim), element -> vertex
    lists ((NE, nodes), or flat with elem_ptr) and per-element coefficients ((NE,) or (NE, ncoef)); kind 0 diffusion, 1
    elasticity.  Lists of 9 (2D) / 27 (3D) nodes are the order-2 quadrilateral (MFEM's H1 order: vertices, edge midpoints,
    centre) / hexahedron (lexicographic), lists of 6 (2D) / 10 (3D) nodes the order-2 triangle / tetrahedron (the vertices, then
    the edge midpoints in the order of elmat_model.P2_EDGES; problems.p2_simplex_nodes makes such lists from a vertex mesh);
    coords then holds all nodes, and the elements may be curved (elmat_model.py).
    Inputs: numpy arrays or device tensors, each on its own.  Returns elmat -- (NE, size, size), or packed in
    element order with elem_ptr -- as a numpy array, or with device=True as a torch tensor on the GPU whose data_ptr goes to
    `Operator` and `Hierarchy.from_operator` unchanged; out: an array / tensor of that many doubles to write into instead of
    a new one.  dofs=True: (elmat, dof_ptr, elem_to_dof), the int32 dof lists the matrices are indexed by (elem_to_dof
    (NE, size) without elem_ptr, else flat)."""
    return _element_matrices(coords, elem_to_vertex, kind, coef, elem_ptr, device, dofs, out, stream, "saamge_amd_element_matrices")


def _element_matrices(coords, elem_to_vertex, kind, coef, elem_ptr, device, dofs, out, stream, fn):
    coords, e2v, coef, ep = _element_arrays(coords, elem_to_vertex, coef, elem_ptr)
    comp = int(coords.shape[1]) if kind == 1 else 1
    if ep is None:
        NE, nconn = int(e2v.shape[0]), int(e2v.shape[0]) * int(e2v.shape[1])
        doubles = NE * (int(e2v.shape[1]) * comp) ** 2
    else:
        NE, nconn = len(ep) - 1, int(e2v.shape[0])
        nd = (ep[1:] - ep[:-1]) * comp
        doubles = int((nd.long() ** 2).sum()) if hasattr(nd, "data_ptr") else int((nd.astype(np.int64) ** 2).sum())

    def new(n, np_dt, torch_dt):
        if device:
            import torch
            return torch.zeros(n, dtype=getattr(torch, torch_dt), device="cuda")
        return np.zeros(max(n, 1), np_dt)[:n]
    elmat = out if out is not None else new(doubles, np.float64, "float64")
    dof_ptr = new(NE + 1, np.int32, "int32") if dofs else None
    e2d = new(nconn * comp, np.int32, "int32") if dofs else None
    _element_matrices_call(coords, e2v, kind, coef, ep, stream, elmat, dof_ptr, e2d, fn)
    if ep is None:
        size = int(e2v.shape[1]) * comp
        elmat = elmat.reshape(NE, size, size)
        e2d = e2d.reshape(NE, size) if dofs else None
    return (elmat, dof_ptr, e2d) if dofs else elmat


def _mass_call(fn, info):
    rc = fn()
    if rc != 0:
        err = RuntimeError("saamge_amd: " + load().saamge_amd_last_error().decode())
        err.info = [int(v) for v in info]
        raise err
    return [int(v) for v in info]


def _mass_sizes(coords, e2v, ep, vdim, square):
    """(NV, dim, NE, nde, doubles of the packed result)"""
    NV, dim = int(coords.shape[0]), int(coords.shape[1])
    if ep is None:
        NE, nde = int(e2v.shape[0]), int(e2v.shape[1])
        return NV, dim, NE, nde, NE * (nde * vdim) ** 2 if square else NE * nde * vdim
    nd = (ep[1:] - ep[:-1]) * vdim
    nd = nd.long() if hasattr(nd, "data_ptr") else nd.astype(np.int64)
    return NV, dim, len(ep) - 1, 0, int((nd ** 2).sum()) if square else int(nd.sum())


def _new_doubles(n, device):
    if device:
        import torch
        return torch.zeros(n, dtype=torch.float64, device="cuda")
    return np.zeros(max(n, 1), np.float64)[:n]


def element_mass(coords, elem_to_vertex, coef, vdim=1, elem_ptr=None, add_to=None, device=False, out=None, stream=0,
                 sizes_only=False):
    """saamge_amd_element_mass: the mass matrices (c u, v) of a mesh, c = coef (NE,), on the types and in the layout of
    `element_matrices`; vdim 1, or dim for the dof layout of elasticity.  add_to: an array / tensor that holds matrices of that
    layout (the output of `element_matrices`); the mass matrices are added to it IN PLACE and it is returned -- K + sigma M with
    sigma in coef.  Otherwise as `element_matrices`: inputs numpy arrays or device tensors, each on its own; device=True: a
    torch tensor on the GPU; out: doubles to write into.  sizes_only: info (8 integers), nothing written.  A refusal raises
    RuntimeError with `.info`.  The order-2 simplices have mass rules of their own (6 / 14 points): a curved element can be
    refused here that `element_matrices` accepts."""
    coords, e2v, coef, ep = _element_arrays(coords, elem_to_vertex, coef, elem_ptr)
    vdim = int(vdim)
    NV, dim, NE, nde, doubles = _mass_sizes(coords, e2v, ep, vdim, True)
    info = (C.c_longlong * 8)()
    if sizes_only:
        elmat = None
    elif add_to is not None:
        elmat = add_to
    else:
        elmat = out if out is not None else _new_doubles(doubles, device)
    got = _mass_call(lambda: load().saamge_amd_element_mass(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(vdim), _ptr(coef),
        C.c_void_p(stream), C.c_int(1 if add_to is not None else 0), _ptr(elmat), info), info)
    if sizes_only:
        return got
    if ep is None and add_to is None:
        elmat = elmat.reshape(NE, nde * vdim, nde * vdim)
    return elmat


def element_loads(coords, elem_to_vertex, src, vdim=1, coef=None, elem_ptr=None, device=False, out=None, stream=0):
    """saamge_amd_element_loads: the load vectors (c f, v) of the source f given at the nodes, src (NV, vdim) or (NV,); coef
    (NE,), None: 1.  Returns (NE, size) or, with elem_ptr, the packed vectors `Operator.assemble_rhs` takes; device=, out=,
    stream= as in `element_matrices`."""
    coords, e2v, coef, ep = _element_arrays(coords, elem_to_vertex, coef, elem_ptr)
    if src is not None and not hasattr(src, "data_ptr"):
        src = np.ascontiguousarray(src, dtype=np.float64)
    vdim = int(vdim)
    NV, dim, NE, nde, doubles = _mass_sizes(coords, e2v, ep, vdim, False)
    info = (C.c_longlong * 8)()
    elvec = out if out is not None else _new_doubles(doubles, device)
    _mass_call(lambda: load().saamge_amd_element_loads(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(vdim), _ptr(coef),
        _ptr(src), C.c_void_p(stream), _ptr(elvec), info), info)
    return elvec.reshape(NE, nde * vdim) if ep is None else elvec


# ---- data at the points of the mass rule (elmat_model.element_points / _eval / _loads_points / _errors) ----
def _num_points(coords, e2v, ep):
    """NQ: the points of the mass rules of all elements"""
    from .elmat_model import MASS_NPOINTS
    dim = int(coords.shape[1])
    if ep is None:
        return int(e2v.shape[0]) * MASS_NPOINTS.get((dim, int(e2v.shape[1])), 0)
    nd = ep[1:] - ep[:-1]
    nd = nd.cpu().numpy() if hasattr(nd, "data_ptr") else np.asarray(nd)
    return int(sum(int((nd == k).sum()) * n for (d, k), n in MASS_NPOINTS.items() if d == dim))


def _doubles(a):
    return a if a is None or hasattr(a, "data_ptr") else np.ascontiguousarray(a, dtype=np.float64)


def _new_or(out, n, device, want):
    """the output array of a call: `out`, or new zeros when it is wanted"""
    if out is not None:
        return out
    return _new_doubles(n, device) if want else None


def element_points(coords, elem_to_vertex, elem_ptr=None, device=False, want=("qp_ptr", "xq", "wdet"), out=None, stream=0,
                   sizes_only=False):
    """saamge_amd_element_points: (qp_ptr (NE + 1,) int64, xq (NQ, dim), wdet (NQ,)) -- the points of every element's mass rule
    (point q of element e: index qp_ptr[e] + q), their physical coordinates and weight * det there.  want: which of the three
    are asked for, the others are passed as NULL and come back None; out: a dict of arrays / tensors to write into, by the same
    names.  device=True: torch tensors on the GPU.  sizes_only: info (8 integers: the type counts in [0..4] and [7], [5] = NQ).
    A refusal raises RuntimeError with `.info` (info[6]: the first element with a non-positive determinant)."""
    coords, e2v, _, ep = _element_arrays(coords, elem_to_vertex, None, elem_ptr)
    NV, dim, NE, nde, _ = _mass_sizes(coords, e2v, ep, 1, False)
    out = dict(out or {})
    want = () if sizes_only else tuple(want)
    NQ = _num_points(coords, e2v, ep)
    qp = out.get("qp_ptr")
    if qp is None and "qp_ptr" in want:
        qp = _new_ints(NE + 1, np.int64, "int64", device)
    xq = _new_or(out.get("xq"), NQ * dim, device, "xq" in want)
    wdet = _new_or(out.get("wdet"), NQ, device, "wdet" in want)
    info = (C.c_longlong * 8)()
    got = _mass_call(lambda: load().saamge_amd_element_points(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_void_p(stream), _ptr(qp),
        _ptr(xq), _ptr(wdet), info), info)
    if sizes_only:
        return got
    return qp, None if xq is None else xq.reshape(NQ, dim), wdet


def element_eval(coords, elem_to_vertex, u, vdim=1, elem_ptr=None, device=False, want=("uq", "gradq"), out=None, stream=0):
    """saamge_amd_element_eval: (uq (NQ, vdim), gradq (NQ, vdim, dim)) of the nodal field u, (NV, vdim) or (NV,), at the points of
    `element_points`; gradq[q, i, j] is the derivative of component i along x_j.  want / out / device / stream as there."""
    coords, e2v, _, ep = _element_arrays(coords, elem_to_vertex, None, elem_ptr)
    vdim = int(vdim)
    NV, dim, NE, nde, _ = _mass_sizes(coords, e2v, ep, vdim, False)
    out = dict(out or {})
    NQ = _num_points(coords, e2v, ep)
    uq = _new_or(out.get("uq"), NQ * vdim, device, "uq" in want)
    gq = _new_or(out.get("gradq"), NQ * vdim * dim, device, "gradq" in want)
    info = (C.c_longlong * 8)()
    _mass_call(lambda: load().saamge_amd_element_eval(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(vdim), _ptr(_doubles(u)),
        C.c_void_p(stream), _ptr(uq), _ptr(gq), info), info)
    return None if uq is None else uq.reshape(NQ, vdim), None if gq is None else gq.reshape(NQ, vdim, dim)


def element_loads_points(coords, elem_to_vertex, fq, vdim=1, coef=None, elem_ptr=None, device=False, out=None, stream=0):
    """saamge_amd_element_loads_points: the load vectors (c f, v) of a source given AT THE POINTS of `element_points`, fq
    (NQ, vdim) or (NQ,); coef (NE,), None: 1.  Returns what `element_loads` returns, in its layout."""
    coords, e2v, coef, ep = _element_arrays(coords, elem_to_vertex, coef, elem_ptr)
    vdim = int(vdim)
    NV, dim, NE, nde, doubles = _mass_sizes(coords, e2v, ep, vdim, False)
    info = (C.c_longlong * 8)()
    elvec = out if out is not None else _new_doubles(doubles, device)
    _mass_call(lambda: load().saamge_amd_element_loads_points(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(vdim), _ptr(coef),
        _ptr(_doubles(fq)), C.c_void_p(stream), _ptr(elvec), info), info)
    return elvec.reshape(NE, nde * vdim) if ep is None else elvec


def element_errors(coords, elem_to_vertex, u, exq=None, exgradq=None, vdim=1, elem_ptr=None, device=False, out=None, stream=0):
    """saamge_amd_element_errors: (NE, 2) -- per element the squared L2 error of the nodal u against exq (NQ, vdim) at the points
    of `element_points`, and the squared error of its gradient against exgradq (NQ, vdim, dim); None: that column is 0.0.  The
    caller sums a column and takes the root."""
    coords, e2v, _, ep = _element_arrays(coords, elem_to_vertex, None, elem_ptr)
    vdim = int(vdim)
    NV, dim, NE, nde, _ = _mass_sizes(coords, e2v, ep, vdim, False)
    info = (C.c_longlong * 8)()
    err = out if out is not None else _new_doubles(NE * 2, device)
    _mass_call(lambda: load().saamge_amd_element_errors(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(vdim), _ptr(_doubles(u)),
        _ptr(_doubles(exq)), _ptr(_doubles(exgradq)), C.c_void_p(stream), _ptr(err), info), info)
    return err.reshape(NE, 2)


# ---- coefficients at the points (elmat_model.element_matrices_points / element_mass_points) ----
def element_matrices_points(coords, elem_to_vertex, kind, coefq, elem_ptr=None, device=False, dofs=False, out=None, stream=0):
    """saamge_amd_element_matrices_points: `element_matrices` with a coefficient row per POINT of `element_points` in the place
    of one per element -- coefq (NQ,) or (NQ, ncoef), row qp_ptr[e] + q for point q of element e (what `element_eval` returns is
    indexed so).  Both forms are integrated with the type's MASS rule here; everything else -- kinds, ncoef, the layout, device=,
    dofs=, out=, stream=, the refusals -- as `element_matrices`.  A curved 6-node triangle / 10-node tetrahedron can be refused
    here at a point `element_matrices` does not have."""
    return _element_matrices(coords, elem_to_vertex, kind, coefq, elem_ptr, device, dofs, out, stream,
                             "saamge_amd_element_matrices_points")


def element_matrices_points_info(coords, elem_to_vertex, kind, coefq, elem_ptr=None, stream=0):
    """The sizes-only call (elmat_out = NULL) of `element_matrices_points`: info as `element_matrices_info`."""
    coords, e2v, coefq, ep = _element_arrays(coords, elem_to_vertex, coefq, elem_ptr)
    return _element_matrices_call(coords, e2v, kind, coefq, ep, stream, None, None, None, "saamge_amd_element_matrices_points")


def element_mass_points(coords, elem_to_vertex, coefq, vdim=1, elem_ptr=None, add_to=None, device=False, out=None, stream=0,
                        sizes_only=False):
    """saamge_amd_element_mass_points: `element_mass` with the coefficient coefq (NQ,) given at the points of `element_points`;
    vdim, add_to (added IN PLACE: K(u) + sigma(u) M), device=, out=, stream=, sizes_only and the refusals as there."""
    coords, e2v, coefq, ep = _element_arrays(coords, elem_to_vertex, coefq, elem_ptr)
    vdim = int(vdim)
    NV, dim, NE, nde, doubles = _mass_sizes(coords, e2v, ep, vdim, True)
    info = (C.c_longlong * 8)()
    if sizes_only:
        elmat = None
    elif add_to is not None:
        elmat = add_to
    else:
        elmat = out if out is not None else _new_doubles(doubles, device)
    got = _mass_call(lambda: load().saamge_amd_element_mass_points(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(vdim), _ptr(coefq),
        C.c_void_p(stream), C.c_int(1 if add_to is not None else 0), _ptr(elmat), info), info)
    if sizes_only:
        return got
    if ep is None and add_to is None:
        elmat = elmat.reshape(NE, nde * vdim, nde * vdim)
    return elmat


def _face_arrays(face_elem, face_local, coef):
    def arr(a, dt):
        return a if a is None or hasattr(a, "data_ptr") else np.ascontiguousarray(a, dtype=dt).ravel()
    fe, fl, coef = arr(face_elem, np.int32), arr(face_local, np.int32), arr(coef, np.float64)
    return fe, fl, coef, 0 if fe is None else int(fe.shape[0])


def _in_place_target(add_to, doubles, device):
    """The target of a boundary call, written in place: add_to -- a device tensor, or a writeable C-contiguous float64 numpy
    array -- or, for None, new zeros (on the GPU with device=True)"""
    if add_to is None:
        return _new_doubles(doubles, device)
    if not hasattr(add_to, "data_ptr") and not (isinstance(add_to, np.ndarray) and add_to.dtype == np.float64 and
                                                  add_to.flags["C_CONTIGUOUS"] and add_to.flags["WRITEABLE"]):
        raise ValueError("add_to: a device tensor or a writeable C-contiguous float64 array is needed (it is written in place)")
    return add_to


def boundary_mass(coords, elem_to_vertex, face_elem, face_local, coef, vdim=1, elem_ptr=None, add_to=None, device=False,
                  stream=0, sizes_only=False):
    """saamge_amd_boundary_mass: the face mass (c u, v) of the listed faces -- face f is the local face face_local[f]
    (elmat_model.FACE_NODES) of element face_elem[f], c = coef (NF,) -- added IN PLACE to add_to, an array / tensor in the layout
    of `element_matrices` / `element_mass` with the same vdim, which is returned: the Robin term.  add_to None: the face terms
    alone, in new zero matrices (device=True: a torch tensor on the GPU).  Inputs numpy arrays or device tensors, each on its own.  sizes_only: info (8 integers: faces by type [0..4], additions, -1, elements touched), nothing
    written.  A refusal raises RuntimeError with `.info` (info[6]: the first refused face).  Faces by type: 2-node segments,
    3-node segments, triangles (of 3 and of 6 nodes), 4-node and 9-node quadrilaterals (elmat_model.face_info_index)."""
    coords, e2v, _, ep = _element_arrays(coords, elem_to_vertex, None, elem_ptr)
    fe, fl, coef, NF = _face_arrays(face_elem, face_local, coef)
    vdim = int(vdim)
    NV, dim, NE, nde, doubles = _mass_sizes(coords, e2v, ep, vdim, True)
    if not sizes_only:
        add_to = _in_place_target(add_to, doubles, device)
    info = (C.c_longlong * 8)()
    got = _mass_call(lambda: load().saamge_amd_boundary_mass(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(NF), _ptr(fe), _ptr(fl),
        C.c_int(vdim), _ptr(coef), C.c_void_p(stream), _ptr(None if sizes_only else add_to), info), info)
    return got if sizes_only else add_to


def boundary_loads(coords, elem_to_vertex, face_elem, face_local, g, vdim=1, coef=None, elem_ptr=None, add_to=None, device=False,
                   stream=0, sizes_only=False):
    """saamge_amd_boundary_loads: the face loads (c g, v) of the data g given at the nodes, (NV, vdim) or (NV,), on the listed
    faces, coef (NF,) or None: 1 -- added IN PLACE to add_to, an array / tensor in the layout of `element_loads`, which is
    returned: the Neumann term.  Data that jumps across an edge takes one call per side; the calls accumulate.  Otherwise as
    `boundary_mass`."""
    coords, e2v, _, ep = _element_arrays(coords, elem_to_vertex, None, elem_ptr)
    fe, fl, coef, NF = _face_arrays(face_elem, face_local, coef)
    if g is not None and not hasattr(g, "data_ptr"):
        g = np.ascontiguousarray(g, dtype=np.float64)
    vdim = int(vdim)
    NV, dim, NE, nde, doubles = _mass_sizes(coords, e2v, ep, vdim, False)
    if not sizes_only:
        add_to = _in_place_target(add_to, doubles, device)
    info = (C.c_longlong * 8)()
    got = _mass_call(lambda: load().saamge_amd_boundary_loads(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(NF), _ptr(fe), _ptr(fl),
        C.c_int(vdim), _ptr(coef), _ptr(g), C.c_void_p(stream), _ptr(None if sizes_only else add_to), info), info)
    return got if sizes_only else add_to


# ---- boundary data at the face points (elmat_model.boundary_points / _eval / _mass_points / _loads_points) ----
def _num_face_points(NV, dim, coords, NE, nde, ep, e2v, NF, fe, fl, stream, brought):
    """NFQ from the checks-only call (saamge_amd_boundary_points without outputs: info[5]), which refuses what the writing call
    would refuse; brought: (name, array, doubles per point) of the outputs the caller brings, which must hold NFQ rows -- the
    library writes through the pointers it is given"""
    info = (C.c_longlong * 8)()
    NFQ = _mass_call(lambda: load().saamge_amd_boundary_points(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(NF), _ptr(fe), _ptr(fl),
        C.c_void_p(stream), None, None, None, None, info), info)[5]
    for name, a, width in brought:
        if a is not None and int(a.numel() if hasattr(a, "data_ptr") else a.size) != NFQ * width:
            raise ValueError("out[%r]: %d doubles are needed" % (name, NFQ * width))
    return NFQ


def boundary_points(coords, elem_to_vertex, face_elem, face_local, elem_ptr=None, device=False,
                    want=("fp_ptr", "xq", "wmeas", "normal"), out=None, stream=0, sizes_only=False):
    """saamge_amd_boundary_points: (fp_ptr (NF + 1,) int64, xq (NFQ, dim), wmeas (NFQ,), normal (NFQ, dim)) -- the points of the
    face rule of every listed face (point q of face f OF THE LIST: index fp_ptr[f] + q), their physical coordinates, weight *
    measure there and the unit normal that points out of the owning element.  want: which of the four are asked for, the others
    are passed as NULL and come back None; out: a dict of arrays / tensors to write into, by the same names.  device=True: torch
    tensors on the GPU.  sizes_only: info (8 integers: faces by type [0..4], [5] = NFQ, -1, elements touched).  A refusal raises
    RuntimeError with `.info` (info[6]: the first refused face) and writes nothing."""
    coords, e2v, _, ep = _element_arrays(coords, elem_to_vertex, None, elem_ptr)
    fe, fl, _, NF = _face_arrays(face_elem, face_local, None)
    NV, dim, NE, nde, _ = _mass_sizes(coords, e2v, ep, 1, False)
    out = dict(out or {})
    want = () if sizes_only else tuple(want)
    NFQ = _num_face_points(NV, dim, coords, NE, nde, ep, e2v, NF, fe, fl, stream,
                           [(k, out.get(k), w) for k, w in (("xq", dim), ("wmeas", 1), ("normal", dim))]) if want else 0
    fp = out.get("fp_ptr")
    if fp is None and "fp_ptr" in want:
        fp = _new_ints(NF + 1, np.int64, "int64", device)
    xq = _new_or(out.get("xq"), NFQ * dim, device, "xq" in want)
    wmeas = _new_or(out.get("wmeas"), NFQ, device, "wmeas" in want)
    normal = _new_or(out.get("normal"), NFQ * dim, device, "normal" in want)
    info = (C.c_longlong * 8)()
    got = _mass_call(lambda: load().saamge_amd_boundary_points(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(NF), _ptr(fe), _ptr(fl),
        C.c_void_p(stream), _ptr(fp), _ptr(xq), _ptr(wmeas), _ptr(normal), info), info)
    if sizes_only:
        return got
    return fp, None if xq is None else xq.reshape(NFQ, dim), wmeas, None if normal is None else normal.reshape(NFQ, dim)


def boundary_eval(coords, elem_to_vertex, face_elem, face_local, u, vdim=1, elem_ptr=None, device=False, want=("uq", "gradq"),
                  out=None, stream=0):
    """saamge_amd_boundary_eval: (uq (NFQ, vdim), gradq (NFQ, vdim, dim)) of the nodal field u, (NV, vdim) or (NV,), at the points
    of `boundary_points`: the trace through the face's shape functions and the WHOLE gradient of the owning element's field
    (gradq[q, i, j]: component i along x_j).  want / out / device / stream as there; want=(): the checks only."""
    coords, e2v, _, ep = _element_arrays(coords, elem_to_vertex, None, elem_ptr)
    fe, fl, _, NF = _face_arrays(face_elem, face_local, None)
    vdim = int(vdim)
    NV, dim, NE, nde, _ = _mass_sizes(coords, e2v, ep, vdim, False)
    out = dict(out or {})
    NFQ = _num_face_points(NV, dim, coords, NE, nde, ep, e2v, NF, fe, fl, stream,
                           [(k, out.get(k), w) for k, w in (("uq", vdim), ("gradq", vdim * dim))]) if want else 0
    uq = _new_or(out.get("uq"), NFQ * vdim, device, "uq" in want)
    gq = _new_or(out.get("gradq"), NFQ * vdim * dim, device, "gradq" in want)
    info = (C.c_longlong * 8)()
    _mass_call(lambda: load().saamge_amd_boundary_eval(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(NF), _ptr(fe), _ptr(fl),
        C.c_int(vdim), _ptr(_doubles(u)), C.c_void_p(stream), _ptr(uq), _ptr(gq), info), info)
    return None if uq is None else uq.reshape(NFQ, vdim), None if gq is None else gq.reshape(NFQ, vdim, dim)


def boundary_mass_points(coords, elem_to_vertex, face_elem, face_local, coefq, vdim=1, elem_ptr=None, add_to=None, device=False,
                         stream=0, sizes_only=False):
    """saamge_amd_boundary_mass_points: `boundary_mass` with the coefficient coefq (NFQ,) given at the points of
    `boundary_points` -- alpha(u_q) formed from the output of `boundary_eval` goes in as it is.  Everything else as there; a
    refusal writes nothing."""
    coords, e2v, _, ep = _element_arrays(coords, elem_to_vertex, None, elem_ptr)
    fe, fl, coefq, NF = _face_arrays(face_elem, face_local, coefq)
    vdim = int(vdim)
    NV, dim, NE, nde, doubles = _mass_sizes(coords, e2v, ep, vdim, True)
    if not sizes_only:
        add_to = _in_place_target(add_to, doubles, device)
    info = (C.c_longlong * 8)()
    got = _mass_call(lambda: load().saamge_amd_boundary_mass_points(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(NF), _ptr(fe), _ptr(fl),
        C.c_int(vdim), _ptr(coefq), C.c_void_p(stream), _ptr(None if sizes_only else add_to), info), info)
    return got if sizes_only else add_to


def boundary_loads_points(coords, elem_to_vertex, face_elem, face_local, gq, vdim=1, coef=None, elem_ptr=None, add_to=None,
                          device=False, stream=0, sizes_only=False):
    """saamge_amd_boundary_loads_points: `boundary_loads` of data given AT THE POINTS of `boundary_points`, gq (NFQ, vdim) or
    (NFQ,); coef (NF,) or None: 1.  A flux g = k grad u . n formed from `normal` does not jump across the edges of a box, so all
    sides go in one call.  Everything else as `boundary_loads`; a refusal writes nothing."""
    coords, e2v, _, ep = _element_arrays(coords, elem_to_vertex, None, elem_ptr)
    fe, fl, coef, NF = _face_arrays(face_elem, face_local, coef)
    vdim = int(vdim)
    NV, dim, NE, nde, doubles = _mass_sizes(coords, e2v, ep, vdim, False)
    if not sizes_only:
        add_to = _in_place_target(add_to, doubles, device)
    info = (C.c_longlong * 8)()
    got = _mass_call(lambda: load().saamge_amd_boundary_loads_points(
        C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(NF), _ptr(fe), _ptr(fl),
        C.c_int(vdim), _ptr(coef), _ptr(_doubles(gq)), C.c_void_p(stream), _ptr(None if sizes_only else add_to), info), info)
    return got if sizes_only else add_to


def _mesh_sizes(NV, e2v, ep):
    """(NV, NE, nde) of a mesh given as (NE, nodes) lists, or flat lists with elem_ptr"""
    if ep is None:
        return int(NV), int(e2v.shape[0]), int(e2v.shape[1])
    return int(NV), len(ep) - 1, 0


def _new_ints(n, np_dt, torch_dt, device):
    if device:
        import torch
        return torch.zeros(int(n), dtype=getattr(torch, torch_dt), device="cuda")
    return np.zeros(max(int(n), 1), np_dt)[:int(n)]


class _MeshHandle(_Handle):
    """A handle whose device arrays a table describes.  _FIELDS: the arguments of the C calls _ARRAYS (addresses) and _GET (copies)
    after the handle, in their order -- (name, numpy dtype, shape(self)) an array, shape None: the handle has no such array;
    (name, ctypes type) a count."""
    _ARRAYS = _GET = None
    _FIELDS = ()

    def arrays(self):
        """dict of the raw device addresses of the handle's arrays (0: the handle has no such array) and of its counts, by the
        names of the class's docstring; valid until free().  `pointer(name)` wraps one for the other entry points."""
        slots = [C.c_void_p() if len(f) == 3 else f[1](0) for f in self._FIELDS]
        _check(getattr(load(), self._ARRAYS)(self.h, *[C.byref(v) for v in slots]))
        return {f[0]: int(v.value or 0) for f, v in zip(self._FIELDS, slots)}

    def pointer(self, name, shape=None):
        """the handle's device array `name` as an object the wrappers take in place of a device tensor (valid until free()), in
        the shape `get()` gives it unless `shape` says otherwise (a node list as (NE, nodes) on a mesh of one type)"""
        _, dt, own = next(f for f in self._FIELDS if f[0] == name and len(f) == 3)
        own = own(self)
        d = _DevicePointer(self.arrays()[name], dt)
        assert own is not None, "the handle has no " + name
        d.shape = own
        if shape is not None:
            d.shape = tuple(shape)
            assert int(np.prod(d.shape)) == int(np.prod(own))
        return d

    def get(self, device=False):
        """the handle's arrays in the order of the class's docstring (None: the handle has no such array): numpy arrays, or torch
        tensors on the GPU with device=True"""
        out = []
        for f in self._FIELDS:
            shape = f[2](self) if len(f) == 3 else None
            if shape is None:
                out.append(None)
            elif f[1] is np.float64:
                out.append(_new_doubles(int(np.prod(shape)), device))
            else:
                out.append(_new_ints(int(np.prod(shape)), f[1], np.dtype(f[1]).name, device))
        _check(getattr(load(), self._GET)(self.h, *[_ptr(a) for a in out]))
        return tuple(a if a is None else a.reshape(f[2](self)) for f, a in zip(self._FIELDS, out) if len(f) == 3)


def _lift_arguments(coords, elem_to_vertex, elem_ptr, NV, dim):
    """(coords, e2v, ep, NV, dim, NE, nde): the head of MeshLift and MeshRefine -- the sizes from coords, or NV and dim given"""
    coords, e2v, _, ep = _element_arrays(coords, elem_to_vertex, None, elem_ptr)
    if coords is not None:
        NV, dim = int(coords.shape[0]), int(coords.shape[1])
    elif NV is None or dim is None:
        raise ValueError("without coords, NV and dim are needed")
    NV, NE, nde = _mesh_sizes(NV, e2v, ep)
    return coords, e2v, ep, NV, int(dim), NE, nde


class FaceTable(_MeshHandle):
    """saamge_amd_face_table_build: which element lies across each local face of a mesh, owned by the library until free()
    (or the end of a `with` block).  saamge_amd/mesh_model.py defines every integer.  elem_to_vertex ((NE, nodes), or flat with
    elem_ptr) and elem_ptr: numpy arrays or device tensors, each on its own.  `.info`: the 8 integers of the call; a refusal
    raises RuntimeError with `.info` (info[6]: the lowest element with a non-manifold face).
    Arrays: slot_ptr int64, nbr_elem, nbr_local, bdr_elem, bdr_local int32, xadj int64, adj int32; counts: NB, nnz."""
    _FREE, _ARRAYS, _GET = "saamge_amd_face_table_free", "saamge_amd_face_table_arrays", "saamge_amd_face_table_get"
    _FIELDS = (("slot_ptr", np.int64, lambda t: (t.NE + 1,)), ("nbr_elem", np.int32, lambda t: (t.slots,)),
               ("nbr_local", np.int32, lambda t: (t.slots,)), ("NB", C.c_longlong), ("bdr_elem", np.int32, lambda t: (t.NB,)),
               ("bdr_local", np.int32, lambda t: (t.NB,)), ("xadj", np.int64, lambda t: (t.NE + 1,)),
               ("adj", np.int32, lambda t: (t.nnz,)), ("nnz", C.c_longlong))

    def __init__(self, NV, dim, elem_to_vertex, elem_ptr=None, stream=0):
        _, e2v, _, ep = _element_arrays(None, elem_to_vertex, None, elem_ptr)
        NV, NE, nde = _mesh_sizes(NV, e2v, ep)
        h = C.c_void_p()
        info = (C.c_longlong * 8)()
        self.info = _mass_call(lambda: load().saamge_amd_face_table_build(
            C.c_int(NV), C.c_int(int(dim)), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_void_p(stream), C.byref(h), info), info)
        self.h = h
        self.NE = NE
        counts = self.arrays()
        self.NB, self.nnz, self.slots = counts["NB"], counts["nnz"], self.info[0]


def face_nodes(NV, dim, elem_to_vertex, face_elem, face_local, elem_ptr=None, device=False, stream=0):
    """saamge_amd_face_nodes: (face_ptr int32 (NF + 1), nodes int32) -- the global node ids of each listed face in the face's own
    node order (elmat_model.FACE_NODES), midside nodes included.  Inputs numpy arrays or device tensors, each on its own;
    device=True: torch tensors on the GPU.  Choose faces by position with your own arithmetic on coords[nodes]."""
    _, e2v, _, ep = _element_arrays(None, elem_to_vertex, None, elem_ptr)
    fe, fl, _, NF = _face_arrays(face_elem, face_local, None)
    NV, NE, nde = _mesh_sizes(NV, e2v, ep)
    count = C.c_longlong(0)

    def call(fptr, nodes):
        _check(load().saamge_amd_face_nodes(C.c_int(NV), C.c_int(int(dim)), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(NF),
                                            _ptr(fe), _ptr(fl), C.c_void_p(stream), _ptr(fptr), _ptr(nodes), C.byref(count)))
    call(None, None)
    fptr = _new_ints(NF + 1, np.int32, "int32", device)
    nodes = _new_ints(count.value, np.int32, "int32", device)
    if NF:
        call(fptr, nodes)
    return fptr, nodes


def face_dofs(NV, dim, elem_to_vertex, face_elem, face_local, bdr_dofs, vdim=1, comp_mask=None, flag=0x02, elem_ptr=None,
              stream=0):
    """saamge_amd_face_dofs: bdr_dofs[vdim * a + i] |= flag IN PLACE for every node a of every listed face and every component i
    with bit i of comp_mask set (None: all vdim components); flag: SAAMGE_AMD_ON_ESS_DOMAIN_BORDER by default.  bdr_dofs: a device
    tensor or a writeable C-contiguous int8 numpy array of vdim * NV entries -- what `Operator` and `Hierarchy` take as bdr.
    Returns info = [faces, distinct nodes touched, bytes whose value changed, -1]; a refusal raises RuntimeError with `.info`
    (info[3]: the first refused face)."""
    _, e2v, _, ep = _element_arrays(None, elem_to_vertex, None, elem_ptr)
    fe, fl, _, NF = _face_arrays(face_elem, face_local, None)
    NV, NE, nde = _mesh_sizes(NV, e2v, ep)
    vdim = int(vdim)
    if comp_mask is None:
        comp_mask = (1 << vdim) - 1
    if bdr_dofs is not None and not hasattr(bdr_dofs, "data_ptr") and not (
            isinstance(bdr_dofs, np.ndarray) and bdr_dofs.dtype == np.int8 and bdr_dofs.flags["C_CONTIGUOUS"] and
            bdr_dofs.flags["WRITEABLE"]):
        raise ValueError("bdr_dofs: a device tensor or a writeable C-contiguous int8 array is needed (it is written in place)")
    if bdr_dofs is not None and int(np.prod(tuple(bdr_dofs.shape))) != vdim * NV and vdim in (1, int(dim)):
        raise ValueError("bdr_dofs: vdim * NV entries are needed")
    info = (C.c_longlong * 4)()
    return _mass_call(lambda: load().saamge_amd_face_dofs(
        C.c_int(NV), C.c_int(int(dim)), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(NF), _ptr(fe), _ptr(fl), C.c_int(vdim),
        C.c_uint(int(comp_mask) & 0xffffffff), C.c_int(int(flag)), C.c_void_p(stream), _ptr(bdr_dofs), info), info)


class MeshLift(_MeshHandle):
    """saamge_amd_mesh_lift_order2: an order-1 mesh lifted to order 2 on the same elements -- all node coordinates, the element
    -> node lists in the node orders `element_matrices` takes (6-node triangle, 9-node quadrilateral, 10-node tetrahedron,
    27-node hexahedron), and the edge table found on the way -- owned by the library until free() (or the end of a `with`
    block).  saamge_amd/mesh_lift_model.py defines every integer and every coordinate bit.  coords ((NV, dim), or None: no
    coordinates, then NV and dim are needed), elem_to_vertex ((NE, nodes), or flat with elem_ptr) and elem_ptr: numpy arrays or
    device tensors, each on its own.  faces: a `FaceTable` of the same mesh (used where the mesh has a hexahedron), None: built
    inside.  `.info`: the 8 integers of the call (NV2, edges, face nodes, centre nodes, entries of elem_to_node, the most edges
    of a vertex, -1, unlisted vertices); a refusal raises RuntimeError with `.info` (info[6]: the lowest refused element).
    Arrays: coords2 float64 (NV2, dim) -- none without coordinates --, elem_ptr2 int32, elem_to_node int32 (flat: element e is
    elem_to_node[elem_ptr2[e]:elem_ptr2[e + 1]], on a mesh of one type too), edge_ptr int64, edge_hi int32, face_slot int64;
    count: NV2."""
    NAMES = ("coords2", "elem_ptr2", "elem_to_node", "edge_ptr", "edge_hi", "face_slot")
    _FREE, _ARRAYS, _GET = "saamge_amd_mesh_lift_free", "saamge_amd_mesh_lift_arrays", "saamge_amd_mesh_lift_get"
    _FIELDS = (("NV2", C.c_int), ("coords2", np.float64, lambda m: (m.NV2, m.dim) if m.has_coords else None),
               ("elem_ptr2", np.int32, lambda m: (m.NE + 1,)), ("elem_to_node", np.int32, lambda m: (m.entries,)),
               ("edge_ptr", np.int64, lambda m: (m.NV + 1,)), ("edge_hi", np.int32, lambda m: (m.NEd,)),
               ("face_slot", np.int64, lambda m: (m.NFq,)))

    def __init__(self, coords, elem_to_vertex, elem_ptr=None, faces=None, NV=None, dim=None, stream=0):
        coords, e2v, ep, NV, dim, NE, nde = _lift_arguments(coords, elem_to_vertex, elem_ptr, NV, dim)
        h = C.c_void_p()
        info = (C.c_longlong * 8)()
        self.info = _mass_call(lambda: load().saamge_amd_mesh_lift_order2(
            C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v),
            faces.h if faces is not None else None, C.c_void_p(stream), C.byref(h), info), info)
        self.h = h
        self.NV, self.NE, self.dim, self.has_coords = NV, NE, dim, coords is not None
        self.NV2, self.NEd, self.NFq, self.NC, self.entries = self.info[:5]


class MeshRefine(_MeshHandle):
    """saamge_amd_mesh_refine: an order-1 mesh refined uniformly `levels` times on the device -- every triangle and quadrilateral
    into 4, every tetrahedron and hexahedron into 8 elements of its own type --, owned by the library until free() (or the end of
    a `with` block).  saamge_amd/mesh_refine_model.py defines every integer and every coordinate bit.  Child k of element e is
    element nc * e + k of the next level (nc = 4 | 8): the nested partitions are arange(NE) >> (2 s | 3 s).  coords ((NV, dim), or
    None: no coordinates, then NV and dim are needed), elem_to_vertex ((NE, nodes), or flat with elem_ptr) and elem_ptr: numpy
    arrays or device tensors, each on its own.  want_interp: the vertex -> vertex interpolations P_0 .. P_{levels-1} are kept
    (`interp(level)`).  `.info`: the 8 integers of the call (NV, NE and entries of elem_to_vertex of the result, levels, total nnz
    of the kept P, the most edges of a vertex, -1, unlisted vertices); a refusal raises RuntimeError with `.info` (info[6]: the
    lowest refused element).
    Arrays: coords float64 (NV, dim) -- none without coordinates --, elem_ptr int32, elem_to_vertex int32 (flat: element c is
    elem_to_vertex[elem_ptr[c]:elem_ptr[c + 1]], on a mesh of one type too); counts: NV, NE."""
    NAMES = ("coords", "elem_ptr", "elem_to_vertex")
    _FREE, _ARRAYS, _GET = "saamge_amd_mesh_refine_free", "saamge_amd_mesh_refine_arrays", "saamge_amd_mesh_refine_get"
    _FIELDS = (("NV", C.c_int), ("NE", C.c_int), ("coords", np.float64, lambda m: (m.NV, m.dim) if m.has_coords else None),
               ("elem_ptr", np.int32, lambda m: (m.NE + 1,)), ("elem_to_vertex", np.int32, lambda m: (m.entries,)))

    def __init__(self, coords, elem_to_vertex, elem_ptr=None, levels=1, want_interp=False, NV=None, dim=None, stream=0):
        coords, e2v, ep, NV, dim, NE, nde = _lift_arguments(coords, elem_to_vertex, elem_ptr, NV, dim)
        h = C.c_void_p()
        info = (C.c_longlong * 8)()
        self.info = _mass_call(lambda: load().saamge_amd_mesh_refine(
            C.c_int(NV), C.c_int(dim), _ptr(coords), C.c_int(NE), C.c_int(nde), _ptr(ep), _ptr(e2v), C.c_int(int(levels)),
            C.c_int(int(bool(want_interp))), C.c_void_p(stream), C.byref(h), info), info)
        self.h = h
        self.dim, self.has_coords, self.want_interp = dim, coords is not None, bool(want_interp)
        self.NV, self.NE, self.entries, self.levels = self.info[:4]

    def level_info(self, level):
        """[NV, NE, entries of the vertex list, NEd, NFq, centres, the most edges of a vertex, nnz of P_level] of level `level`
        in [0, levels]; the last level was not lifted: -1 from NEd on"""
        info = (C.c_longlong * 8)()
        _check(load().saamge_amd_mesh_refine_level_info(self.h, C.c_int(int(level)), info))
        return [int(v) for v in info]

    def interp_arrays(self, level):
        """P_level as a dict of raw device addresses (rowptr, col, val) and nrows, ncols, nnz; valid until free()"""
        p = [C.c_void_p() for _ in range(3)]
        nrows, ncols, nnz = C.c_int(0), C.c_int(0), C.c_longlong(0)
        _check(load().saamge_amd_mesh_refine_interp_arrays(self.h, C.c_int(int(level)), C.byref(nrows), C.byref(ncols), C.byref(nnz),
                                                           *[C.byref(v) for v in p]))
        out = {k: int(v.value or 0) for k, v in zip(("rowptr", "col", "val"), p)}
        out.update(nrows=int(nrows.value), ncols=int(ncols.value), nnz=int(nnz.value))
        return out

    def interp(self, level, device=False):
        """P_level as (nrows, ncols, rowptr int32, col int32, val float64): numpy arrays, or torch tensors on the GPU with
        device=True"""
        nrows, ncols, nnz = C.c_int(0), C.c_int(0), C.c_longlong(0)
        _check(load().saamge_amd_mesh_refine_interp_get(self.h, C.c_int(int(level)), C.byref(nrows), C.byref(ncols), C.byref(nnz),
                                                        None, None, None))
        out = [_new_ints(nrows.value + 1, np.int32, "int32", device), _new_ints(nnz.value, np.int32, "int32", device),
               _new_doubles(nnz.value, device)]
        _check(load().saamge_amd_mesh_refine_interp_get(self.h, C.c_int(int(level)), None, None, None, *[_ptr(a) for a in out]))
        return (int(nrows.value), int(ncols.value)) + tuple(out)


def get_options():
    o = Options()
    load().saamge_amd_get_options(C.byref(o))
    return o


def set_options(**kw):
    """The process-wide DEFAULT options of the library (saamge_amd_options); returns the previous values.  default_params()
    copies the current default into params.options, and params.options is what a hierarchy uses for its whole life: a later
    set_options does not reach hierarchies that already exist.  The entry points without a hierarchy (spmv,
    lower_eigens_batched) use the default directly."""
    old = get_options()
    new = Options.from_buffer_copy(old)
    for k, v in kw.items():
        assert hasattr(new, k), k
        setattr(new, k, int(v))
    load().saamge_amd_set_options(C.byref(new))
    return old


def reset_options():
    o = Options()
    load().saamge_amd_options_default(C.byref(o))
    load().saamge_amd_set_options(C.byref(o))


class PartitionOptions(C.Structure):      # saamge_amd_partition_options
    _fields_ = [("min_shared", C.c_int), ("lloyd_iters", C.c_int), ("max_size", C.c_int), ("min_size", C.c_int),
                ("seed", C.c_uint), ("seeding", C.c_int)]


class PartitionOptionsV2(C.Structure):    # saamge_amd_partition_options_v2: the same fields, then `growth`
    _fields_ = PartitionOptions._fields_ + [("growth", C.c_int)]


def partition_options(**kw):
    """The library's defaults with the given fields replaced: a PartitionOptions, or a PartitionOptionsV2 when `growth` is
    among them."""
    if "growth" in kw:
        o = PartitionOptionsV2()
        load().saamge_amd_partition_options_v2_default(C.byref(o))
    else:
        o = PartitionOptions()
        load().saamge_amd_partition_options_default(C.byref(o))
    for k, v in kw.items():
        if k not in dict(o._fields_):
            raise KeyError(k)
        setattr(o, k, int(v))
    return o


def _v2(o, name):
    """The entry point that takes the struct o: `name` or `name`_v2."""
    return getattr(load(), name + "_v2" if isinstance(o, PartitionOptionsV2) else name)


def partition_graph(n, xadj, adj, elems_per_agg, part=None, stream=0, **opts):
    """saamge_amd_partition_graph.  xadj (int64) / adj (int32): numpy arrays or device tensors.  part: None (a numpy array
    is returned) or a device tensor of n int32 that receives the partition.  Keywords are the fields of PartitionOptions
    (seeding=1: spaced seeds) or, with `growth` among them (1: balanced growth), of PartitionOptionsV2, which goes to
    saamge_amd_partition_graph_v2.  Returns (part, nparts)."""
    o = partition_options(**opts)
    if part is None:
        part = np.zeros(max(int(n), 1), np.int32)[:int(n)]
    npt = C.c_int(0)
    _check(_v2(o, "saamge_amd_partition_graph")(C.c_int(int(n)), _ptr(xadj), _ptr(adj), C.c_int(int(elems_per_agg)), C.byref(o),
                                                C.c_void_p(stream), _ptr(part), C.byref(npt)))
    return part, int(npt.value)


def partition_seeding_info():
    """saamge_amd_partition_seeding_info: what the spaced seeding did in this thread's last partition of one graph."""
    info = (C.c_longlong * 4)()
    fn = load().saamge_amd_partition_seeding_info
    fn.restype = None
    fn(info)
    return dict(radius=int(info[0]), rounds=int(info[1]), seeds_first=int(info[2]), seeds=int(info[3]))


def partition_growth_info():
    """saamge_amd_partition_growth_info: what the balanced growth did in this thread's last partition of one graph."""
    info = (C.c_longlong * 4)()
    fn = load().saamge_amd_partition_growth_info
    fn.restype = None
    fn(info)
    return dict(rounds=int(info[0]), quota_nodes=int(info[1]), open_parts=int(info[2]), released_nodes=int(info[3]))


def partition_refine(n, xadj, adj, nparts, part, rounds, max_size=0, min_size=0, seed=0, renumber=False, stream=0):
    """saamge_amd_partition_refine: the boundary refinement pass on any partition, in place.  part: a numpy int32 array or a
    device tensor of n int32.  Returns (part, info) with info = dict(rounds, moved, gain, converged)."""
    info = (C.c_longlong * 4)()
    _check(load().saamge_amd_partition_refine(C.c_int(int(n)), _ptr(xadj), _ptr(adj), C.c_int(int(nparts)), _ptr(part),
                                              C.c_int(int(rounds)), C.c_int(int(max_size)), C.c_int(int(min_size)),
                                              C.c_uint(int(seed)), C.c_int(int(renumber)), C.c_void_p(stream), info))
    return part, dict(rounds=int(info[0]), moved=int(info[1]), gain=int(info[2]), converged=int(info[3]))


def partition_refine_info():
    """saamge_amd_partition_refine_info: what this thread's last refinement pass did."""
    info = (C.c_longlong * 4)()
    fn = load().saamge_amd_partition_refine_info
    fn.restype = None
    fn(info)
    return dict(rounds=int(info[0]), moved=int(info[1]), gain=int(info[2]), converged=int(info[3]))


class Partitioning(_Handle):
    """saamge_amd_partition_mesh: the partitions of every coarsening, owned by the library until close().  Keywords beyond
    the named ones are the fields of PartitionOptions (seeding=1: spaced seeds) or, with `growth` among them (1: balanced
    growth), of PartitionOptionsV2 (saamge_amd_partition_mesh_v2).  refine_rounds: one count per coarsening, the boundary
    refinement of saamge_amd_partition_mesh_refined (None: the entry points without it)."""
    _FREE = "saamge_amd_partitioning_free"

    def __init__(self, elem_to_dof, ND, elems_per_agg, elem_ptr=None, nde=0, NE=None, stream=0, refine_rounds=None, **opts):
        if refine_rounds is not None:
            if len(refine_rounds) != len(elems_per_agg):
                raise ValueError("refine_rounds: one entry per coarsening")
            opts.setdefault("growth", 0)      # the refined entry point takes the v2 options
        o = partition_options(**opts)
        if NE is None:
            NE = len(elem_ptr) - 1 if elem_ptr is not None else int(elem_to_dof.shape[0])
        if elem_ptr is None and not nde:
            nde = int(elem_to_dof.shape[1])
        epa = (C.c_int * len(elems_per_agg))(*[int(x) for x in elems_per_agg])
        h = C.c_void_p()
        if refine_rounds is not None:
            rr = (C.c_int * len(refine_rounds))(*[int(x) for x in refine_rounds])
            _check(load().saamge_amd_partition_mesh_refined(C.c_int(int(NE)), C.c_int(int(nde)), _ptr(elem_ptr), _ptr(elem_to_dof),
                                                            C.c_int(int(ND)), C.c_int(len(elems_per_agg)), epa, C.byref(o), rr,
                                                            C.c_void_p(stream), C.byref(h)))
        else:
            _check(_v2(o, "saamge_amd_partition_mesh")(C.c_int(int(NE)), C.c_int(int(nde)), _ptr(elem_ptr), _ptr(elem_to_dof),
                                                       C.c_int(int(ND)), C.c_int(len(elems_per_agg)), epa, C.byref(o),
                                                       C.c_void_p(stream), C.byref(h)))
        self.h = h
        self.num_coarsenings = len(elems_per_agg)
        self.nparts, self.n_elem = [], []
        for k in range(self.num_coarsenings):
            ne, npt = C.c_int(0), C.c_int(0)
            _check(load().saamge_amd_partitioning_get(self.h, C.c_int(k), None, C.byref(ne), C.byref(npt)))
            self.n_elem.append(int(ne.value))
            self.nparts.append(int(npt.value))

    def pointers(self, on_host=False):
        """Raw addresses of the partition arrays (device, or the handle's host copies), one per coarsening."""
        pp = C.POINTER(C.c_void_p)()
        _check(load().saamge_amd_partitioning_arrays(self.h, C.c_int(int(on_host)), C.byref(pp), None))
        return [int(pp[k] or 0) for k in range(self.num_coarsenings)]

    def part(self, level):
        out = np.zeros(max(self.n_elem[level], 1), np.int32)[:self.n_elem[level]]
        _check(load().saamge_amd_partitioning_get(self.h, C.c_int(level), _ptr(out), None, None))
        return out

    def graph(self, level, device=False):
        """(xadj int64, adj int32) of graph `level` (0: elements, k: the quotient graph of level k - 1): numpy arrays, or
        torch tensors on the GPU with device=True."""
        n, nnz = C.c_int(0), C.c_longlong(0)
        _check(load().saamge_amd_partitioning_graph(self.h, C.c_int(level), None, None, C.byref(n), C.byref(nnz)))
        if device:
            import torch
            xadj = torch.zeros(n.value + 1, dtype=torch.int64, device="cuda")
            adj = torch.zeros(int(nnz.value), dtype=torch.int32, device="cuda")
        else:
            xadj = np.zeros(n.value + 1, np.int64)
            adj = np.zeros(max(int(nnz.value), 1), np.int32)[:int(nnz.value)]
        _check(load().saamge_amd_partitioning_graph(self.h, C.c_int(level), _ptr(xadj), _ptr(adj), None, None))
        return xadj, adj


def partition_mesh(elem_to_dof, ND, elems_per_agg, elem_ptr=None, **kw):
    return Partitioning(elem_to_dof, ND, elems_per_agg, elem_ptr=elem_ptr, **kw)


class _DevicePointer(object):
    """A raw device address with the dtype the entry points look at (`Hierarchy` picks the 64-bit entry by it)."""

    def __init__(self, address, dtype):
        self._address, self.dtype = int(address or 0), dtype

    def data_ptr(self):
        return self._address


class Operator(_Handle):
    """saamge_amd_operator_assemble: the fine operator assembled on the device from the element matrices, owned by the
    library until close().  saamge_amd/assemble_model.py defines its pattern and values."""
    _FREE = "saamge_amd_operator_free"

    def __init__(self, n, elem_to_dof, elmat, bdr=None, elem_ptr=None, nde=0, NE=None, stream=0):
        if NE is None:
            NE = len(elem_ptr) - 1 if elem_ptr is not None else int(elem_to_dof.shape[0])
        if elem_ptr is None and not nde:
            nde = int(elem_to_dof.shape[1])
        h = C.c_void_p()
        _check(load().saamge_amd_operator_assemble(C.c_int(int(n)), C.c_int(int(NE)), C.c_int(int(nde)), _ptr(elem_ptr),
                                                   _ptr(elem_to_dof), _ptr(elmat), _ptr(bdr), C.c_void_p(stream), C.byref(h)))
        self.h = h
        self.n = int(n)
        nnz = C.c_longlong(0)
        _check(load().saamge_amd_operator_get(self.h, None, None, None, C.byref(nnz)))
        self.nnz = int(nnz.value)

    @classmethod
    def assemble(cls, prob, stream=0, device=False):
        """From a problems.Problem: its host arrays, or (device=True) copies of them on the GPU."""
        def arr(a, dt):
            if a is None or hasattr(a, "data_ptr"):
                return a
            a = np.ascontiguousarray(a, dtype=dt)
            if device:
                import torch
                return torch.as_tensor(a).cuda()
            return a
        eptr = getattr(prob, "elem_ptr", None)
        e2d = arr(prob.elem_to_dof, np.int32)
        op = cls(prob.ND, e2d, arr(prob.elmat, np.float64), arr(prob.bdr, np.int8), elem_ptr=arr(eptr, np.int32),
                 nde=0 if eptr is not None else int(prob.elem_to_dof.shape[1]), NE=prob.NE, stream=stream)
        return op

    def arrays(self):
        """(rowptr, col, val, nnz): raw device addresses, valid until close()."""
        rp, cp, vp, nnz = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_longlong(0)
        _check(load().saamge_amd_operator_arrays(self.h, C.byref(rp), C.byref(cp), C.byref(vp), C.byref(nnz)))
        return int(rp.value or 0), int(cp.value or 0), int(vp.value or 0), int(nnz.value)

    def get(self, device=False):
        """(rowptr int64, col int32, val float64): numpy arrays, or torch tensors on the GPU with device=True."""
        if device:
            import torch
            rowptr = torch.zeros(self.n + 1, dtype=torch.int64, device="cuda")
            col = torch.zeros(self.nnz, dtype=torch.int32, device="cuda")
            val = torch.zeros(self.nnz, dtype=torch.float64, device="cuda")
        else:
            rowptr = np.zeros(self.n + 1, np.int64)
            col = np.zeros(max(self.nnz, 1), np.int32)[:self.nnz]
            val = np.zeros(max(self.nnz, 1), np.float64)[:self.nnz]
        _check(load().saamge_amd_operator_get(self.h, _ptr(rowptr), _ptr(col), _ptr(val), None))
        return rowptr, col, val

    def update(self, elmat):
        """New element matrices (host array or device tensor), same mesh and flags: the values are rewritten in place."""
        if not hasattr(elmat, "data_ptr"):
            elmat = np.ascontiguousarray(elmat, dtype=np.float64)
        _check(load().saamge_amd_operator_update(self.h, _ptr(elmat)))

    def eliminate_rhs(self, elmat, x_ess, b):
        """b (numpy array or device tensor) in place; returns it."""
        if not hasattr(elmat, "data_ptr"):
            elmat = np.ascontiguousarray(elmat, dtype=np.float64)
        _check(load().saamge_amd_operator_eliminate_rhs(self.h, _ptr(elmat), _ptr(x_ess), _ptr(b)))
        return b

    def assemble_rhs(self, elvec, b=None, device=False):
        """b (n, overwritten; a new numpy array, or device tensor with device=True, when None) from the packed element vectors
        of `element_loads` on the operator's mesh (host array or device tensor); returns b."""
        if not hasattr(elvec, "data_ptr"):
            elvec = np.ascontiguousarray(elvec, dtype=np.float64)
        if b is None:
            b = _new_doubles(self.n, device)
        _check(load().saamge_amd_operator_assemble_rhs(self.h, _ptr(elvec), _ptr(b)))
        return b

    def path_counts(self):
        """Rows by the path they took: {"symbolic": (short, lds, global), "numeric": (short, lds, global)}."""
        c = (C.c_longlong * 6)()
        _check(load().saamge_amd_operator_path_counts(self.h, c))
        return {"symbolic": tuple(int(v) for v in c[:3]), "numeric": tuple(int(v) for v in c[3:])}


def operator_path_limits(short_candidates=-1, lds_candidates=-1):
    """Tests: candidate limits of the short and the LDS path of the assemblies that follow (-1: the default)."""
    _check(load().saamge_amd_operator_set_path_limits(C.c_int(int(short_candidates)), C.c_int(int(lds_candidates))))


class LobpcgOptions(C.Structure):      # saamge_amd_lobpcg_options
    _fields_ = [("nev", C.c_int), ("block", C.c_int), ("tol", C.c_double), ("max_iter", C.c_int),
                ("constrain_essential", C.c_int), ("seed", C.c_uint)]


def _block(a):
    """a block of vectors for the C ABI: numpy n x p -> (column-major copy, ld = n); (pointer or tensor, n, p, ld) as given"""
    if isinstance(a, tuple):
        return a
    a = np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(a.T), a.shape[0], a.shape[1], a.shape[0]


def blockvec_gram(S, T=None):
    """G = S^T T (saamge_amd_blockvec_gram); T = None: T is S itself (half the work).  A block: numpy n x p, or
    (pointer / tensor / column-major numpy buffer, n, p, ld)."""
    s, n, p, lds = _block(S)
    t, n2, q, ldt = (s, n, p, lds) if T is None else _block(T)
    assert n2 == n
    G = np.zeros((max(q, 0), max(p, 0)))
    _check(load().saamge_amd_blockvec_gram(C.c_int(n), C.c_int(p), _ptr(s), C.c_longlong(lds), C.c_int(q), _ptr(t),
                                           C.c_longlong(ldt), _ptr(G)))
    return G.T


def blockvec_combine(S, Cm, Y=None, accumulate=False):
    """Y = S C or Y += S C (saamge_amd_blockvec_combine).  S, Y: blocks as blockvec_gram takes them (Y None: a new numpy
    block, returned n x q; Y given as a tuple is written in place and returned as given)."""
    s, n, p, lds = _block(S)
    Cm = np.asarray(Cm, dtype=np.float64)
    q = Cm.shape[1]
    assert Cm.shape[0] == p
    fresh = Y is None or not isinstance(Y, tuple)
    y, n2, q2, ldy = _block(np.zeros((n, q)) if Y is None else Y)
    assert (n2, q2) == (n, q)
    c = np.ascontiguousarray(Cm.T)      # column-major p x q; named, so that it outlives the pointer taken from it
    _check(load().saamge_amd_blockvec_combine(C.c_int(n), C.c_int(p), _ptr(s), C.c_longlong(lds), C.c_int(q),
                                              _ptr(c), _ptr(y), C.c_longlong(ldy), C.c_int(int(accumulate))))
    return y.T if fresh else Y


def pool_counts(reset=False):
    """(hipMalloc calls, their bytes, hipFree of cached blocks, idle bytes) of the library's cache of device blocks since the last reset."""
    c = (C.c_longlong * 4)()
    load().saamge_amd_pool_counts(c, C.c_int(int(reset)))
    return tuple(int(v) for v in c)


def memory_stats(reset_peak=False):
    """(live, peak) device bytes held by the library's buffers (the caller's own arrays and the idle cache not counted)."""
    live, peak = C.c_longlong(0), C.c_longlong(0)
    load().saamge_amd_memory_stats(C.byref(live), C.byref(peak), C.c_int(int(reset_peak)))
    return int(live.value), int(peak.value)


def profile(enable=True):
    load().saamge_amd_profile_enable(C.c_int(int(enable)))


def profile_reset():
    load().saamge_amd_profile_reset()


def profile_stats():
    lib = load()
    out = []
    for i in range(lib.saamge_amd_profile_count()):
        name = C.create_string_buffer(64)
        ms = C.c_double()
        launches = C.c_longlong()
        by = C.c_double()
        fl = C.c_double()
        fb = C.c_double()
        lib.saamge_amd_profile_get2(C.c_int(i), name, C.c_int(64), C.byref(ms), C.byref(launches),
                                    C.byref(by), C.byref(fl), C.byref(fb))
        out.append(dict(name=name.value.decode(), ms=ms.value, launches=launches.value,
                        bytes=by.value, flops=fl.value, fmt_bytes=fb.value))
    return out
