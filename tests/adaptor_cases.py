"""What tests/cxx/mfem_adaptor_run reads and writes: a flat little-endian container of named arrays, and the problem files
made from saamge_amd.problems for the scenarios of tests/test_gpu_mfem_adaptor.py / tests/test_adaptor_cases.py.

Container:  8 bytes "SAAC1\\0\\0\\0" | u32 number of arrays | per array: u32 length of the name, the name, u32 type code
(0 int32, 1 float64, 2 int8, 3 int64), u64 number of elements, the elements.  A scalar is an array of one element."""
import os
import struct
import subprocess

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "tests", "cxx", "mfem_adaptor_run")
MAGIC = b"SAAC1\0\0\0"
_TYPES = [np.dtype("<i4"), np.dtype("<f8"), np.dtype("i1"), np.dtype("<i8")]


def write_container(path, arrays):
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<I", len(arrays)))
        for name, a in arrays.items():
            a = np.ascontiguousarray(a).ravel()
            if a.dtype == np.bool_:
                a = a.astype(np.int32)
            code = [i for i, t in enumerate(_TYPES) if t == a.dtype.newbyteorder("<") or t == a.dtype]
            assert code, (name, a.dtype)
            nm = name.encode()
            f.write(struct.pack("<I", len(nm)) + nm + struct.pack("<IQ", code[0], a.size) + a.astype(_TYPES[code[0]]).tobytes())


def read_container(path):
    with open(path, "rb") as f:
        raw = f.read()
    assert raw[:8] == MAGIC, raw[:8]
    (count,), off, out = struct.unpack_from("<I", raw, 8), 12, {}
    for _ in range(count):
        (ln,) = struct.unpack_from("<I", raw, off)
        name = raw[off + 4:off + 4 + ln].decode()
        code, n = struct.unpack_from("<IQ", raw, off + 4 + ln)
        off += 4 + ln + 12
        out[name] = np.frombuffer(raw, dtype=_TYPES[code], count=n, offset=off).copy()
        off += n * _TYPES[code].itemsize
    assert off == len(raw)
    return out


def text(a):
    """An int8 array of the container as the string it holds."""
    return bytes(np.asarray(a, dtype=np.int8).view(np.uint8)).decode()


def run_driver(problem_file, scenarios, out_file, timeout=120):
    """One child process for all `scenarios` of one problem -> the arrays it wrote (names prefixed "<scenario>.")."""
    assert os.path.exists(PROGRAM), "tests/cxx/mfem_adaptor_run is missing: build() (make -C saamge_amd/csrc) builds it"
    p = subprocess.run([PROGRAM, str(problem_file), ",".join(scenarios), str(out_file)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=timeout, text=True)
    assert p.returncode == 0, "%s %s: exit status %d\n%s" % (PROGRAM, ",".join(scenarios), p.returncode, p.stdout)
    return read_container(out_file)


def diag_first_unsorted(A):
    """The rows of A the way hypre keeps a square diagonal block: the diagonal entry first, the rest in no order (here: descending
    columns, rotated by the row number) -> rowptr, col, val.  The adaptor's csr_of has to sort them."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    col, val = A.indices.astype(np.int32).copy(), A.data.astype(np.float64).copy()
    for i in range(A.shape[0]):
        lo, hi = A.indptr[i], A.indptr[i + 1]
        c, v = col[lo:hi], val[lo:hi]
        d = np.flatnonzero(c == i)
        rest = np.flatnonzero(c != i)[::-1]
        if rest.size:
            rest = np.roll(rest, i % rest.size)
        order = np.concatenate([d, rest])
        col[lo:hi], val[lo:hi] = c[order], v[order]
    return A.indptr.astype(np.int32), col, val


def element_graph(elem_ptr, elem_to_dof, min_shared):
    """elem_to_elem as MFEM's ElementToElementTable gives it: the elements across a face (at least min_shared common dofs),
    without the element itself -> (I, J)."""
    elem_ptr, elem_to_dof = np.asarray(elem_ptr), np.asarray(elem_to_dof).ravel()
    NE = len(elem_ptr) - 1
    rows = np.repeat(np.arange(NE), np.diff(elem_ptr))
    E = sp.csr_matrix((np.ones(elem_to_dof.size, dtype=np.int32), (rows, elem_to_dof)))
    S = sp.csr_matrix(E @ E.T)
    S.setdiag(0)
    S.data[S.data < min_shared] = 0
    S.eliminate_zeros()
    S.sort_indices()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32)


def problem_arrays(prob, coarsenings, nparts=None, dim=3, **scalars):
    """The input file of a problem of saamge_amd.problems: A diagonal-first and unsorted, the element arrays, elem_to_elem, the
    flags, one partition per coarsening that the problem has (the others come from a hook), b and a start vector, and scalars."""
    rowptr, col, val = diag_first_unsorted(prob.A)
    mixed = getattr(prob, "elem_ptr", None) is not None
    e2d = np.asarray(prob.elem_to_dof, dtype=np.int32)
    eptr = np.asarray(prob.elem_ptr, dtype=np.int32) if mixed else np.arange(e2d.shape[0] + 1, dtype=np.int32) * e2d.shape[1]
    gI, gJ = element_graph(eptr, e2d, 2 if dim == 2 else 3)
    n = prob.A.shape[0]
    parts = [np.asarray(p, dtype=np.int32) for p in prob.partitions[:coarsenings]]
    if nparts is None:
        nparts = [int(p.max()) + 1 for p in parts]
    out = {"A_rowptr": rowptr, "A_col": col, "A_val": val, "elem_to_dof": e2d.ravel(),
           "elmat": np.asarray(prob.elmat, dtype=np.float64).ravel(), "e2e_I": gI, "e2e_J": gJ,
           "bdr": np.asarray(prob.bdr, dtype=np.int8),
           # a boundary attribute per dof for the stand-in space: 4 on the essential boundary (mltest.mesh's attribute), 0 inside
           "bdr_attribute": np.where(np.asarray(prob.ess), 4, 0).astype(np.int32),
           "nparts": np.asarray(nparts, dtype=np.int32), "b": np.asarray(prob.b, dtype=np.float64),
           "x0": np.sin(0.37 * np.arange(n)) * (~np.asarray(prob.ess)), "coarsenings": np.int32(coarsenings)}
    if mixed:
        out["elem_ptr"] = eptr
    else:
        out["nde"] = np.int32(e2d.shape[1])
    for k, p in enumerate(parts):
        out["part%d" % k] = p
    for k, v in scalars.items():
        out[k] = np.float64(v) if isinstance(v, float) else np.int32(v)
    return out


def algebraic_arrays(A, part, theta):
    """tg_produce_data_algebraic's inputs: the matrix and the dof -> AE map."""
    rowptr, col, val = diag_first_unsorted(A)
    n = A.shape[0]
    return {"A_rowptr": rowptr, "A_col": col, "A_val": val, "part0": np.asarray(part, dtype=np.int32),
            "nparts": np.asarray([int(np.max(part)) + 1], dtype=np.int32), "b": np.ones(n), "x0": np.sin(0.37 * np.arange(n)),
            "theta": np.float64(theta), "coarsenings": np.int32(1)}


def scaled_values(A, k):
    """Values of D A D, D = diag(1 + 0.1 sin(i + k)), in A's own (given) entry order: same pattern, still SPD."""
    rowptr, col, val = A
    d = 1.0 + 0.1 * np.sin(np.arange(len(rowptr) - 1) + float(k))
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return d[rows] * val * d[col]
