// Element matrices computed on the device from vertex coordinates, element -> vertex lists and per-element coefficients
// (elmat.hip).  saamge_amd/elmat_model.py defines the result -- types, rules, the order of every operation -- and the kernels
// give the same bits.
#pragma once
#include "common.h"

#include <string>

#include "mesh.h"      // MeshArgs: the mesh arguments every call below starts with

namespace saamge_amd {

// The arguments of saamge_amd_element_matrices after the mesh.  The checks that need no device run before the first HIP call;
// info is filled before a refusal for a non-positive Jacobian is thrown.  Every call below runs on s and returns with s idle.
void element_matrices(hipStream_t s, const MeshArgs &m, int kind, int ncoef, const double *coef, double *elmat_out, int *dof_ptr_out,
                      int *elem_to_dof_out, long long info[8]);

// The arguments of saamge_amd_element_mass: the mass matrices with the per-element coefficient coef, vdim 1 or dim; accumulate:
// added to the matrices elmat_inout holds.  elmat_model.element_mass defines the result.
void element_mass(hipStream_t s, const MeshArgs &m, int vdim, const double *coef, int accumulate, double *elmat_inout,
                  long long info[8]);
// The arguments of saamge_amd_element_loads: the load vectors of the nodal source src (NV x vdim); coef NULL: 1.0.
void element_loads(hipStream_t s, const MeshArgs &m, int vdim, const double *coef, const double *src, double *elvec_out,
                   long long info[8]);

// The arguments of saamge_amd_boundary_mass: the mass matrices of the NF listed faces (element face_elem[f], local face
// face_local[f], coefficient coef[f]) added to the matrices elmat_inout holds.  elmat_model.boundary_mass defines the result.
void boundary_mass(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim, const double *coef,
                   double *elmat_inout, long long info[8]);
// The arguments of saamge_amd_boundary_loads: the load vectors of the nodal g (NV x vdim) on the listed faces added to the
// vectors elvec_inout holds; coef NULL: 1.0.  elmat_model.boundary_loads defines the result.
void boundary_loads(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim, const double *coef,
                    const double *g, double *elvec_inout, long long info[8]);

// Boundary data at the face points (elmat_model.boundary_points / boundary_eval / boundary_mass_points / boundary_loads_points):
// point q of face f of the list has the global index fp_ptr[f] + q, NFQ = fp_ptr[NF], in the order of the LIST.  Face lists, checks
// and info[0..4], [6], [7] as boundary_mass; every pointer host or device; a refusal writes no output.
// The arguments of saamge_amd_boundary_points: fp_ptr_out (NF + 1), xq_out (NFQ x dim), wmeas_out (NFQ), normal_out (NFQ x dim), the
// unit normal out of the owning element; any of them may be NULL.  info[5] = NFQ.
void boundary_points(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, long long *fp_ptr_out,
                     double *xq_out, double *wmeas_out, double *normal_out, long long info[8]);
// The arguments of saamge_amd_boundary_eval: the nodal u (NV x vdim) at the face points, uq_out (NFQ x vdim) the trace and gradq_out
// (NFQ x vdim x dim) the whole gradient of the owning element's field; either may be NULL.  The first face whose element has a
// non-positive determinant at a face point is refused.  info[5] = NFQ.
void boundary_eval(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim, const double *u,
                   double *uq_out, double *gradq_out, long long info[8]);
// The arguments of saamge_amd_boundary_mass_points: boundary_mass with the coefficient coefq (NFQ) given at the face points.
void boundary_mass_points(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim,
                          const double *coefq, double *elmat_inout, long long info[8]);
// The arguments of saamge_amd_boundary_loads_points: boundary_loads of gq (NFQ x vdim) given at the face points; coef (NF) NULL: 1.0.
void boundary_loads_points(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim,
                           const double *coef, const double *gq, double *elvec_inout, long long info[8]);

// Data at the points of the mass rule (elmat_model.element_points / element_eval / element_loads_points / element_errors): point q
// of element e has the global index qp_ptr[e] + q, NQ = qp_ptr[NE].  Every pointer host or device; a refusal writes no output.
// The arguments of saamge_amd_element_points: qp_ptr_out (NE + 1), xq_out (NQ x dim), wdet_out (NQ); any of them may be NULL.
void element_points(hipStream_t s, const MeshArgs &m, long long *qp_ptr_out, double *xq_out, double *wdet_out, long long info[8]);
// The arguments of saamge_amd_element_eval: the nodal u (NV x vdim) at the points, uq_out (NQ x vdim) and gradq_out
// (NQ x vdim x dim); either may be NULL.
void element_eval(hipStream_t s, const MeshArgs &m, int vdim, const double *u, double *uq_out, double *gradq_out, long long info[8]);
// The arguments of saamge_amd_element_loads_points: the load vectors of fq (NQ x vdim) given at the points, in the layout of
// element_loads; coef NULL: 1.0.
void element_loads_points(hipStream_t s, const MeshArgs &m, int vdim, const double *coef, const double *fq, double *elvec_out,
                          long long info[8]);
// The arguments of saamge_amd_element_errors: err_out (NE x 2), the squared errors of the nodal u against exq (NQ x vdim) and of
// its gradient against exgradq (NQ x vdim x dim); exact data NULL: that column is 0.0.
void element_errors(hipStream_t s, const MeshArgs &m, int vdim, const double *u, const double *exq, const double *exgradq,
                    double *err_out, long long info[8]);

// Coefficients at the points (elmat_model.element_matrices_points / element_mass_points): the calls above with a coefficient row
// per point of the MASS rule -- row qp_ptr[e] + q of coefq belongs to point q of element e -- in the place of one per element.
// The arguments of saamge_amd_element_matrices_points (coefq NQ x ncoef; the stiffness forms integrate with the mass rule here)
// and of saamge_amd_element_mass_points (coefq NQ); checks, outputs and info as element_matrices / element_mass.
void element_matrices_points(hipStream_t s, const MeshArgs &m, int kind, int ncoef, const double *coefq, double *elmat_out,
                             int *dof_ptr_out, int *elem_to_dof_out, long long info[8]);
void element_mass_points(hipStream_t s, const MeshArgs &m, int vdim, const double *coefq, int accumulate, double *elmat_inout,
                         long long info[8]);

}  // namespace saamge_amd
