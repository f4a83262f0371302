// Element matrices computed on the device from vertex coordinates, element -> vertex lists and per-element coefficients
// (elmat.hip).  saamge_amd/elmat_model.py defines the result -- types, rules, the order of every operation -- and the kernels
// give the same bits.
#pragma once
#include "common.h"

namespace saamge_amd {

// The arguments of saamge_amd_element_matrices (include/saamge_amd.h).  The checks that need no device run before the first
// HIP call; info is filled before a refusal for a non-positive Jacobian is thrown.  Runs on s and returns with s idle.
void element_matrices(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                      const int *elem_to_vertex, int kind, int ncoef, const double *coef, double *elmat_out, int *dof_ptr_out,
                      int *elem_to_dof_out, long long info[8]);

// The arguments of saamge_amd_element_mass: the mass matrices with the per-element coefficient coef, vdim 1 or dim; accumulate:
// added to the matrices elmat_inout holds.  elmat_model.element_mass defines the result.
void element_mass(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                  const int *elem_to_vertex, int vdim, const double *coef, int accumulate, double *elmat_inout, long long info[8]);
// The arguments of saamge_amd_element_loads: the load vectors of the nodal source src (NV x vdim); coef NULL: 1.0.
void element_loads(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                   const int *elem_to_vertex, int vdim, const double *coef, const double *src, double *elvec_out,
                   long long info[8]);

// The arguments of saamge_amd_boundary_mass: the mass matrices of the NF listed faces (element face_elem[f], local face
// face_local[f], coefficient coef[f]) added to the matrices elmat_inout holds.  elmat_model.boundary_mass defines the result.
void boundary_mass(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                   const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim, const double *coef,
                   double *elmat_inout, long long info[8]);
// The arguments of saamge_amd_boundary_loads: the load vectors of the nodal g (NV x vdim) on the listed faces added to the
// vectors elvec_inout holds; coef NULL: 1.0.  elmat_model.boundary_loads defines the result.
void boundary_loads(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                    const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim, const double *coef,
                    const double *g, double *elvec_inout, long long info[8]);

}  // namespace saamge_amd
