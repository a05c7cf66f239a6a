/*
 * caar_f90.h — compute_and_apply_rhs directly on Fortran-ordered device arrays.
 *
 * Additive to include/caar.h (included here) and NOT part of its frozen ABI 6 surface; exported by the same
 * libcaar_hip.so.  For a Fortran host (HOMME) whose 16 element arrays already live on the device in Fortran order —
 * first index fastest, the element index last:
 *     v(np,np,2,nlev,timelevels,ne)  T,dp3d(np,np,nlev,timelevels,ne)  Qdp(np,np,nlev,qsize_d,2,ne)
 *     phi,omega_p,pecnd(np,np,nlev,ne)  vn0(np,np,2,nlev,ne)  eta_dot_dpdn(np,np,nlev+1,ne)
 *     D,Dinv(np,np,2,2,ne)  fcor,spheremp,metdet,rmetdet,phis(np,np,ne)
 * (the arrays caar_layout_from_f90 takes, caar.h "Fortran-layout ingest / egress").  The kernels read and write them in
 * place: one pass over the arrays per call, no layout conversion, no second copy, bit-identical to caar_launch on the
 * same values in the C++ layout.
 *
 * caar_arrays_alloc (caar.h) may allocate these arrays: caar_array_len is the same for both orders, so a Fortran host
 * gets the bandwidth-placed allocation too — it simply stores Fortran-ordered data in the 16 buffers.
 */
#ifndef CAAR_F90_H
#define CAAR_F90_H

#include "caar.h"

#ifdef __cplusplus
extern "C" {
#endif

/* caar_launch on Fortran-ordered arrays: one compute_and_apply_rhs for elements [params->nets, params->nete).  `f90_dev`
 * holds DEVICE pointers to the arrays above in CaarArrays member order; 8-byte alignment is enough for every array.
 * `dvv_dev`: a DEVICE buffer of np*np doubles holding params->Dvv (row-major Dvv[i][j], as for caar_launch).  Asynchronous
 * on `stream` (a hipStream_t, NULL = default stream), no allocation, no synchronisation, safe to capture in a hipGraph.
 * The arguments are validated as by caar_launch, before any HIP call.  The vertically Lagrangian form only: rsplit == 0,
 * and any (np, nlev) caar_supported refuses, return CAAR_EUNSUPPORTED with nothing enqueued.  The cache window of
 * caar_set_cache_window (caar_tuning.h) applies as for caar_launch; the adaptive window does not tune these launches. */
int caar_launch_f90(const CaarDims *dims, const CaarArrays *f90_dev, const double *dvv_dev, const CaarParams *params,
                    void *stream);

/* `nsteps` (>= 1) consecutive caar_launch_f90 calls, with TestData::update_time_levels (np1, nm1, n0 <- nm1, n0, np1)
 * between them if rotate != 0: nsteps launches (there is no fused Fortran-order step-loop kernel).  Bit-identical to
 * caar_launch_steps on the same values in the C++ layout. */
int caar_launch_steps_f90(const CaarDims *dims, const CaarArrays *f90_dev, const double *dvv_dev, const CaarParams *params,
                          int nsteps, int rotate, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CAAR_F90_H */
