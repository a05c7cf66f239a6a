/*
 * caar_dss.h — direct stiffness summation (DSS) of the new time level on the device.
 *
 * Additive to include/caar.h (included here) and NOT part of its frozen ABI 6 surface; exported by the same
 * libcaar_hip.so.  compute_and_apply_rhs leaves T, v and dp3d at np1 as element-local values multiplied by the mass
 * matrix, spheremp * (x(nm1) + dt2 * tendency) (routine_mod.F90:183-187).  HOMME then packs them into an edge buffer,
 * exchanges it (bndry_exchangeV), sums every GLL point that several elements share and multiplies by rspheremp
 * (routine_extracted.F90:533-611).  caar_dss_launch does that step for the elements one device holds.
 *
 * Contract
 *   - A mesh is given as HOMME gives it: gdof, a 64-bit global id for every GLL point of every element, C++ layout
 *     gdof[ie][a][b] or Fortran layout gdofP(a+1,b+1,ie) (the same logical array).  Points with equal ids are one point.
 *     Ids must be >= 0 and need not be dense.  An interior point (0 < a, b < np-1) must have an id of its own.
 *   - For each global point, its sharers are ordered by (ie, a*np+b) ascending; S = ((x0 + x1) + x2) + ... from the first
 *     sharer, left to right.  Every copy receives rspheremp[ie][a][b] * S.  Where rspheremp is equal across the copies of a
 *     point (as 1/sum(spheremp) is), all copies come out bitwise equal.
 *   - It applies to every level of T, both components of v and dp3d at one time level tl, in place.  Other time levels and
 *     other arrays do not change.
 *   - A plan assembles over the elements it holds.  A point of an element edge that no other held element shares keeps the
 *     sum over the sharers present (exact on a closed mesh held by one device); such points are counted as open
 *     (caar_dss_plan_info): a sharded host knows from it that its halo is not exchanged.  A point is open when one of the
 *     element-boundary segments it ends (two neighbouring boundary points of one element edge, as an unordered pair of
 *     ids) occurs in only one element of the plan.
 *   - At most CAAR_DSS_MAX_SHARERS sharers per point.
 */
#ifndef CAAR_DSS_H
#define CAAR_DSS_H

#include "caar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CAAR_DSS_MAX_SHARERS 8

/* Layout of gdof, rspheremp and the state arrays. */
enum {
  CAAR_DSS_LAYOUT_CXX = 0, /* gdof, rspheremp [ie][a][b]; T, dp3d [ie][tl][nlev][a][b]; v [ie][tl][nlev][a][b][2] (caar.h)  */
  CAAR_DSS_LAYOUT_F90 = 1  /* gdofP, rspheremp (a,b,ie); T, dp3d (a,b,nlev,tl,ie); v (a,b,2,nlev,tl,ie) (caar_f90.h)         */
};

typedef struct CaarDssPlan CaarDssPlan;

/* Builds the sharer lists of the mesh `gdof_host` (a HOST array of dims->num_elems * np * np ids in `layout`) once on the
 * host, uploads them to HIP device `device` and allocates the plan's edge buffer there
 * (num_elems * 4*(np-1) * 4*nlev doubles).  dims->np, dims->nlev and dims->num_elems are fixed for the plan; qsize_d and
 * timelevels are not read.  device < 0 builds a host-only plan: caar_dss_plan_info works, caar_dss_launch refuses it with
 * CAAR_ENODEVICE.  Returns CAAR_EINVAL for a null pointer, a bad layout, num_elems < 0, a negative id or an interior point
 * that shares its id; CAAR_EUNSUPPORTED for an (np, nlev) caar_supported refuses or a point with more than
 * CAAR_DSS_MAX_SHARERS sharers; CAAR_ENOMEM; a HIP error.  Synchronous; *plan is NULL on failure. */
int caar_dss_plan_create(CaarDssPlan **plan, const CaarDims *dims, const long long *gdof_host, int layout, int device);
/* Frees the plan's device storage (synchronises its device first, so no DSS on it may still be running).  NULL is a
 * no-op.  Not during a hipGraph capture: the synchronisation would invalidate it. */
void caar_dss_plan_destroy(CaarDssPlan *plan);
/* What the plan found: distinct ids, ids with more than one sharer, open points (see above), the largest sharer count.
 * Any output pointer may be NULL. */
int caar_dss_plan_info(const CaarDssPlan *plan, long long *unique_points, long long *shared_points, long long *open_points,
                       int *max_sharers);
/* One DSS of T, v and dp3d at time level `tl` of `arrays_dev` (DEVICE pointers; only elem_state_T, elem_state_v and
 * elem_state_dp3d are read, 8-byte aligned) given in `layout`, with `rspheremp_dev` (DEVICE, num_elems * np * np doubles
 * in the same layout), all on the plan's device.  Two kernels in stream order on `stream`, a hipStream_t of the plan's
 * device (NULL: the default stream of the calling thread's current device, which must then be the plan's): a pack of the
 * element boundaries into the plan's edge buffer, then the summation, which writes every point of every element back.  No allocation, no synchronisation: safe to capture in a hipGraph.  The arguments are checked before
 * any HIP call: a null pointer, dims that differ from the plan's (np, nlev, num_elems) or have timelevels < 1, a layout
 * other than the plan's and tl outside [0, timelevels) return CAAR_EINVAL with nothing enqueued.
 * ONE DSS MAY BE IN FLIGHT PER PLAN: the plan owns the edge buffer, so two launches on different streams must be ordered by
 * the host (an event), or use two plans. */
int caar_dss_launch(const CaarDssPlan *plan, const CaarDims *dims, int layout, const CaarArrays *arrays_dev, int tl,
                    const double *rspheremp_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CAAR_DSS_H */
