// caar_f90.hip — compute_and_apply_rhs on Fortran-ordered device arrays (include/caar_f90.h), hand-written HIP for gfx950.
//
// A HOMME host keeps the 16 element arrays with the first index fastest (include/caar.h "Fortran-layout ingest / egress").
// Nothing in the kernels ties them to the C++ order: elements are the slowest index in both orders, a tile of 4 levels x 16
// points (NP=4) or one level (NP=8) is the same contiguous 512 B block (1 KiB for v) in both, and only the place of a point
// inside a level and the order of the small inner axes of v, vn0, D, Dinv and Qdp differ.  So these kernels run the SAME
// element bodies as caar_np4.hip / caar_np8.hip with the layout parameter F90 = true (caar_np4_kernel.h, caar_np8_kernel.h):
// the same bytes move in the same cache lines, with the same arithmetic in the same order — bit-identical results to
// caar_launch on the same inputs in C++ order — and a Fortran host needs neither the two layout passes of
// caar_layout_from_f90 / caar_layout_to_f90 nor a second copy of the arrays.
//
// Only what a default launch of the vertically Lagrangian form (rsplit > 0) reaches is instantiated, each kernel with the
// launch shape, cache policy and element mapping of its C++-layout twin (the default variant of caar_np4.hip /
// caar_np8.hip): 18 NP=4 kernels (NLEV 72 and 128, the seven run-time-level-count shapes, moist and dry) and 2 NP=8 ones.
#include <hip/hip_runtime.h>

#include "caar_np4_kernel.h"
#include "caar_np8_kernel.h"

namespace caar {

// caar_np4_kernel's twin (same launch bounds, same LDS, POL as there) on Fortran-ordered arrays
template <int NLEV_T, int TPW, int MINW, bool MOIST, int POL, int PF, int DYNW = 8, int PARK = 0>
__global__ __launch_bounds__(NLEV_T ? ((NLEV_T + 3) / 4 + TPW - 1) / TPW * 64 : DYNW * 64, MINW) void caar_np4_f90_kernel(const KernelArgs k) {
  request_kernel_args(k);
  __shared__ Np4Lds<NLEV_T, TPW, false, false, DYNW, PARK> lds;
  if constexpr (POL == 2) {  // hybrid cache policy: the accumulators of the elements element_is_cached picks stay in the cache
    const long long ie_s = element_of_block(k, blockIdx.x);
    if (ie_s < 0) return;
    if (element_is_cached(k, ie_s))
      caar_np4_element<NLEV_T, TPW, MINW, MOIST, true, false, PF, false, false, false, DYNW, PARK, false, 0, 0, -1, 0, true>(k, lds, nullptr, 3, 0, ie_s);
    else
      caar_np4_element<NLEV_T, TPW, MINW, MOIST, true, true, PF, false, false, false, DYNW, PARK, false, 0, 0, -1, 0, true>(k, lds, nullptr, 3, 0, ie_s);
  } else {
    caar_np4_element<NLEV_T, TPW, MINW, MOIST, POL == 1, POL == 1, PF, false, false, false, DYNW, PARK, false, 0, 0, -1, 0, true>(k, lds);
  }
}

// caar_np8_kernel's MFMA form (the default variant) on Fortran-ordered arrays
template <int NLEV, int TPW, int MINW, bool MOIST, bool SNT, int LA>
__global__ __launch_bounds__(NLEV / TPW * 64, MINW) void caar_np8_f90_kernel(const KernelArgs k) {
  request_kernel_args(k);
  __shared__ Np8Lds<NLEV, TPW, false, false, true> lds;
  caar_np8_element<NLEV, TPW, MINW, MOIST, SNT, false, false, false, false, true, LA, false, 0, true>(k, lds);
}

// NLEV 72 / 128: the shapes of kNp4Nlev72[0] (4 waves x 5, 5, 4, 4 tiles) and kNp4Nlev128[0] (4 waves x 8 tiles, scan results
// parked), hybrid cache policy
template <int NLEV, int TPW, int MINW, int PARK>
static hipError_t launch_np4_f90(const KernelArgs& k, int num_elems, hipStream_t stream) {
  constexpr int THREADS = ((NLEV + 3) / 4 + TPW - 1) / TPW * 64;
  const int grid = k.per_xcd ? 8 * k.per_xcd : num_elems;
  if (k.qn0 >= 0)
    hipLaunchKernelGGL((caar_np4_f90_kernel<NLEV, TPW, MINW, true, 2, 0, 8, PARK>), dim3(grid), dim3(THREADS), 0, stream, k);
  else  // dry branch (P:128-139)
    hipLaunchKernelGGL((caar_np4_f90_kernel<NLEV, TPW, MINW, false, 2, 0, 8, PARK>), dim3(grid), dim3(THREADS), 0, stream, k);
  return hipGetLastError();
}

// any other level count in 2..256: the run-time-level-count shapes of caar_np4.hip launch_np4_dyn (its rsplit > 0 choices)
template <int TPW, int MAXW, int PF, int PARK = 0>
static hipError_t launch_np4_f90_dyn_shape(const KernelArgs& k, int num_elems, hipStream_t stream) {
  const int tiles = (k.nlev + 3) / 4, waves = (tiles + TPW - 1) / TPW;
  const int grid = k.per_xcd ? 8 * k.per_xcd : num_elems;
  if (waves > MAXW) return hipErrorInvalidValue;
  if (k.qn0 >= 0)
    hipLaunchKernelGGL((caar_np4_f90_kernel<0, TPW, 1, true, 2, PF, MAXW, PARK>), dim3(grid), dim3(waves * 64), 0, stream, k);
  else
    hipLaunchKernelGGL((caar_np4_f90_kernel<0, TPW, 1, false, 2, PF, MAXW, PARK>), dim3(grid), dim3(waves * 64), 0, stream, k);
  return hipGetLastError();
}
static hipError_t launch_np4_f90_dyn(const KernelArgs& k, int num_elems, hipStream_t stream) {
  if (k.nlev < 2 || k.nlev > 256) return hipErrorInvalidValue;
  const int tiles = (k.nlev + 3) / 4;
  if (tiles <= 8) return launch_np4_f90_dyn_shape<2, 8, 1>(k, num_elems, stream);       // <= 4 waves x 2 tiles
  if (tiles <= 12) return launch_np4_f90_dyn_shape<3, 8, 0>(k, num_elems, stream);      // 4 waves x 3
  if (tiles <= 16) return launch_np4_f90_dyn_shape<4, 8, 0>(k, num_elems, stream);      // 4 waves x 4
  if (tiles <= 20) return launch_np4_f90_dyn_shape<5, 8, 0>(k, num_elems, stream);      // 4 waves x 5
  if (tiles <= 24) return launch_np4_f90_dyn_shape<6, 8, 0>(k, num_elems, stream);      // 4 waves x 6
  if (tiles <= 32) return launch_np4_f90_dyn_shape<8, 4, 0, 27>(k, num_elems, stream);  // 4 waves x 8, scan results parked
  return launch_np4_f90_dyn_shape<8, 8, 0, 27>(k, num_elems, stream);                   // <= 8 waves x 8, parked
}

// NP=8 NLEV=72: the shape of kNp8Nlev72[0] (8 waves x 9 levels, all streaming, update inputs two levels ahead)
static hipError_t launch_np8_f90_72(const KernelArgs& k, int num_elems, hipStream_t stream) {
  const int grid = k.per_xcd ? 8 * k.per_xcd : num_elems;
  if (k.qn0 >= 0)
    hipLaunchKernelGGL((caar_np8_f90_kernel<72, 9, 1, true, true, 2>), dim3(grid), dim3(512), 0, stream, k);
  else
    hipLaunchKernelGGL((caar_np8_f90_kernel<72, 9, 1, false, true, 2>), dim3(grid), dim3(512), 0, stream, k);
  return hipGetLastError();
}

struct F90Kernel {
  hipError_t (*launch)(const KernelArgs&, int num_elems, hipStream_t stream);
  bool prefers_xcd_chunked;  // the twin's measured element mapping (KernelVariant::prefers_xcd_chunked)
};

// The Fortran-order kernel for (np, nlev), launch == nullptr if there is none.  (The vertically Lagrangian form only: the
// caller refuses rsplit == 0.)
F90Kernel f90_kernel(int np, int nlev) {
  if (np == 4 && nlev == 72) return {launch_np4_f90<72, 5, 1, 0>, true};
  if (np == 4 && nlev == 128) return {launch_np4_f90<128, 8, 2, 27>, true};
  if (np == 4 && nlev >= 2 && nlev <= 256) return {launch_np4_f90_dyn, false};
  if (np == 8 && nlev == 72) return {launch_np8_f90_72, true};
  return {nullptr, false};
}

}  // namespace caar
