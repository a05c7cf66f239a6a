// caar_np8.hip — compute_and_apply_rhs for NP=8 on gfx950 (MI355X), hand-written HIP.
//
// Same algorithm and reference citations as caar_np4.hip (P = cxx/pointers_only/
// compute_and_apply_rhs.cpp, S = sphere_operators.cpp); different mapping because one
// level of an NP=8 element is exactly one wavefront:
//   * one workgroup = one element; lane -> GLL point by the MFMA result layout (np8::mfma_point; a*8+b in the
//     LDS-tile comparator variant); a wave owns TPW consecutive
//     levels and walks them in registers, so the three vertical integrals are plain
//     running sums inside a wave (the reference's own summation order within the
//     chunk) plus one wave total per integral exchanged through LDS (two barriers).
//   * every field access of a wave is one contiguous 512 B (scalar) / 1 KiB (v) row of
//     the reference layout [lev][a][b]: each byte read once, written once.
//   * the 8x8 Dvv contractions run on the matrix cores (DEFAULT, MFMA = true): v_mfma_f64_4x4x4, two issues per
//     8x8 product, operands placed by one bank-masked DPP row_ror (d/da) or one ds_bpermute (d/db) per k-block,
//     results landing where the pointwise code needs them — no LDS tile, no LDS copy of Dvv (caar_np8_ops.h "MFMA
//     form"; +1 % A/B against the direct form, profiles/r02/kbench_np8_nlev72_mfma.log).  The direct form (one
//     comparator variant): a wave-private 512 B LDS tile, the field written once and each lane reading its row
//     (4 x ds_read_b128) or column (8 x ds_read_b64), Dvv staged transposed in LDS.
//   * an NP=8 element does not fit the register file the way an NP=4 one does (7 live
//     values x 64 points x 72 levels = 258 KB): between the phases dp, u, v, T of every
//     level are read through a two-deep prefetch ring, dp, u, v are parked in LDS
//     (3 x 36 KB, each lane re-reads only what it wrote) and only {T, T_v, divdp}
//     stay in registers; p, 1/p and the divdp prefix are re-formed
//     in the last phase from the running sums.
#include <hip/hip_runtime.h>

#include "caar_np8_kernel.h"

namespace caar {

template <int NLEV, int TPW, int MINW, bool MOIST, bool SNT, bool COEF_LDS, bool RELOAD_T, bool BATCH, bool VADV = false, bool MFMA = false, int LA = 1>
__global__ __launch_bounds__(NLEV / TPW * 64, MINW) void caar_np8_kernel(const KernelArgs k) {
  request_kernel_args(k);
  __shared__ Np8Lds<NLEV, TPW, BATCH, VADV, MFMA> lds;
  caar_np8_element<NLEV, TPW, MINW, MOIST, SNT, COEF_LDS, RELOAD_T, BATCH, VADV, MFMA, LA>(k, lds);
}

// caar_run_steps / caar_launch_steps as ONE launch for NP=8 (the MFMA form; see caar_np4_steps.hip): every
// workgroup makes all nsteps calls for its element.  With rotating, distinct time levels the first call loads everything
// and every later call finds dp3d, u, v at n0 in the LDS park and T in registers, where the previous call left its np1
// results, and its nm1 state — the n0 state of the call before — in registers too (36 doubles per lane: a 512-thread
// workgroup alone on its CU may use 256 VGPRs); the state is therefore stored by the last three calls only (the earlier
// stores would be overwritten unread).  Default cache policy, so that the accumulators are re-read from the L2 that
// holds them.  Bit-identical to nsteps single launches.
template <int NLEV, int TPW, int MINW, bool MOIST, bool SNT, int LA>
__global__ __launch_bounds__(NLEV / TPW * 64, MINW) void caar_np8_steps_kernel(const KernelArgs k0, int nsteps, int rotate) {
  __shared__ Np8Lds<NLEV, TPW, false, false, true, true> lds;
  if (element_of_block(k0, blockIdx.x) < 0) return;
  int n0 = k0.n0, np1 = k0.np1, nm1 = k0.nm1;
  Np8Carry<TPW> cy;  // handed from call to call
  const bool steady = rotate && n0 != np1 && n0 != nm1 && np1 != nm1;  // uniform
  auto rotate_levels = [&] {  // TestData::update_time_levels
    const int t = np1;
    np1 = nm1;
    nm1 = n0;
    n0 = t;
  };
  auto args = [&] {
    KernelArgs k = reload_args();
    k.n0 = n0;
    k.np1 = np1;
    k.nm1 = nm1;
    return k;
  };
  auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  if (steady) {
    caar_np8_element<NLEV, TPW, MINW, MOIST, SNT, false, false, false, false, true, LA, true, 0>(args(), lds, &cy, nsteps == 1, nsteps <= 3);
    for (int s = 1; s < nsteps; ++s) {
      rotate_levels();
      // (no barrier: the only LDS data a wave reads from other waves are the wave totals, and alternate calls use
      // alternate sets — see caar_np4_steps.hip)
      caar_np8_element<NLEV, TPW, MINW, MOIST, SNT, false, false, false, false, true, LA, true, 2>(args(), lds, &cy, s == nsteps - 1, s >= nsteps - 3, s & 1);
    }
  } else {
    for (int s = 0; s < nsteps; ++s) {
      caar_np8_element<NLEV, TPW, MINW, MOIST, SNT, false, false, false, false, true, LA, true, 0>(args(), lds, &cy, s == nsteps - 1);
      if (rotate) rotate_levels();
      lds_barrier();
    }
  }
}

template <int NLEV, int TPW, int MINW, bool SNT, int LA>
static hipError_t launch_np8_steps(const KernelArgs& k, int num_elems, int nsteps, int rotate, hipStream_t stream) {
  constexpr int THREADS = NLEV / TPW * 64;
  if (k.vadv) return hipErrorNotSupported;
  const int grid = k.per_xcd ? 8 * k.per_xcd : num_elems;
  if (k.qn0 >= 0) hipLaunchKernelGGL((caar_np8_steps_kernel<NLEV, TPW, MINW, true, SNT, LA>), dim3(grid), dim3(THREADS), 0, stream, k, nsteps, rotate);
  else hipLaunchKernelGGL((caar_np8_steps_kernel<NLEV, TPW, MINW, false, SNT, LA>), dim3(grid), dim3(THREADS), 0, stream, k, nsteps, rotate);
  return hipGetLastError();
}

template <int NLEV, int TPW, int MINW, bool NT, bool COEF_LDS = false, bool RELOAD_T = false, bool BATCH = false, bool MFMA = false, int LA = 1>
static hipError_t launch_np8(const KernelArgs& k, int num_elems, hipStream_t stream) {
  constexpr int THREADS = NLEV / TPW * 64;
  const int grid = k.per_xcd ? 8 * k.per_xcd : num_elems;
  if (k.vadv) {  // rsplit == 0: T stays in registers (no RELOAD_T form); every variant takes the MFMA contractions (the
                 // Eulerian form of the LDS-tile comparators spilled 6 VGPRs, and nothing compares Eulerian forms)
    if (k.qn0 >= 0)
      hipLaunchKernelGGL((caar_np8_kernel<NLEV, TPW, MINW, true, NT, false, false, false, true, true>), dim3(grid), dim3(THREADS), 0, stream, k);
    else
      hipLaunchKernelGGL((caar_np8_kernel<NLEV, TPW, MINW, false, NT, false, false, false, true, true>), dim3(grid), dim3(THREADS), 0, stream, k);
    return hipGetLastError();
  }
  if (k.qn0 >= 0)
    hipLaunchKernelGGL((caar_np8_kernel<NLEV, TPW, MINW, true, NT, COEF_LDS, RELOAD_T, BATCH, false, MFMA, LA>), dim3(grid), dim3(THREADS), 0, stream, k);
  else  // dry branch (P:128-139)
    hipLaunchKernelGGL((caar_np8_kernel<NLEV, TPW, MINW, false, NT, COEF_LDS, RELOAD_T, BATCH, false, MFMA, LA>), dim3(grid), dim3(THREADS), 0, stream, k);
  return hipGetLastError();
}

// (non-const on purpose, see caar_np4.hip)
KernelVariant kNp8Nlev72[] = {
    {"caar_np8_kernel<72, 9, 1, true, true, false, false, false, false, true, 2>", "8 waves x 9 levels, nt, MFMA contractions, update-phase inputs requested two levels ahead", launch_np8<72, 9, 1, true, false, false, false, true, 2>, true, launch_np8_steps<72, 9, 1, false, 2>},
    {"caar_np8_kernel<72, 9, 1, true, true, false, false, false, false, true, 1>", "8 waves x 9 levels, nt, Dvv contractions on v_mfma_f64_4x4x4 (lane = MFMA result layout, no LDS tile)", launch_np8<72, 9, 1, true, false, false, false, true>, false, launch_np8_steps<72, 9, 1, true, 1>},
    {"caar_np8_kernel<72, 9, 1, true, true, true, false, false, false, false, 1>", "8 waves x 9 levels, nt, Dvv slices re-read from LDS", launch_np8<72, 9, 1, true, true, false, false>},
    {"caar_np8_kernel<72, 9, 1, true, false, true, false, false, false, false, 1>", "8 waves x 9 levels, default cache policy", launch_np8<72, 9, 1, false, true, false, false>},
    {"caar_np8_kernel<72, 12, 1, true, true, false, false, false, false, true, 1>", "6 waves x 12 levels, nt, MFMA contractions", launch_np8<72, 12, 1, true, false, false, false, true>},
};
int kNp8Nlev72Count = sizeof(kNp8Nlev72) / sizeof(kNp8Nlev72[0]);

#ifdef CAAR_DEBUG
long long debug_dp3d_count_np8(int reset) { return debug_dp3d_count_of_this_tu(reset); }
#endif

}  // namespace caar
