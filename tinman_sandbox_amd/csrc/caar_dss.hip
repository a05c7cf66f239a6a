// caar_dss.hip — direct stiffness summation of the new time level (include/caar_dss.h), hand-written HIP for gfx950.
//
// HOMME's edgeVpack / bndry_exchangeV / edgeVunpack / rspheremp multiply (routine_extracted.F90:533-611) for the elements one
// device holds, as two kernels in stream order (stream order is what makes the packed rows visible across XCDs; there is
// no hand-off inside a launch and no atomic, so the result is deterministic):
//   caar_dss_pack<NP, F90>    copies the 4*(NP-1) boundary points of T, u, v, dp3d at tl into edge rows
//                             edge[ie][bp][4][nlev] (one row of 4*nlev doubles per boundary point: 2304 B at NLEV=72);
//   caar_dss_unpack<NP, F90>  sums, for every boundary point of its element, the rows of the point's sharers in the
//                             contract's order ((ie, a*NP+b) ascending, left to right), multiplies by rspheremp, and writes
//                             every point of the element back, interior points as rspheremp * x, in whole level slabs.
// Both kernels work on one element per 256-thread workgroup, as many levels at a time as 32 KiB of LDS hold, and turn the
// element's point-fastest level slabs into level-fastest rows (and back) through LDS, so that every global access of a wave is a
// contiguous run.  The sharer lists (sharers[ie*NB+bp][0..7]: edge-row numbers in the order of the sum, -1 after the last)
// are built once on the host by caar_dss_plan_create.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <new>
#include <utility>
#include <vector>

#include "../../include/caar_dss.h"

// the sums and the products are the contract's: no contraction into FMA, no reassociation
#pragma clang fp contract(off)

namespace caar {

constexpr int kDssThreads = 256;          // four waves
constexpr int kDssLdsBytes = 32768;       // LDS per workgroup: sets the levels per pass (NP=4: up to 85, NP=8: 36)

// Boundary point bp (0 .. 4*(NP-1)-1) <-> (a, b), numbered in ascending a*NP+b: the row a = 0, two points per inner row,
// the row a = NP-1.
__host__ __device__ constexpr int dss_bp_a(int np, int bp) {
  return bp < np ? 0 : (bp < np + 2 * (np - 2) ? 1 + (bp - np) / 2 : np - 1);
}
__host__ __device__ constexpr int dss_bp_b(int np, int bp) {
  return bp < np ? bp : (bp < np + 2 * (np - 2) ? (((bp - np) & 1) ? np - 1 : 0) : bp - np - 2 * (np - 2));
}
// -1 for an interior point
__host__ __device__ constexpr int dss_bp_of(int np, int a, int b) {
  return a == 0 ? b
                : (a == np - 1 ? np + 2 * (np - 2) + b
                               : (b == 0 ? np + 2 * (a - 1) : (b == np - 1 ? np + 2 * (a - 1) + 1 : -1)));
}

struct DssArgs {
  double* T;          // elem_state_T of element 0, time level tl
  double* v;          // elem_state_v ...
  double* dp;         // elem_state_dp3d ...
  const double* rsph; // rspheremp of element 0
  double* edge;       // [num_elems][NB][4][nlev]
  const int* sharers; // [num_elems*NB][CAAR_DSS_MAX_SHARERS]: edge rows ie*NB + bp of the sharers in the order of the sum,
                      // -1 after the last
  long long tstride;  // doubles per element of T / dp3d (timelevels*nlev*NP*NP); v: twice that
  int nlev;
  int num_elems;
  int kc;             // levels per pass
  int ldsw;           // doubles per boundary point in the LDS image: 4*kc + 1 (odd: rows spread over the banks)
};

// The state slab of level k of element e holds 4*NP*NP values: T (NP*NP), v (2*NP*NP), dp3d (NP*NP) in memory order.
// Slab index s -> (field f = 0 T, 1 u, 2 v, 3 dp3d; point a, b) and the address of that value.
// Workgroup b runs on XCD b % 8: element (b % 8) * per + b / 8, per = ceil(num_elems / 8), so that each XCD works through a
// contiguous range of elements and the neighbours whose rows an element gathers were packed and are read by the same XCD
// (its L2).  -1 for the at most 7 workgroups past the end.
__device__ inline long long dss_element(int num_elems) {
  const int per = (num_elems + 7) / 8;
  const long long e = (long long)(blockIdx.x % 8) * per + blockIdx.x / 8;
  return e < num_elems ? e : -1;
}

template <int NP, bool F90>
__device__ inline double* dss_slab_value(const DssArgs& g, long long e, int k, int s, int& f, int& a, int& b) {
  constexpr int PP = NP * NP;
  const long long lev = e * g.tstride + (long long)k * PP;
  if (s < PP || s >= 3 * PP) {
    const int o = s < PP ? s : s - 3 * PP;
    f = s < PP ? 0 : 3;
    a = F90 ? o % NP : o / NP;
    b = F90 ? o / NP : o % NP;
    return (s < PP ? g.T : g.dp) + lev + o;
  }
  const int o = s - PP;
  int c, q;
  if (F90) {  // (a, b, c): a fastest, u plane then v plane
    c = o / PP;
    q = o % PP;
    b = q / NP;
    a = q % NP;
  } else {    // [a][b][c]: (u, v) pairs
    c = o & 1;
    q = o >> 1;
    a = q / NP;
    b = q % NP;
  }
  f = 1 + c;
  return g.v + 2 * lev + o;
}

// Address of field f at point (a, b), level k, element e (pack: boundary points only).
template <int NP, bool F90>
__device__ inline const double* dss_point(const DssArgs& g, long long e, int k, int f, int a, int b) {
  constexpr int PP = NP * NP;
  const long long lev = e * g.tstride + (long long)k * PP;
  const int p = F90 ? b * NP + a : a * NP + b;
  if (f == 0) return g.T + lev + p;
  if (f == 3) return g.dp + lev + p;
  return g.v + 2 * lev + (F90 ? (f - 1) * PP + p : 2 * p + (f - 1));
}

// One element per workgroup.  The LDS image of a pass of kc levels holds, per boundary point bp, its 4*kc values in row
// order: lds[bp*ldsw + f*kc + kk].  (A) the boundary values, read point-fastest (the slab order); (B) wave w writes the
// rows of boundary points w, w+4, ..., its lanes along the row (one contiguous run of 4*nlev doubles when kc == nlev).
template <int NP, bool F90>
__global__ __launch_bounds__(kDssThreads) void caar_dss_pack(const DssArgs g) {
  constexpr int NB = 4 * (NP - 1);
  extern __shared__ double lds[];
  const long long e = dss_element(g.num_elems);
  if (e < 0) return;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row4 = 4 * g.nlev, ldsw = g.ldsw;
  double* erow = g.edge + e * NB * row4;
  for (int k0 = 0; k0 < g.nlev; k0 += g.kc) {
    const int kc = min(g.kc, g.nlev - k0), n = kc * 4 * NB, m = 4 * kc;
#pragma unroll 4
    for (int i = threadIdx.x; i < n; i += kDssThreads) {
      const int kk = i / (4 * NB), r = i % (4 * NB), f = r / NB, bp = r % NB;
      lds[bp * ldsw + f * kc + kk] = *dss_point<NP, F90>(g, e, k0 + kk, f, dss_bp_a(NP, bp), dss_bp_b(NP, bp));
    }
    __syncthreads();
    for (int bp = w; bp < NB; bp += 4)
      for (int t = lane; t < m; t += 64) {
        const int f = t / kc;
        erow[bp * row4 + f * g.nlev + k0 + (t - f * kc)] = lds[bp * ldsw + t];
      }
    __syncthreads();
  }
}

// One element per workgroup, the LDS image as in the pack.  (1) wave w sums the rows of boundary points w, w+4, ..., its
// lanes along the row, two values per lane with all their sharers' loads in flight: S = ((x0 + x1) + x2) + ..., times
// rspheremp; (2) every point of the kc level slabs in memory order, boundary points from LDS, interior points rspheremp * x
// (their loads issued before any store of the batch).
template <int NP, bool F90>
__global__ __launch_bounds__(kDssThreads) void caar_dss_unpack(const DssArgs g) {
  constexpr int NB = 4 * (NP - 1), PP = NP * NP, MS = CAAR_DSS_MAX_SHARERS, BATCH = 8;
  extern __shared__ double lds[];
  const long long e = dss_element(g.num_elems);
  if (e < 0) return;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row4 = 4 * g.nlev, ldsw = g.ldsw;
  const double* rsph = g.rsph + e * PP;  // [a][b] (C++) or (a,b) (Fortran): NP*NP doubles per element in both
  for (int k0 = 0; k0 < g.nlev; k0 += g.kc) {
    const int kc = min(g.kc, g.nlev - k0), m = 4 * kc;
    for (int bp = w; bp < NB; bp += 4) {
      const int* sh = g.sharers + (e * NB + bp) * MS;
      int row[MS];
#pragma unroll
      for (int j = 0; j < MS; ++j) row[j] = sh[j];
      const int a = dss_bp_a(NP, bp), b = dss_bp_b(NP, bp);
      const double r = rsph[F90 ? b * NP + a : a * NP + b];
      for (int t0 = lane; t0 < m; t0 += 128) {
        double x[2][MS];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int t = t0 + 64 * q, f = t / kc;
          const long long col = (long long)f * g.nlev + k0 + (t - f * kc);
#pragma unroll
          for (int j = 0; j < MS; ++j)
            if (t < m && row[j] >= 0) x[q][j] = g.edge[(long long)row[j] * row4 + col];
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int t = t0 + 64 * q;
          if (t < m) {
            double S = x[q][0];
#pragma unroll
            for (int j = 1; j < MS; ++j)
              if (row[j] >= 0) S = S + x[q][j];
            lds[bp * ldsw + t] = r * S;
          }
        }
      }
    }
    __syncthreads();
    const int n = kc * 4 * PP;
    for (int b0 = threadIdx.x; b0 < n; b0 += BATCH * kDssThreads) {
      double v[BATCH];
#pragma unroll
      for (int q = 0; q < BATCH; ++q) {
        const int i = b0 + q * kDssThreads, kk = i / (4 * PP), s = i % (4 * PP);
        int f, a, b;
        const double* p = dss_slab_value<NP, F90>(g, e, k0 + kk, s, f, a, b);
        if (i < n && dss_bp_of(NP, a, b) < 0) v[q] = *p;
      }
#pragma unroll
      for (int q = 0; q < BATCH; ++q) {
        const int i = b0 + q * kDssThreads, kk = i / (4 * PP), s = i % (4 * PP);
        int f, a, b;
        double* p = dss_slab_value<NP, F90>(g, e, k0 + kk, s, f, a, b);
        const int bp = dss_bp_of(NP, a, b);
        if (i < n) *p = bp >= 0 ? lds[bp * ldsw + f * kc + kk] : rsph[F90 ? b * NP + a : a * NP + b] * v[q];
      }
    }
    __syncthreads();
  }
}

template <int NP, bool F90>
static hipError_t launch_dss(const DssArgs& g, int num_elems, hipStream_t stream) {
  const int grid = 8 * ((num_elems + 7) / 8);
  const size_t lds = sizeof(double) * 4 * (NP - 1) * g.ldsw;
  hipLaunchKernelGGL((caar_dss_pack<NP, F90>), dim3(grid), dim3(kDssThreads), lds, stream, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((caar_dss_unpack<NP, F90>), dim3(grid), dim3(kDssThreads), lds, stream, g);
  return hipGetLastError();
}

}  // namespace caar

struct CaarDssPlan {
  int np, nlev, num_elems, layout, device;
  long long unique_points, shared_points, open_points;
  int max_sharers;
  int* rows_dev;
  double* edge_dev;
};

namespace {

// The host analysis: sharer lists, counts, open points.  Returns CAAR_OK or an error code.
int dss_analyse(CaarDssPlan* P, const long long* gdof, std::vector<int>& rows) {
  const int NP = P->np, PP = NP * NP, NB = 4 * (NP - 1);
  const long long NE = P->num_elems, npts = NE * PP;
  // logical ids g[ie*PP + a*NP + b]
  std::vector<long long> g((size_t)npts);
  for (long long e = 0; e < NE; ++e)
    for (int a = 0; a < NP; ++a)
      for (int b = 0; b < NP; ++b) {
        const long long id = gdof[e * PP + (P->layout == CAAR_DSS_LAYOUT_F90 ? b * NP + a : a * NP + b)];
        if (id < 0) return CAAR_EINVAL;
        g[(size_t)(e * PP + a * NP + b)] = id;
      }
  // points sorted by (id, ie*PP + a*NP + b): each id's sharers in the contract's order
  std::vector<int> order((size_t)npts);
  for (long long i = 0; i < npts; ++i) order[(size_t)i] = (int)i;
  std::sort(order.begin(), order.end(), [&](int x, int y) { return g[x] != g[y] ? g[x] < g[y] : x < y; });
  std::vector<int> group_of((size_t)npts), gstart;
  for (long long i = 0; i < npts; ++i) {
    if (i == 0 || g[order[(size_t)i]] != g[order[(size_t)i - 1]]) gstart.push_back((int)i);
    group_of[order[(size_t)i]] = (int)gstart.size() - 1;
  }
  const int ngroups = (int)gstart.size();
  gstart.push_back((int)npts);
  P->unique_points = ngroups;
  P->shared_points = 0;
  P->max_sharers = 0;
  for (int q = 0; q < ngroups; ++q) {
    const int n = gstart[q + 1] - gstart[q];
    P->max_sharers = std::max(P->max_sharers, n);
    if (n > 1) {
      ++P->shared_points;
      for (int j = gstart[q]; j < gstart[q + 1]; ++j) {
        const int p = order[j] % PP;
        if (caar::dss_bp_of(NP, p / NP, p % NP) < 0) return CAAR_EINVAL;  // an interior point shares its id
      }
    }
  }
  if (P->max_sharers > CAAR_DSS_MAX_SHARERS) return CAAR_EUNSUPPORTED;
  // sharer lists of every boundary point, as edge-row numbers, -1 after the last
  rows.assign((size_t)(NE * NB * CAAR_DSS_MAX_SHARERS), -1);
  for (long long e = 0; e < NE; ++e)
    for (int bp = 0; bp < NB; ++bp) {
      const int a = caar::dss_bp_a(NP, bp), b = caar::dss_bp_b(NP, bp);
      const int q = group_of[(size_t)(e * PP + a * NP + b)];
      for (int j = gstart[q]; j < gstart[q + 1]; ++j) {
        const int pt = order[j], p = pt % PP;
        rows[(size_t)((e * NB + bp) * CAAR_DSS_MAX_SHARERS + j - gstart[q])] = (pt / PP) * NB + caar::dss_bp_of(NP, p / NP, p % NP);
      }
    }
  // open points: ends of a boundary segment (two neighbouring points of one element edge, unordered) that only one
  // element of the plan has
  std::vector<std::pair<long long, long long>> seg;
  seg.reserve((size_t)(NE * NB));
  auto id = [&](long long e, int a, int b) { return g[(size_t)(e * PP + a * NP + b)]; };
  auto add = [&](long long x, long long y) { seg.emplace_back(std::min(x, y), std::max(x, y)); };
  for (long long e = 0; e < NE; ++e)
    for (int t = 0; t + 1 < NP; ++t) {
      add(id(e, 0, t), id(e, 0, t + 1));
      add(id(e, NP - 1, t), id(e, NP - 1, t + 1));
      add(id(e, t, 0), id(e, t + 1, 0));
      add(id(e, t, NP - 1), id(e, t + 1, NP - 1));
    }
  std::sort(seg.begin(), seg.end());
  std::vector<long long> open_ids;
  for (size_t i = 0; i < seg.size();) {
    size_t j = i + 1;
    while (j < seg.size() && seg[j] == seg[i]) ++j;
    if (j - i == 1) {
      open_ids.push_back(seg[i].first);
      open_ids.push_back(seg[i].second);
    }
    i = j;
  }
  std::sort(open_ids.begin(), open_ids.end());
  P->open_points = (long long)(std::unique(open_ids.begin(), open_ids.end()) - open_ids.begin());
  return CAAR_OK;
}

void dss_free_device(CaarDssPlan* P) {
  if (P->device < 0) return;
  int caller = -1;
  (void)hipGetDevice(&caller);
  (void)hipSetDevice(P->device);
  (void)hipDeviceSynchronize();
  if (P->rows_dev) (void)hipFree(P->rows_dev);
  if (P->edge_dev) (void)hipFree(P->edge_dev);
  P->rows_dev = nullptr;
  P->edge_dev = nullptr;
  if (caller >= 0 && caller != P->device) (void)hipSetDevice(caller);
}

}  // namespace

extern "C" {

int caar_dss_plan_create(CaarDssPlan** plan, const CaarDims* dims, const long long* gdof_host, int layout, int device) {
  if (!plan) return CAAR_EINVAL;
  *plan = nullptr;
  if (!dims || (dims->num_elems > 0 && !gdof_host)) return CAAR_EINVAL;
  if (layout != CAAR_DSS_LAYOUT_CXX && layout != CAAR_DSS_LAYOUT_F90) return CAAR_EINVAL;
  if (dims->num_elems < 0) return CAAR_EINVAL;
  if ((dims->np != 4 && dims->np != 8) || !caar_supported(dims->np, dims->nlev)) return CAAR_EUNSUPPORTED;
  const int NB = 4 * (dims->np - 1);
  // int row numbers and CSR offsets: at most NB*8 entries per element
  if ((long long)dims->num_elems * NB * CAAR_DSS_MAX_SHARERS >= INT_MAX) return CAAR_EINVAL;
  CaarDssPlan* P = new (std::nothrow) CaarDssPlan();
  if (!P) return CAAR_ENOMEM;
  P->np = dims->np;
  P->nlev = dims->nlev;
  P->num_elems = dims->num_elems;
  P->layout = layout;
  P->device = device < 0 ? -1 : device;
  std::vector<int> rows;
  int rc;
  try {
    rc = dss_analyse(P, gdof_host, rows);
  } catch (const std::bad_alloc&) {
    rc = CAAR_ENOMEM;
  }
  if (rc == CAAR_OK && P->device >= 0) {
    int caller = -1;
    hipError_t e = hipGetDevice(&caller);
    if (e == hipSuccess) e = hipSetDevice(P->device);
    const size_t edge_n = (size_t)P->num_elems * NB * 4 * P->nlev;
    if (e == hipSuccess) e = hipMalloc((void**)&P->rows_dev, sizeof(int) * std::max<size_t>(rows.size(), 1));
    if (e == hipSuccess) e = hipMalloc((void**)&P->edge_dev, sizeof(double) * std::max<size_t>(edge_n, 1));
    if (e == hipSuccess && !rows.empty())
      e = hipMemcpy(P->rows_dev, rows.data(), sizeof(int) * rows.size(), hipMemcpyHostToDevice);
    if (caller >= 0 && caller != P->device) (void)hipSetDevice(caller);
    if (e != hipSuccess) rc = e == hipErrorOutOfMemory ? CAAR_ENOMEM : (int)e;
  }
  if (rc != CAAR_OK) {
    dss_free_device(P);
    delete P;
    return rc;
  }
  *plan = P;
  return CAAR_OK;
}

void caar_dss_plan_destroy(CaarDssPlan* plan) {
  if (!plan) return;
  dss_free_device(plan);
  delete plan;
}

int caar_dss_plan_info(const CaarDssPlan* plan, long long* unique_points, long long* shared_points, long long* open_points,
                       int* max_sharers) {
  if (!plan) return CAAR_EINVAL;
  if (unique_points) *unique_points = plan->unique_points;
  if (shared_points) *shared_points = plan->shared_points;
  if (open_points) *open_points = plan->open_points;
  if (max_sharers) *max_sharers = plan->max_sharers;
  return CAAR_OK;
}

int caar_dss_launch(const CaarDssPlan* plan, const CaarDims* dims, int layout, const CaarArrays* arrays_dev, int tl,
                    const double* rspheremp_dev, void* stream) {
  if (!plan || !dims || !arrays_dev || !rspheremp_dev) return CAAR_EINVAL;
  if (dims->np != plan->np || dims->nlev != plan->nlev || dims->num_elems != plan->num_elems || dims->timelevels < 1)
    return CAAR_EINVAL;
  if (layout != plan->layout || tl < 0 || tl >= dims->timelevels) return CAAR_EINVAL;
  double* T = arrays_dev->elem_state_T;
  double* v = arrays_dev->elem_state_v;
  double* dp = arrays_dev->elem_state_dp3d;
  if (!T || !v || !dp) return CAAR_EINVAL;
  if (((size_t)T | (size_t)v | (size_t)dp | (size_t)rspheremp_dev) & 7) return CAAR_EINVAL;
  if (plan->device < 0) return CAAR_ENODEVICE;
  if (plan->num_elems == 0) return CAAR_OK;
  const long long pp = (long long)plan->np * plan->np, lev = (long long)plan->nlev * pp;
  caar::DssArgs g;
  g.T = T + tl * lev;
  g.v = v + 2 * tl * lev;
  g.dp = dp + tl * lev;
  g.rsph = rspheremp_dev;
  g.edge = plan->edge_dev;
  g.sharers = plan->rows_dev;
  g.tstride = (long long)dims->timelevels * lev;
  g.nlev = plan->nlev;
  g.num_elems = plan->num_elems;
  // as many levels per pass as kDssLdsBytes hold, in equal passes: NP=4 NLEV 72 in one pass, 128 in 2 x 64; NP=8 72 in 2 x 36
  const int nb = 4 * (plan->np - 1), kc_max = (caar::kDssLdsBytes / (8 * nb) - 1) / 4;
  const int passes = (plan->nlev + kc_max - 1) / kc_max;
  g.kc = (plan->nlev + passes - 1) / passes;
  g.ldsw = 4 * g.kc + 1;
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  if (plan->np == 4)
    e = plan->layout == CAAR_DSS_LAYOUT_F90 ? caar::launch_dss<4, true>(g, plan->num_elems, s)
                                            : caar::launch_dss<4, false>(g, plan->num_elems, s);
  else
    e = plan->layout == CAAR_DSS_LAYOUT_F90 ? caar::launch_dss<8, true>(g, plan->num_elems, s)
                                            : caar::launch_dss<8, false>(g, plan->num_elems, s);
  return (int)e;
}

}  // extern "C"
