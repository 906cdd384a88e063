// gfx950 kernel of eks_smooth_heavy_fit's M-step for the smoothing parameter: the fixed-order float64 reduction of
// S_k = sum_t u_t delta_t over the planes a middle pass of eks_smooth_heavy leaves behind, and the step on s[k]
// (model, order of the sum and conventions: eks_smooth_heavy_fit_lane.hpp).  No reference counterpart.  ONE launch of
// its own behind the combine launch; jumps_combine_kernel and the replays are not touched:
//   heavy_fit : block = (slab of kFitSlab rows, tile of KT keypoints), keypoints along the wave.  A lane adds the
//               kFitSub rows of a sub-slab in order (256 / KT lanes of a keypoint share its kFitSubs sub-slabs), the sums
//               meet in LDS and the tile's first KT lanes add each keypoint's in order into part[slab][k].  KT is 4 or
//               16 by K - narrow sessions keep their lanes busy - and moves no sum: a keypoint's order is a function of
//               t alone.  The block that takes the LAST ticket of its tile (an integer counter per tile; nobody waits
//               for anybody, so no co-residency is assumed) gathers the tile's slab sums, a round at a time, in LDS; the
//               first lane of each keypoint adds them in order and makes the step.  s[k] and dlog[k] are written there
//               only.  Which block comes last changes nothing: it reads every slab's sum, its own included, from
//               part[] and adds them in slab order.
// The tickets count modulo the slabs, so a launch leaves them a multiple of the slab count and the next one needs no
// reset; heavy_fit_begin zeroes them once a call (a workspace arrives with anything in it).
// s is the device vector every pass reads at its start, so the next pass smooths under the new value with no host
// round trip.  Templated on the contribution type as jumps_combine_kernel is.
#include <hip/hip_runtime.h>

#include "eks_internal.hpp"
#include "eks_smooth_heavy_fit_lane.hpp"

namespace eks {

// Publication of a block's slab sums to blocks on other XCDs: eks_diag_nll.hip's scheme (gf_publish, measured there) -
// agent-scope atomic stores (gfx950: written through the XCD's L2), acknowledged (vmcnt(0)) before the wave takes its
// ticket, and an agent-scope acquire fence in the block that reads.  A release fence at agent scope would walk the whole
// L2 (5 us a block there).  The ordering argument is about gfx950's caches, not the HIP memory model: hence the guard.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "heavy_fit_kernel relies on gfx950's write-through sc1 stores: use a release at agent scope on the ticket for other targets"
#endif

template <typename C, int ND>
__global__ __launch_bounds__(256) void heavy_fit_kernel(const C* __restrict__ contrib, int nd,
                                                       const float* __restrict__ scales, int T, int K, int kt_log2,
                                                       int k_tiles, int n_slabs, double* part, int32_t* tickets,
                                                       double n, double lo, double hi, double* s, float* dlog) {
  __shared__ double subs[kFitSubs * 16];
  __shared__ int last_flag;
  const int KT = 1 << kt_log2, SL = 256 >> kt_log2;
  const int kl = threadIdx.x & (KT - 1), sl = threadIdx.x >> kt_log2;
  const int slab = blockIdx.x / k_tiles, tile = blockIdx.x % k_tiles;
  const int k = tile * KT + kl;
  const long row0 = 1 + (long)slab * kFitSlab;
  if (k < K)
    for (int sub = sl; sub < kFitSubs; sub += SL)
      subs[sub * KT + kl] = heavy_fit_sub_lane<C, ND>(contrib, nd, scales, K, T, k, row0 + (long)sub * kFitSub);
  __syncthreads();
  if ((int)threadIdx.x < KT) {   // KT <= 16: lanes of wave 0
    if (k < K)
      __hip_atomic_store(part + (size_t)slab * (size_t)K + (unsigned)k, heavy_fit_slab_lane(subs + kl, KT),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);
    if (threadIdx.x == 0) last_flag = (atomicAdd(tickets + tile, 1) + 1) % n_slabs == 0;
  }
  __syncthreads();
  if (!last_flag) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the other blocks' slab sums
  // ---- the tile's last block: 256 / KT lanes per keypoint fetch a round of 1024 / KT slab sums (four independent loads
  // a lane), the keypoint's first lane adds the round in order
  const int round = (kFitSubs * 16) >> kt_log2;
  double S = 0.0;
  for (int j0 = 0; j0 < n_slabs; j0 += round) {
    double v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + c * SL + sl;
      v[c] = k < K && j < n_slabs ? part[(size_t)j * (size_t)K + (unsigned)k] : 0.0;
    }
    __syncthreads();   // subs: the sub-slab sums, or the round before, have been read
#pragma unroll
    for (int c = 0; c < 4; ++c) subs[(c * SL + sl) * KT + kl] = v[c];
    __syncthreads();
    if (sl == 0) S = heavy_fit_sum_lane(S, subs + kl, n_slabs - j0 < round ? n_slabs - j0 : round, KT);
  }
  if (sl == 0 && k < K) heavy_fit_apply_lane(S, k, n, lo, hi, s, dlog);
}

static int heavy_fit_kt_log2(int K) { return K <= 4 ? 2 : 4; }
static int heavy_fit_tiles(int K) {
  const int l = heavy_fit_kt_log2(K);
  return (K + (1 << l) - 1) >> l;
}

// the fit's own region of a workspace: [slabs][K] partial sums, then one ticket per keypoint tile, each on 256 bytes
static size_t heavy_fit_part_only_bytes(int T, int K) {
  return align_up((size_t)heavy_fit_slabs(T) * (size_t)K * sizeof(double), 256);
}
size_t heavy_fit_part_bytes(int T, int K) {
  return heavy_fit_part_only_bytes(T, K) + align_up((size_t)heavy_fit_tiles(K) * sizeof(int32_t), 256);
}

int heavy_fit_begin(void* fit_ws, int T, int K, hipStream_t st) {
  return hip_status(hipMemsetAsync(static_cast<char*>(fit_ws) + heavy_fit_part_only_bytes(T, K), 0,
                                   (size_t)heavy_fit_tiles(K) * sizeof(int32_t), st));
}

template <typename C, int ND>
static void launch_fit(dim3 grid, hipStream_t st, const void* contrib, int nd, const float* scales, int T, int K,
                       int n_slabs, double* part, int32_t* tickets, double n, double lo, double hi, double* s,
                       float* dlog) {
  hipLaunchKernelGGL((heavy_fit_kernel<C, ND>), grid, dim3(256), 0, st, static_cast<const C*>(contrib), nd, scales, T, K,
                     heavy_fit_kt_log2(K), heavy_fit_tiles(K), n_slabs, part, tickets, n, lo, hi, s, dlog);
}

int heavy_fit_step(const void* contrib, bool f64, int nd, const float* scales, int T, int K, int D, double lo,
                   double hi, void* fit_ws, double* s, float* dlog, hipStream_t st) {
  if (T < 2) return EKS_OK;
  const int n_slabs = heavy_fit_slabs(T);
  double* part = static_cast<double*>(fit_ws);
  int32_t* tickets = reinterpret_cast<int32_t*>(static_cast<char*>(fit_ws) + heavy_fit_part_only_bytes(T, K));
  const dim3 grid((unsigned)((long)n_slabs * heavy_fit_tiles(K)));
  const double n = (double)D * (double)(T - 1);
  ProfScope ps("heavy_fit", st);
  // nd at compile time where the sessions have it (the inner loop unrolls); the run-time form serves D > 3
  if (f64) launch_fit<double, 1>(grid, st, contrib, 1, scales, T, K, n_slabs, part, tickets, n, lo, hi, s, dlog);
  else if (nd == 1) launch_fit<float, 1>(grid, st, contrib, nd, scales, T, K, n_slabs, part, tickets, n, lo, hi, s, dlog);
  else if (nd == 2) launch_fit<float, 2>(grid, st, contrib, nd, scales, T, K, n_slabs, part, tickets, n, lo, hi, s, dlog);
  else if (nd == 3) launch_fit<float, 3>(grid, st, contrib, nd, scales, T, K, n_slabs, part, tickets, n, lo, hi, s, dlog);
  else launch_fit<float, 0>(grid, st, contrib, nd, scales, T, K, n_slabs, part, tickets, n, lo, hi, s, dlog);
  return hip_status(hipGetLastError());
}

}  // namespace eks
