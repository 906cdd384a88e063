// gfx950 kernels of eks_smooth_robust_group on scalar chains (EKS_FLAG_DIAG_MODEL): eks_smooth_robust with one
// Student-t weight per group of g consecutive coordinates of a keypoint (model, formulas and the race rule in
// eks_smooth_robust_group_lane.hpp).  No reference counterpart.  A middle pass is six launches:
//   G1 robust_group_summarize : eks_smooth_robust's summarize body, the weight read at [t][k][d / g]
//   S1 kalman scan x3         : eks_chain.hip's chain_scan, as it is
//   G3 robust_group_replay    : lane = (chain, chunk): filter in registers, fuse, RTS backwards, no output code; every
//                               frame stores delta_{t,d} into the [T][N] contribution plane (reads y, var, lam)
//   G4 robust_group_combine   : lane = (frame, keypoint, group): sums the g contributions in float64, writes lam into
//                               the weight plane - the one launch that changes it - and max-es |lam_new - lam_old|
//                               into change
// The last pass is a summarize, the scan and a replay that streams ms, Vs out under the plane.  All launches are
// enqueued back to back.  A call's first pass without input weights compiles without the weight loads.  The windowed
// replay of eks_smooth is never taken.  General models: eks_dense.hip, dense_smooth_robust_group.
#include <hip/hip_runtime.h>

#include "eks_chain_plan.hpp"
#include "eks_internal.hpp"
#include "eks_smooth_robust_group_lane.hpp"

namespace eks {

template <int B, bool UNIT, bool HAS_LAM>
__global__ __launch_bounds__(256) void robust_group_summarize_kernel(ChainMap L, SampleWs W, DiagModel M,
                                                                    RobustGroupCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  robust_group_summarize_lane<B, UNIT, HAS_LAM>(W, M, c, n, j);
}

template <int B, bool UNIT, int VS_ROW, bool HAS_LAM, bool LAST>
__global__ __launch_bounds__(256) void robust_group_replay_kernel(ChainMap L, SampleWs W, DiagModel M,
                                                                 RobustGroupCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  robust_group_replay_lane<B, UNIT, VS_ROW, HAS_LAM, LAST>(W, M, c, n, j);
}

// lane = (frame, column of the weight plane), columns along the wave: whole rows of the plane, g adjacent floats of
// the contribution row each.  K <= 64: the changes of a block meet in LDS before one atomic per keypoint and block
// reaches change[] (eks_smooth_jumps.hip: jumps_combine_kernel has the measurement); wider sessions go to change[]
// directly, behind robust_change_max's plain load.
__global__ __launch_bounds__(256) void robust_group_combine_kernel(const float* __restrict__ contrib, int g, float* lam,
                                                                  float* change, int T, int NG, int per_keypoint,
                                                                  int K, double nu, int has_lam) {
  __shared__ unsigned smax[64];
  const bool in_lds = change && K <= 64;   // uniform over the grid
  if (in_lds) {
    if (threadIdx.x < 64) smax[threadIdx.x] = 0u;
    __syncthreads();
  }
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < (long)T * NG) {
    const int q = (int)(idx % NG), k = q / per_keypoint;
    const float ch = robust_group_combine_lane(contrib, g, lam, NG, (int)(idx / NG), q, nu, has_lam);
    if (in_lds) atomicMax(&smax[k], __float_as_uint(ch));
    else if (change) robust_change_max(change + k, ch);
  }
  if (in_lds) {
    __syncthreads();
    if ((int)threadIdx.x < K && smax[threadIdx.x] != 0u)
      robust_change_max(change + threadIdx.x, __uint_as_float(smax[threadIdx.x]));
  }
}

template <bool UNIT, bool HAS_LAM>
static void launch_group_last(int vs_row, const ChainPlan& E, const DiagModel& M, const RobustGroupCall& c,
                              hipStream_t st) {
#define EKS_GROUP_REPLAY(R)                                                                                            \
  case R:                                                                                                              \
    hipLaunchKernelGGL((robust_group_replay_kernel<kChainChunk, UNIT, R, HAS_LAM, true>), dim3(E.blocks), dim3(256), 0, \
                       st, E.L, E.W, M, c);                                                                            \
    break;
  switch (vs_row) {
    EKS_GROUP_REPLAY(0)
    EKS_GROUP_REPLAY(1)
    EKS_GROUP_REPLAY(2)
    EKS_GROUP_REPLAY(3)
    EKS_GROUP_REPLAY(4)
    EKS_GROUP_REPLAY(5)
    EKS_GROUP_REPLAY(6)
    EKS_GROUP_REPLAY(7)
    EKS_GROUP_REPLAY(8)
  }
#undef EKS_GROUP_REPLAY
}

template <bool UNIT, bool HAS_LAM>
static int launch_group_pass(bool last, int vs_row, const ChainPlan& E, const DiagModel& M, const RobustGroupCall& c,
                             hipStream_t st) {
  const dim3 grid(E.blocks), block(256);
  {
    ProfScope ps("robust_group_summarize", st);
    hipLaunchKernelGGL((robust_group_summarize_kernel<kChainChunk, UNIT, HAS_LAM>), grid, block, 0, st, E.L, E.W, M, c);
  }
  const int rc = chain_scan(E, M, "robust_group_scan", st);
  if (rc != EKS_OK) return rc;
  ProfScope ps("robust_group_replay", st);
  if (last) launch_group_last<UNIT, HAS_LAM>(vs_row, E, M, c, st);
  else hipLaunchKernelGGL((robust_group_replay_kernel<kChainChunk, UNIT, 0, HAS_LAM, false>), grid, block, 0, st, E.L,
                          E.W, M, c);
  return EKS_OK;
}

// eks_em_stats' workspace (its float64 plane stays unused), the [T][N / g] weight plane, the [T] vector of ones and
// the [T][N] contribution plane
static size_t group_plane_bytes(int T, int N) { return align_up((size_t)T * (size_t)N * sizeof(float), 256); }
size_t diag_smooth_robust_group_workspace_bytes(int T, int N, int g) {
  return align_up(diag_em_workspace_bytes(T, N), 256) + group_plane_bytes(T, N / g) + group_plane_bytes(T, 1) +
         group_plane_bytes(T, N);
}

int diag_smooth_robust_group(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, double nu,
                             int g, int n_iters, float* weights, int weights_in, float* change, float* ms, float* Vs,
                             void* ws, size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, K = d.n_keypoints, D = d.state_dim, N = K * D, NG = N / g;
  int rc = diag_smooth_tv_check(d);
  if (rc != EKS_OK) return rc;
  if (ws_bytes < diag_smooth_robust_group_workspace_bytes(T, N, g)) return EKS_ERR_WORKSPACE;
  const ChainPlan E = chain_plan(T, N, 0, true, ws);
  char* tail = static_cast<char*>(ws) + align_up(diag_em_workspace_bytes(T, N), 256);
  float* lam = weights ? weights : reinterpret_cast<float*>(tail);
  float* ones = reinterpret_cast<float*>(tail + group_plane_bytes(T, NG));
  float* contrib = reinterpret_cast<float*>(tail + group_plane_bytes(T, NG) + group_plane_bytes(T, 1));
  {
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ones), 0x3f800000, (size_t)T, st);   // 1.0f
    // a single pass without input weights smooths under ones and returns them
    if (e == hipSuccess && n_iters == 1 && !weights_in)
      e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(lam), 0x3f800000, (size_t)T * (size_t)NG, st);
    if (e == hipSuccess && change) e = hipMemsetAsync(change, 0, (size_t)K * sizeof(float), st);
    if (e != hipSuccess) return hip_status(e);
  }
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0;
  const int vs_row = (d.flags & EKS_FLAG_VS_DIAG) ? 0 : D;
  const RobustGroupCall c{y, var, lam, contrib, ms, Vs, T, g, NG, ones};
  for (int it = 0; it < n_iters; ++it) {
    const bool last = it == n_iters - 1, has_lam = it > 0 || weights_in;
    if (unit) rc = has_lam ? launch_group_pass<true, true>(last, vs_row, E, M, c, st)
                           : launch_group_pass<true, false>(last, vs_row, E, M, c, st);
    else rc = has_lam ? launch_group_pass<false, true>(last, vs_row, E, M, c, st)
                      : launch_group_pass<false, false>(last, vs_row, E, M, c, st);
    if (rc != EKS_OK) return rc;
    if (last) break;
    const long lanes = (long)T * NG;
    ProfScope ps("robust_group_combine", st);
    // change: the last weight update is that of the pass before the last
    hipLaunchKernelGGL(robust_group_combine_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, contrib, g,
                       lam, it == n_iters - 2 ? change : nullptr, T, NG, D / g, K, nu, has_lam ? 1 : 0);
  }
  return hip_status(hipGetLastError());
}

}  // namespace eks
