// gfx950 kernels of eks_smooth_jumps on scalar chains (EKS_FLAG_DIAG_MODEL): the smoother under Student-t process
// noise, one scale per keypoint and frame, by n_iters Gaussian smoothing passes under eks_smooth_tv's per-keypoint
// qscale with a closed-form scale update between them (model, formulas and the race argument in
// eks_smooth_jumps_lane.hpp).  No reference counterpart.  A middle pass is six launches:
//   J1 jumps_summarize  : eks_smooth_tv's summarize body on the scale plane (reads y, var, w)
//   S1 kalman scan x3   : eks_chain.hip's chain_scan, as it is
//   J3 jumps_replay     : lane = (chain, chunk): filter in registers, fuse, RTS backwards, no output code; every step
//                         stores delta_{t,d} into the [T][N] contribution plane (reads y, var, w)
//   J4 jumps_combine    : lane = (frame, keypoint): sums the D contributions, writes the new w into the scale plane -
//                         the one launch that changes it - and max-es |u_new - u_old| into change
// The last pass is eks_smooth_tv itself on the plane (diag_smooth_tv: five launches), so the scales returned are the
// ones ms, Vs were smoothed under, bit for bit.  All launches are enqueued back to back.  The windowed replay of
// eks_smooth is never taken.  The combine kernel also serves general models (eks_dense.hip, dense_smooth_jumps) with
// one float64 contribution per keypoint.
#include <hip/hip_runtime.h>

#include "eks_chain_plan.hpp"
#include "eks_internal.hpp"
#include "eks_smooth_jumps_lane.hpp"

namespace eks {

template <int B, bool UNIT>
__global__ __launch_bounds__(256) void jumps_summarize_kernel(ChainMap L, SampleWs W, DiagModel M, SmoothTvCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  smooth_tv_summarize_lane<B, UNIT>(W, M, c, n, j);
}

template <int B, bool UNIT>
__global__ __launch_bounds__(256) void jumps_replay_kernel(ChainMap L, SampleWs W, DiagModel M, JumpsCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  jumps_replay_lane<B, UNIT>(W, M, c, n, j);
}

// lane = (frame 1 .. T-1, keypoint), keypoints along the wave: whole rows of the scale plane.  K <= 64: a block holds
// at least four frames of every keypoint, and their changes meet in LDS before one atomic per keypoint and block
// reaches change[] (K = 4: 64 times fewer; the first launch's atomics, all against a zero, cost 0.33 ms of a 1.6 ms call
// without it).  Wider sessions have few frames of a keypoint per block and gain nothing from it (K = 256: 0.127 ms per
// launch either way), so their lanes go to change[] directly, behind robust_change_max's plain load.
template <typename C>
__global__ __launch_bounds__(256) void jumps_combine_kernel(const C* __restrict__ contrib, int nd, float* scales,
                                                           float* change, int T, int K, double nu, double nu_d) {
  __shared__ unsigned smax[256];
  const bool in_lds = change && K <= 64;   // uniform over the grid
  if (in_lds) {
    smax[threadIdx.x] = 0u;
    __syncthreads();
  }
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < (long)(T - 1) * K) {
    const int k = (int)(idx % K);
    const float ch = jumps_combine_lane<C>(contrib, nd, scales, K, (int)(idx / K) + 1, k, nu, nu_d);
    if (in_lds) atomicMax(&smax[k], __float_as_uint(ch));
    else if (change) robust_change_max(change + k, ch);
  }
  if (in_lds) {
    __syncthreads();
    if ((int)threadIdx.x < K && smax[threadIdx.x] != 0u)
      robust_change_max(change + threadIdx.x, __uint_as_float(smax[threadIdx.x]));
  }
}

int jumps_combine(const void* contrib, bool f64, int nd, float* scales, float* change, int T, int K, double nu,
                  int D, hipStream_t st) {
  if (T < 2) return EKS_OK;
  const long lanes = (long)(T - 1) * K;
  const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
  ProfScope ps("jumps_combine", st);
  if (f64)
    hipLaunchKernelGGL(jumps_combine_kernel<double>, grid, block, 0, st, static_cast<const double*>(contrib), nd, scales,
                       change, T, K, nu, nu + (double)D);
  else
    hipLaunchKernelGGL(jumps_combine_kernel<float>, grid, block, 0, st, static_cast<const float*>(contrib), nd, scales,
                       change, T, K, nu, nu + (double)D);
  return hip_status(hipGetLastError());
}

// the scale plane a call works on: ones everywhere, or (scales_in) the caller's values with row 0 set to 1
int jumps_init_plane(float* plane, int T, int K, int scales_in, float* change, hipStream_t st) {
  const size_t n = scales_in ? (size_t)K : (size_t)T * (size_t)K;
  hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(plane), 0x3f800000, n, st);   // 1.0f
  if (e == hipSuccess && change) e = hipMemsetAsync(change, 0, (size_t)K * sizeof(float), st);
  return hip_status(e);
}

// eks_em_stats' workspace (its float64 plane stays unused), the [T][K] scale plane and the [T][N] contribution plane
static size_t jumps_plane_bytes(int T, int N) { return align_up((size_t)T * (size_t)N * sizeof(float), 256); }
size_t diag_smooth_jumps_workspace_bytes(int T, int K, int D) {
  return align_up(diag_em_workspace_bytes(T, K * D), 256) + jumps_plane_bytes(T, K) + jumps_plane_bytes(T, K * D);
}

int diag_smooth_jumps(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, double nu, int n_iters,
                      float* scales, int scales_in, float* change, float* ms, float* Vs, void* ws, size_t ws_bytes,
                      hipStream_t st) {
  const int T = d.n_frames, K = d.n_keypoints, D = d.state_dim, N = K * D;
  int rc = diag_smooth_tv_check(d);
  if (rc != EKS_OK) return rc;
  if (ws_bytes < diag_smooth_jumps_workspace_bytes(T, K, D)) return EKS_ERR_WORKSPACE;
  const ChainPlan E = chain_plan(T, N, 0, true, ws);
  char* tail = static_cast<char*>(ws) + align_up(diag_em_workspace_bytes(T, N), 256);
  float* plane = scales ? scales : reinterpret_cast<float*>(tail);
  float* contrib = reinterpret_cast<float*>(tail + jumps_plane_bytes(T, K));
  rc = jumps_init_plane(plane, T, K, scales_in, change, st);
  if (rc != EKS_OK) return rc;
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0;
  const dim3 grid(E.blocks), block(256);
  const SmoothTvCall tv{y, var, plane, nullptr, nullptr, T, K, 1};
  const JumpsCall c{y, var, plane, contrib, T, K};
  for (int it = 0; it + 1 < n_iters; ++it) {
    {
      ProfScope ps("jumps_summarize", st);
      if (unit) hipLaunchKernelGGL((jumps_summarize_kernel<kChainChunk, true>), grid, block, 0, st, E.L, E.W, M, tv);
      else hipLaunchKernelGGL((jumps_summarize_kernel<kChainChunk, false>), grid, block, 0, st, E.L, E.W, M, tv);
    }
    rc = chain_scan(E, M, "jumps_scan", st);
    if (rc != EKS_OK) return rc;
    {
      ProfScope ps("jumps_replay", st);
      if (unit) hipLaunchKernelGGL((jumps_replay_kernel<kChainChunk, true>), grid, block, 0, st, E.L, E.W, M, c);
      else hipLaunchKernelGGL((jumps_replay_kernel<kChainChunk, false>), grid, block, 0, st, E.L, E.W, M, c);
    }
    // change: the last scale update is that of the pass before the last
    rc = jumps_combine(contrib, false, D, plane, it == n_iters - 2 ? change : nullptr, T, K, nu, D, st);
    if (rc != EKS_OK) return rc;
  }
  return diag_smooth_tv(d, y, var, plane, 1, M, ms, Vs, ws, ws_bytes, st);
}

}  // namespace eks
