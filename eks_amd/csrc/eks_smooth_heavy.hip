// gfx950 kernels of eks_smooth_heavy on scalar chains (EKS_FLAG_DIAG_MODEL): the smoother under Student-t noise on
// observations AND process, by n_iters Gaussian smoothing passes with both closed-form updates between them (model,
// formulas and who writes what in eks_smooth_heavy_lane.hpp).  No reference counterpart.  A middle pass is six
// launches:
//   H1 heavy_summarize  : robust_summarize_lane's body on the keypoint's column of the scale plane (reads y, var, lam, w)
//   S1 kalman scan x3   : eks_chain.hip's chain_scan, as it is
//   H3 heavy_replay     : lane = (chain, chunk): filter in registers under r / lam and s q w, fuse, one RTS loop backwards
//                         with no output code: delta_{t,d} into the [T][N] contribution plane, lam_new in place
//                         (reads y, var, lam, w; writes lam, contrib)
//   J4 jumps_combine    : eks_smooth_jumps.hip's, as it is: the one launch that changes the scale plane
// The last pass is H1, the scan and a replay that streams ms, Vs out under both planes and updates nothing, so the
// planes returned are the ones the outputs were smoothed under.  All launches are enqueued back to back.  A call's
// first pass without input weights does not read the weight plane.  The windowed replay of eks_smooth is never taken.
// General models: eks_dense.hip, dense_smooth_heavy.
#include <hip/hip_runtime.h>

#include "eks_chain_plan.hpp"
#include "eks_internal.hpp"
#include "eks_smooth_heavy_lane.hpp"

namespace eks {

template <int B, bool UNIT, bool HAS_LAM>
__global__ __launch_bounds__(256) void heavy_summarize_kernel(ChainMap L, SampleWs W, DiagModel M, HeavyCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  heavy_summarize_lane<B, UNIT, HAS_LAM>(W, M, c, n, j);
}

template <int B, bool UNIT, bool HAS_LAM>
__global__ __launch_bounds__(256) void heavy_replay_kernel(ChainMap L, SampleWs W, DiagModel M, HeavyCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  heavy_replay_lane<B, UNIT, HAS_LAM>(W, M, c, n, j);
}

template <int B, bool UNIT, int VS_ROW, bool HAS_LAM>
__global__ __launch_bounds__(256) void heavy_last_kernel(ChainMap L, SampleWs W, DiagModel M, HeavyCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  heavy_last_lane<B, UNIT, VS_ROW, HAS_LAM>(W, M, c, n, j);
}

template <bool UNIT, bool HAS_LAM>
static void launch_heavy_last(int vs_row, const ChainPlan& E, const DiagModel& M, const HeavyCall& c, hipStream_t st) {
#define EKS_HEAVY_LAST(R)                                                                                          \
  case R:                                                                                                          \
    hipLaunchKernelGGL((heavy_last_kernel<kChainChunk, UNIT, R, HAS_LAM>), dim3(E.blocks), dim3(256), 0, st, E.L, E.W, \
                       M, c);                                                                                      \
    break;
  switch (vs_row) {
    EKS_HEAVY_LAST(0)
    EKS_HEAVY_LAST(1)
    EKS_HEAVY_LAST(2)
    EKS_HEAVY_LAST(3)
    EKS_HEAVY_LAST(4)
    EKS_HEAVY_LAST(5)
    EKS_HEAVY_LAST(6)
    EKS_HEAVY_LAST(7)
    EKS_HEAVY_LAST(8)
  }
#undef EKS_HEAVY_LAST
}

template <bool UNIT, bool HAS_LAM>
static int launch_heavy_pass(bool last, int vs_row, const ChainPlan& E, const DiagModel& M, const HeavyCall& c,
                             hipStream_t st) {
  const dim3 grid(E.blocks), block(256);
  {
    ProfScope ps("heavy_summarize", st);
    hipLaunchKernelGGL((heavy_summarize_kernel<kChainChunk, UNIT, HAS_LAM>), grid, block, 0, st, E.L, E.W, M, c);
  }
  const int rc = chain_scan(E, M, "heavy_scan", st);
  if (rc != EKS_OK) return rc;
  ProfScope ps("heavy_replay", st);
  if (last) launch_heavy_last<UNIT, HAS_LAM>(vs_row, E, M, c, st);
  else hipLaunchKernelGGL((heavy_replay_kernel<kChainChunk, UNIT, HAS_LAM>), grid, block, 0, st, E.L, E.W, M, c);
  return EKS_OK;
}

// eks_em_stats' workspace (its float64 plane stays unused), the [T][N] weight plane, the [T][K] scale plane and the
// [T][N] contribution plane; the first two are there whether or not the caller passes planes of their own
static size_t heavy_plane_bytes(int T, int N) { return align_up((size_t)T * (size_t)N * sizeof(float), 256); }
size_t diag_smooth_heavy_workspace_bytes(int T, int K, int D) {
  return align_up(diag_em_workspace_bytes(T, K * D), 256) + 2 * heavy_plane_bytes(T, K * D) + heavy_plane_bytes(T, K);
}

int diag_smooth_heavy(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, double nu_obs,
                      double nu_proc, int n_iters, float* weights, float* scales, int planes_in, float* change,
                      float* ms, float* Vs, void* ws, size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, K = d.n_keypoints, D = d.state_dim, N = K * D;
  int rc = diag_smooth_tv_check(d);
  if (rc != EKS_OK) return rc;
  if (ws_bytes < diag_smooth_heavy_workspace_bytes(T, K, D)) return EKS_ERR_WORKSPACE;
  const ChainPlan E = chain_plan(T, N, 0, true, ws);
  char* tail = static_cast<char*>(ws) + align_up(diag_em_workspace_bytes(T, N), 256);
  float* lam = weights ? weights : reinterpret_cast<float*>(tail);
  float* plane = scales ? scales : reinterpret_cast<float*>(tail + heavy_plane_bytes(T, N));
  float* contrib = reinterpret_cast<float*>(tail + heavy_plane_bytes(T, N) + heavy_plane_bytes(T, K));
  rc = jumps_init_plane(plane, T, K, planes_in & 2, nullptr, st);
  if (rc != EKS_OK) return rc;
  if (change) {
    const hipError_t e = hipMemsetAsync(change, 0, 2 * (size_t)K * sizeof(float), st);
    if (e != hipSuccess) return hip_status(e);
  }
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0;
  const int vs_row = (d.flags & EKS_FLAG_VS_DIAG) ? 0 : D;
  for (int it = 0; it < n_iters; ++it) {
    const bool last = it == n_iters - 1, has_lam = it > 0 || (planes_in & 1);
    // change: the last update of either plane is that of the pass before the last
    float* ch = it == n_iters - 2 ? change : nullptr;
    const HeavyCall c{y, var, lam, plane, contrib, ch, ms, Vs, T, K, (float)nu_obs, (float)(nu_obs + 1.0),
                      (float)((nu_obs + 1.0) / nu_obs)};
    if (unit) rc = has_lam ? launch_heavy_pass<true, true>(last, vs_row, E, M, c, st)
                           : launch_heavy_pass<true, false>(last, vs_row, E, M, c, st);
    else rc = has_lam ? launch_heavy_pass<false, true>(last, vs_row, E, M, c, st)
                      : launch_heavy_pass<false, false>(last, vs_row, E, M, c, st);
    if (rc != EKS_OK) return rc;
    if (!last) {
      rc = jumps_combine(contrib, false, D, plane, ch ? ch + K : nullptr, T, K, nu_proc, D, st);
      if (rc != EKS_OK) return rc;
    }
  }
  return hip_status(hipGetLastError());
}

}  // namespace eks
