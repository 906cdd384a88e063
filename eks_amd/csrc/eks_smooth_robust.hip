// gfx950 kernels of eks_smooth_robust on scalar chains (EKS_FLAG_DIAG_MODEL): the smoother under Student-t observation
// noise, by n_iters Gaussian smoothing passes under reweighted variances with a closed-form weight update between them
// (model, formulas and the in-place argument in eks_smooth_robust_lane.hpp).  No reference counterpart.  Every pass is
// the five-launch form of eks_smooth_tv:
//   R1 robust_summarize : lane = (chain, chunk of B frames): the chunk's filter element under r / lam (reads y, var, lam)
//   S1 kalman scan x3   : eks_chain.hip's chain_scan, as it is
//   R3 robust_replay    : lane = (chain, chunk): filter in registers, fuse, RTS backwards; a middle pass forms delta and
//                         stores the new weights in place (reads y, var, lam; writes lam), the last pass streams ms and
//                         Vs out instead (no weight update: the weights returned are those ms, Vs were smoothed under)
// All n_iters x 5 launches are enqueued back to back; nothing comes back to the host between passes.  A call's first
// pass without input weights does not read the plane.  The frames run eks_smooth_tv's bodies at w = 1, read from a
// [T] vector of ones in the workspace (eks_smooth_robust_lane.hpp says why).  The windowed replay of eks_smooth is never taken.  General
// models: eks_dense.hip, dense_smooth_robust.
#include <hip/hip_runtime.h>

#include "eks_chain_plan.hpp"
#include "eks_internal.hpp"
#include "eks_smooth_robust_lane.hpp"

namespace eks {

// y and r of the chunk stay in registers for the weight update (-DEKS_ROBUST_RELOAD: the A/B build that loads them
// again in the backward pass; DESIGN.md 9i has both register counts and the reason for the choice)
#ifdef EKS_ROBUST_RELOAD
constexpr bool kRobustKeep = false;
#else
constexpr bool kRobustKeep = true;
#endif

template <int B, bool UNIT, bool HAS_LAM>
__global__ __launch_bounds__(256) void robust_summarize_kernel(ChainMap L, SampleWs W, DiagModel M, RobustCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  robust_summarize_lane<B, UNIT, HAS_LAM>(W, M, c, n, j);
}

template <int B, bool UNIT, int VS_ROW, bool HAS_LAM, bool LAST>
__global__ __launch_bounds__(256) void robust_replay_kernel(ChainMap L, SampleWs W, DiagModel M, RobustCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  robust_replay_lane<B, UNIT, VS_ROW, HAS_LAM, LAST, kRobustKeep>(W, M, c, n, j);
}

template <bool UNIT, bool HAS_LAM>
static void launch_robust_last(int vs_row, const ChainPlan& E, const DiagModel& M, const RobustCall& c, hipStream_t st) {
#define EKS_ROBUST_REPLAY(R)                                                                                     \
  case R:                                                                                                        \
    hipLaunchKernelGGL((robust_replay_kernel<kChainChunk, UNIT, R, HAS_LAM, true>), dim3(E.blocks), dim3(256), 0, st, \
                       E.L, E.W, M, c);                                                                          \
    break;
  switch (vs_row) {
    EKS_ROBUST_REPLAY(0)
    EKS_ROBUST_REPLAY(1)
    EKS_ROBUST_REPLAY(2)
    EKS_ROBUST_REPLAY(3)
    EKS_ROBUST_REPLAY(4)
    EKS_ROBUST_REPLAY(5)
    EKS_ROBUST_REPLAY(6)
    EKS_ROBUST_REPLAY(7)
    EKS_ROBUST_REPLAY(8)
  }
#undef EKS_ROBUST_REPLAY
}

template <bool UNIT, bool HAS_LAM>
static void launch_robust_pass(bool last, int vs_row, const ChainPlan& E, const DiagModel& M, const RobustCall& c,
                               hipStream_t st) {
  const dim3 grid(E.blocks), block(256);
  {
    ProfScope ps("robust_summarize", st);
    hipLaunchKernelGGL((robust_summarize_kernel<kChainChunk, UNIT, HAS_LAM>), grid, block, 0, st, E.L, E.W, M, c);
  }
  chain_scan(E, M, "robust_scan", st);
  ProfScope ps("robust_replay", st);
  if (last) launch_robust_last<UNIT, HAS_LAM>(vs_row, E, M, c, st);
  else hipLaunchKernelGGL((robust_replay_kernel<kChainChunk, UNIT, 0, HAS_LAM, false>), grid, block, 0, st, E.L, E.W, M, c);
}

// eks_em_stats' workspace (its float64 plane stays unused), one [T][N] plane of weights and the [T] vector of ones
static size_t robust_plane_bytes(int T, int N) { return align_up((size_t)T * (size_t)N * sizeof(float), 256); }
size_t diag_smooth_robust_workspace_bytes(int T, int N) {
  return align_up(diag_em_workspace_bytes(T, N), 256) + robust_plane_bytes(T, N) + robust_plane_bytes(T, 1);
}

int diag_smooth_robust(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, double nu, int n_iters,
                       float* weights, int weights_in, float* change, float* ms, float* Vs, void* ws, size_t ws_bytes,
                       hipStream_t st) {
  const int T = d.n_frames, D = d.state_dim, N = d.n_keypoints * D;
  const int rc = diag_smooth_tv_check(d);
  if (rc != EKS_OK) return rc;
  if (ws_bytes < diag_smooth_robust_workspace_bytes(T, N)) return EKS_ERR_WORKSPACE;
  const ChainPlan E = chain_plan(T, N, 0, true, ws);
  char* tail = static_cast<char*>(ws) + align_up(diag_em_workspace_bytes(T, N), 256);
  float* lam = weights ? weights : reinterpret_cast<float*>(tail);
  float* ones = reinterpret_cast<float*>(tail + robust_plane_bytes(T, N));
  {
    const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ones), 0x3f800000, (size_t)T, st);   // 1.0f
    if (e != hipSuccess) return hip_status(e);
  }
  if (change) {
    const hipError_t e = hipMemsetAsync(change, 0, (size_t)d.n_keypoints * sizeof(float), st);
    if (e != hipSuccess) return hip_status(e);
  }
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0;
  const int vs_row = (d.flags & EKS_FLAG_VS_DIAG) ? 0 : D;
  for (int it = 0; it < n_iters; ++it) {
    const bool last = it == n_iters - 1, has_lam = it > 0 || weights_in;
    // change: the last weight update is that of the pass before the last
    const RobustCall c{y, var, lam, it == n_iters - 2 ? change : nullptr, ms, Vs, T, (float)nu, (float)(nu + 1.0),
                       (float)((nu + 1.0) / nu), ones};
    if (unit) {
      if (has_lam) launch_robust_pass<true, true>(last, vs_row, E, M, c, st);
      else launch_robust_pass<true, false>(last, vs_row, E, M, c, st);
    } else {
      if (has_lam) launch_robust_pass<false, true>(last, vs_row, E, M, c, st);
      else launch_robust_pass<false, false>(last, vs_row, E, M, c, st);
    }
  }
  return hip_status(hipGetLastError());
}

}  // namespace eks
