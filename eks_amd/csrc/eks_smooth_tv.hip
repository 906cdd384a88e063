// gfx950 kernels of eks_smooth_tv on scalar chains (EKS_FLAG_DIAG_MODEL): eks_smooth with one process-noise scale
// per frame, x_t = a x_{t-1} + N(0, s w_t q) (formulas and index conventions in eks_smooth_tv_lane.hpp).  No
// reference counterpart.  The plain five-launch form:
//   T1 smooth_tv_summarize : lane = (chain, chunk of B frames): the chunk's filter element (reads y, var, w)
//   S1 kalman scan x3      : belief entering / information after every chunk - eks_chain.hip's chain_scan:
//                            composing, applying and pulling back elements never sees Q
//   T3 smooth_tv_replay    : lane = (chain, chunk): filter in registers, fuse, RTS backwards over them; ms and Vs
//                            stream out once, non-temporal (reads y, var, w)
// The B values of w a lane needs (those of the steps out of its frames) stay in registers for both passes of T3.
// The windowed replay of eks_smooth is never taken: its forgetting bound assumes a constant q.  General models:
// eks_dense.hip, dense_smooth_tv.
#include <hip/hip_runtime.h>

#include "eks_chain_plan.hpp"
#include "eks_internal.hpp"
#include "eks_smooth_tv_lane.hpp"

namespace eks {

template <int B, bool UNIT>
__global__ __launch_bounds__(256) void smooth_tv_summarize_kernel(ChainMap L, SampleWs W, DiagModel M, SmoothTvCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  smooth_tv_summarize_lane<B, UNIT>(W, M, c, n, j);
}

template <int B, bool UNIT, int VS_ROW>
__global__ __launch_bounds__(256) void smooth_tv_replay_kernel(ChainMap L, SampleWs W, DiagModel M, SmoothTvCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  smooth_tv_replay_lane<B, UNIT, VS_ROW>(W, M, c, n, j);
}

// shapes the scalar-chain form takes (EKS_OK) or the status it refuses them with; nothing here touches the device
int diag_smooth_tv_check(const eks_dims_t& d) {
  if (!(d.flags & EKS_FLAG_VS_DIAG) && d.state_dim > 8) return EKS_ERR_UNSUPPORTED;   // as diag_smooth
  return diag_chain_covers(d.n_frames, d.n_keypoints * d.state_dim) ? EKS_OK : EKS_ERR_SHAPE;
}

int diag_smooth_tv(const eks_dims_t& d, const float* y, const float* var, const float* qscale, int per_keypoint,
                   const DiagModel& M, float* ms, float* Vs, void* ws, size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, D = d.state_dim, N = d.n_keypoints * D;
  const int rc = diag_smooth_tv_check(d);
  if (rc != EKS_OK) return rc;
  if (ws_bytes < diag_em_workspace_bytes(T, N)) return EKS_ERR_WORKSPACE;
  const ChainPlan E = chain_plan(T, N, 0, true, ws);   // eks_em_stats' workspace; its float64 plane stays unused
  const dim3 grid(E.blocks), block(256);
  const SmoothTvCall c{y, var, qscale, ms, Vs, T, d.n_keypoints, per_keypoint ? 1 : 0};
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0;
  {
    ProfScope ps("smooth_tv_summarize", st);
    if (unit) hipLaunchKernelGGL((smooth_tv_summarize_kernel<kChainChunk, true>), grid, block, 0, st, E.L, E.W, M, c);
    else hipLaunchKernelGGL((smooth_tv_summarize_kernel<kChainChunk, false>), grid, block, 0, st, E.L, E.W, M, c);
  }
  const int rs = chain_scan(E, M, "em_scan", st);
  if (rs != EKS_OK) return rs;
  {
    ProfScope ps("smooth_tv_replay", st);
    const int vs_row = (d.flags & EKS_FLAG_VS_DIAG) ? 0 : D;
    with_vs_row(vs_row, [&](auto r) {
      constexpr int R = decltype(r)::value;
      if (unit) hipLaunchKernelGGL((smooth_tv_replay_kernel<kChainChunk, true, R>), grid, block, 0, st, E.L, E.W, M, c);
      else hipLaunchKernelGGL((smooth_tv_replay_kernel<kChainChunk, false, R>), grid, block, 0, st, E.L, E.W, M, c);
    });
  }
  return hip_status(hipGetLastError());
}

}  // namespace eks
