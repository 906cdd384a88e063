// gfx950 kernels of eks_smooth_increments on scalar chains (EKS_FLAG_DIAG_MODEL): eks_smooth plus the posterior of
// the frame-to-frame increment (lag1, dmean, dV; formulas in eks_increments_lane.hpp).  No reference counterpart.
//   I1 summarize            : lane = (chain, chunk of B frames): the chunk's filter element (reads y, var)  } eks_chain.hip,
//   S1 kalman scan x3       : belief entering / information after every chunk (grouped, lanes along chains) } chain_forward
//   I2 increments_replay    : lane = (chain, chunk): filter in registers, fuse, RTS backwards; the five outputs stream
//                             out once, 256-byte rows per wave, non-temporal (reads y, var)
// y and var are read twice, every requested output is written once.  General models: eks_dense.hip, dense_increments.
#include <hip/hip_runtime.h>

#include "eks_chain_plan.hpp"
#include "eks_increments_lane.hpp"
#include "eks_internal.hpp"

namespace eks {

template <int B, bool UNIT, bool ALL>
__global__ __launch_bounds__(256) void increments_replay_kernel(ChainMap L, SampleWs W, DiagModel M, IncrementsCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  increments_replay_lane<B, UNIT, ALL>(W, M, c, n, j);
}

// ------------------------------------------------------------------------------------------------------------------
size_t diag_increments_workspace_bytes(int T, int N) { return chain_workspace_bytes(T, N, 0, false); }

int diag_increments(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, float* ms, float* Vs,
                    float* lag1, float* dmean, float* dV, void* ws, size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, N = d.n_keypoints * d.state_dim;
  if (!diag_chain_covers(T, N)) return EKS_ERR_SHAPE;
  if (ws_bytes < diag_increments_workspace_bytes(T, N)) return EKS_ERR_WORKSPACE;
  const ChainPlan P = chain_plan(T, N, 0, false, ws);
  const dim3 grid(P.blocks), block(256);
  const SampleCall cs{y, var, nullptr, nullptr, nullptr, T, 0u, 0u, 0u, 0u};
  const IncrementsCall c{y, var, ms, Vs, lag1, dmean, dV, T};
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0;
  const bool all = ms && Vs && lag1 && dmean && dV;
  constexpr int B = kChainChunk;

  const int rc = chain_forward(P, M, cs, unit, "increments_summarize", "increments_scan", st);
  if (rc != EKS_OK) return rc;
  {
    ProfScope ps("increments_replay", st);
    if (unit && all) hipLaunchKernelGGL((increments_replay_kernel<B, true, true>), grid, block, 0, st, P.L, P.W, M, c);
    else if (unit) hipLaunchKernelGGL((increments_replay_kernel<B, true, false>), grid, block, 0, st, P.L, P.W, M, c);
    else if (all) hipLaunchKernelGGL((increments_replay_kernel<B, false, true>), grid, block, 0, st, P.L, P.W, M, c);
    else hipLaunchKernelGGL((increments_replay_kernel<B, false, false>), grid, block, 0, st, P.L, P.W, M, c);
  }
  return hip_status(hipGetLastError());
}

}  // namespace eks
