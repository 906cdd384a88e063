// gfx950 kernels of eks_innovations on scalar chains (EKS_FLAG_DIAG_MODEL): the forward filter's one-step-ahead
// prediction errors, their variances and the exact log-likelihood of the model eks_smooth runs (formulas in
// eks_innov_lane.hpp).  No reference counterpart.
//   E1 summarize     : lane = (chain, chunk of B frames): the chunk's filter element (reads y, var)   } eks_chain.hip,
//   S1 kalman scan x3: predicted belief entering every chunk (grouped, lanes along chains)            } chain_forward
//   I2 innov_replay  : lane = (chain, chunk): filter forwards in registers from the belief that entered the chunk;
//                      d and S stream out frame by frame, one float64 partial of the log-likelihood per lane goes
//                      to a [chunk][chain] plane
//   E3 em_reduce     : per chain, the chunk partials summed in the fixed order of eks_em.hip: two calls, or a call on
//                      a subset of the keypoints, give the same bits
// y and var are read twice; with loglik alone nothing of length T is written.  General models: eks_dense.hip,
// dense_innovations.
#include <hip/hip_runtime.h>

#include "eks_chain_plan.hpp"
#include "eks_innov_lane.hpp"
#include "eks_internal.hpp"

namespace eks {

template <int B, bool UNIT>
__global__ __launch_bounds__(256) void innov_replay_kernel(ChainMap L, SampleWs W, DiagModel M, InnovCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  innov_replay_lane<B, UNIT>(W, M, c, n, j);
}

int diag_innovations(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, float* innov,
                     float* innov_var, double* loglik, void* ws, size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, N = d.n_keypoints * d.state_dim;
  if (!diag_chain_covers(T, N)) return EKS_ERR_SHAPE;
  if (ws_bytes < diag_em_workspace_bytes(T, N)) return EKS_ERR_WORKSPACE;
  const ChainPlan E = chain_plan(T, N, 0, true, ws);   // eks_em_stats' workspace
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0;
  const SampleCall cs{y, var, nullptr, nullptr, nullptr, T, 0u, 0u, 0u, 0u};
  const int rc = chain_forward(E, M, cs, unit, "em_summarize", "em_scan", st);
  if (rc != EKS_OK) return rc;
  const InnovCall c{y, var, innov, innov_var, loglik ? E.part : nullptr, T};
  {
    ProfScope ps("innov_replay", st);
    if (unit) hipLaunchKernelGGL((innov_replay_kernel<kChainChunk, true>), dim3(E.blocks), dim3(256), 0, st, E.L, E.W, M, c);
    else hipLaunchKernelGGL((innov_replay_kernel<kChainChunk, false>), dim3(E.blocks), dim3(256), 0, st, E.L, E.W, M, c);
  }
  if (!loglik) return hip_status(hipGetLastError());
  return em_reduce(E.part, E.W.nc, N, loglik, st);
}

}  // namespace eks
