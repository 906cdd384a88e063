// gfx950 kernels and launches the scalar-chain entry points on eks_chain_plan.hpp share (eks_sample,
// eks_smooth_increments, eks_em_stats, eks_innovations, eks_smooth_tv): the forward pass in front of every replay.
//   C1 chain_summarize : lane = (chain, chunk of B frames): the chunk's filter element (reads y, var)
//   S1 kalman scan x3  : belief entering / information after every chunk (grouped, lanes along chains; the
//                        kalman_group_* bodies over SampleWs planes, eks_sample_lane.hpp)
// Every caller names the two profile scopes its launches are reported under.
#include <hip/hip_runtime.h>

#include "eks_chain_plan.hpp"
#include "eks_internal.hpp"

namespace eks {

template <int B, bool UNIT>
__global__ __launch_bounds__(256) void chain_summarize_kernel(ChainMap L, SampleWs W, DiagModel M, SampleCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  sample_summarize_lane<B, UNIT>(W, M, c, n, j);
}

// scan: one thread per (group, chain) or per chain, chains fastest
__global__ __launch_bounds__(256) void chain_scan_reduce_kernel(SampleWs W) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < W.ng * W.N) kalman_group_reduce(W, idx % W.N, idx / W.N);
}
__global__ __launch_bounds__(64) void chain_scan_kernel(SampleWs W, DiagModel M) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= W.N) return;
  float m, P;
  load_chain_prior(M, n, m, P);
  kalman_group_scan(W, n, m, P);
}
__global__ __launch_bounds__(256) void chain_scan_apply_kernel(SampleWs W) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < W.ng * W.N) kalman_group_apply(W, idx % W.N, idx / W.N);
}

// every launch indexes its threads with an int
bool diag_chain_covers(int T, int N) { return (size_t)chain_geometry(T, kChainChunk).nc * N < (1u << 30); }

// S1.  The elements of eks_smooth_tv carry a per-frame process noise the scan never sees: composing, applying and
// pulling back elements does not involve Q.
int chain_scan(const ChainPlan& P, const DiagModel& M, const char* scan_scope, hipStream_t st) {
  const SampleWs& W = P.W;
  const unsigned gN = (unsigned)(((size_t)W.ng * W.N + 255) / 256);
  ProfScope ps(scan_scope, st);
  hipLaunchKernelGGL(chain_scan_reduce_kernel, dim3(gN), dim3(256), 0, st, W);
  hipLaunchKernelGGL(chain_scan_kernel, dim3((W.N + 63) / 64), dim3(64), 0, st, W, M);
  hipLaunchKernelGGL(chain_scan_apply_kernel, dim3(gN), dim3(256), 0, st, W);
  return hip_status(hipGetLastError());
}

// C1 + S1
int chain_forward(const ChainPlan& P, const DiagModel& M, const SampleCall& c, bool unit, const char* summarize_scope,
                  const char* scan_scope, hipStream_t st) {
  constexpr int B = kChainChunk;
  {
    ProfScope ps(summarize_scope, st);
    if (unit) hipLaunchKernelGGL((chain_summarize_kernel<B, true>), dim3(P.blocks), dim3(256), 0, st, P.L, P.W, M, c);
    else hipLaunchKernelGGL((chain_summarize_kernel<B, false>), dim3(P.blocks), dim3(256), 0, st, P.L, P.W, M, c);
  }
  return chain_scan(P, M, scan_scope, st);
}

}  // namespace eks
