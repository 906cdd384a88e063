// gfx950 kernels of eks_sample: whole trajectories drawn from the smoothing distribution p(x_1..x_T | y_1..y_T).
// No reference counterpart (the reference returns the marginals ms, Vs only: eks/core.py:296-297).
//
// Scalar chains (EKS_FLAG_DIAG_MODEL), lane bodies in eks_sample_lane.hpp, lanes along chains as in eks_diag.hip:
//   P1 summarize        : lane = (chain, chunk of B frames): the chunk's filter element (reads y, var)  } eks_chain.hip,
//   S1 kalman scan x3   : belief entering / information after every chunk (grouped, lanes along chains) } chain_forward
//   P2 sample_beta      : lane = (chain, chunk): filtered variances from var alone, the chunk's (G_t, sd_t) in
//                         registers, Gamma once and beta for EVERY draw from regenerated normals (reads var)
//   S2 draw scan x3     : e_next of every chunk per (chain, draw)
//   P3 sample_replay    : lane = (chain, chunk): filter + RTS means in registers once, then every draw walks the
//                         registers backwards with the same normals and streams ms + e out (reads y, var)
// y is read twice and var three times per CALL whatever n_draws is; the output is n_draws * T * N floats written once.
#include <hip/hip_runtime.h>

#include "eks_chain_plan.hpp"
#include "eks_internal.hpp"

namespace eks {

template <int B, bool UNIT, bool INJ>
__global__ __launch_bounds__(256) void sample_beta_kernel(ChainMap L, SampleWs W, DiagModel M, SampleCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  sample_beta_lane<B, UNIT, INJ>(W, M, c, n, j);
}

template <int B, bool UNIT, bool INJ>
__global__ __launch_bounds__(256) void sample_replay_kernel(ChainMap L, SampleWs W, DiagModel M, SampleCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  sample_replay_lane<B, UNIT, INJ>(W, M, c, n, j);
}

// draw scans: one thread per (draw, group, chain) or per (draw, chain), chains fastest
__global__ __launch_bounds__(256) void sample_draw_reduce_kernel(SampleWs W) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= W.n_draws * W.ng * W.N) return;
  const int gn = idx % (W.ng * W.N);
  draw_group_reduce(W, gn % W.N, gn / W.N, idx / (W.ng * W.N));
}
__global__ __launch_bounds__(64) void sample_draw_scan_kernel(SampleWs W) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx < W.n_draws * W.N) draw_group_scan(W, idx % W.N, idx / W.N);
}
__global__ __launch_bounds__(256) void sample_draw_apply_kernel(SampleWs W) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= W.n_draws * W.ng * W.N) return;
  const int gn = idx % (W.ng * W.N);
  draw_group_apply(W, gn % W.N, gn / W.N, idx / (W.ng * W.N));
}

// eks_sample_noise: thread = (draw, frame / 4, chain), chains fastest; noise [n_draws][T][N]
__global__ __launch_bounds__(256) void sample_noise_kernel(int T, int N, int n_draws, uint32_t k0, uint32_t k1,
                                                           uint32_t n_base, uint32_t d_base, float* __restrict__ noise) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int nq = (T + 3) / 4;
  if (idx >= (size_t)n_draws * nq * N) return;
  const int n = (int)(idx % N);
  const int tq = (int)((idx / N) % nq);
  const int d = (int)(idx / ((size_t)N * nq));
  float z[4];
  NoiseGen{k0, k1, n_base + (uint32_t)n, d_base + (uint32_t)d}.get4(tq, 4, z);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (4 * tq + i < T) noise[((size_t)d * T + 4 * tq + i) * (size_t)N + n] = z[i];
}

// ------------------------------------------------------------------------------------------------------------------
size_t diag_sample_workspace_bytes(int T, int N, int n_draws) { return chain_workspace_bytes(T, N, n_draws, false); }

int diag_sample(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, int n_draws, uint64_t seed,
                int first_keypoint, int first_draw, const float* noise, float* ms, float* draws, void* ws,
                size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, N = d.n_keypoints * d.state_dim;
  if (ws_bytes < diag_sample_workspace_bytes(T, N, n_draws)) return EKS_ERR_WORKSPACE;
  const ChainPlan P = chain_plan(T, N, n_draws, false, ws);
  const SampleWs& W = P.W;
  // every launch indexes its threads with an int
  if ((size_t)n_draws * W.ng * N >= (1u << 30) || !diag_chain_covers(T, N)) return EKS_ERR_SHAPE;
  const dim3 grid(P.blocks), block(256);
  const ChainMap& L = P.L;
  const SampleCall c{y, var, noise, ms, draws, T, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (uint32_t)first_keypoint * (uint32_t)d.state_dim, (uint32_t)first_draw};
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0, inj = noise != nullptr;
  constexpr int B = kChainChunk;
  const unsigned dgN = (unsigned)(((size_t)n_draws * W.ng * N + 255) / 256);

  const int rc = chain_forward(P, M, c, unit, "sample_summarize", "sample_kalman_scan", st);
  if (rc != EKS_OK) return rc;
  {
    ProfScope ps("sample_beta", st);
    if (unit && inj) hipLaunchKernelGGL((sample_beta_kernel<B, true, true>), grid, block, 0, st, L, W, M, c);
    else if (unit) hipLaunchKernelGGL((sample_beta_kernel<B, true, false>), grid, block, 0, st, L, W, M, c);
    else if (inj) hipLaunchKernelGGL((sample_beta_kernel<B, false, true>), grid, block, 0, st, L, W, M, c);
    else hipLaunchKernelGGL((sample_beta_kernel<B, false, false>), grid, block, 0, st, L, W, M, c);
  }
  {
    ProfScope ps("sample_draw_scan", st);
    hipLaunchKernelGGL(sample_draw_reduce_kernel, dim3(dgN), dim3(256), 0, st, W);
    hipLaunchKernelGGL(sample_draw_scan_kernel, dim3((unsigned)(((size_t)n_draws * N + 63) / 64)), dim3(64), 0, st, W);
    hipLaunchKernelGGL(sample_draw_apply_kernel, dim3(dgN), dim3(256), 0, st, W);
  }
  {
    ProfScope ps("sample_replay", st);
    if (unit && inj) hipLaunchKernelGGL((sample_replay_kernel<B, true, true>), grid, block, 0, st, L, W, M, c);
    else if (unit) hipLaunchKernelGGL((sample_replay_kernel<B, true, false>), grid, block, 0, st, L, W, M, c);
    else if (inj) hipLaunchKernelGGL((sample_replay_kernel<B, false, true>), grid, block, 0, st, L, W, M, c);
    else hipLaunchKernelGGL((sample_replay_kernel<B, false, false>), grid, block, 0, st, L, W, M, c);
  }
  return hip_status(hipGetLastError());
}

int diag_sample_noise(int T, int N, int D, int n_draws, uint64_t seed, int first_keypoint, int first_draw, float* noise,
                      hipStream_t st) {
  const size_t total = (size_t)n_draws * ((T + 3) / 4) * N;
  if ((total + 255) / 256 >= (1u << 31)) return EKS_ERR_SHAPE;
  hipLaunchKernelGGL(sample_noise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, T, N, n_draws,
                     (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)first_keypoint * (uint32_t)D, (uint32_t)first_draw,
                     noise);
  return hip_status(hipGetLastError());
}

}  // namespace eks
