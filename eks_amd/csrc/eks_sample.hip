// gfx950 kernels of eks_sample: whole trajectories drawn from the smoothing distribution p(x_1..x_T | y_1..y_T).
// No reference counterpart (the reference returns the marginals ms, Vs only: eks/core.py:296-297).
//
// Scalar chains (EKS_FLAG_DIAG_MODEL), lane bodies in eks_sample_lane.hpp, lanes along chains as in eks_diag.hip:
//   P1 sample_summarize : lane = (chain, chunk of B frames): the chunk's filter element (reads y, var)
//   S1 kalman scan x3   : belief entering / information after every chunk (grouped, lanes along chains)
//   P2 sample_beta      : lane = (chain, chunk): filtered variances from var alone, the chunk's (G_t, sd_t) in
//                         registers, Gamma once and beta for EVERY draw from regenerated normals (reads var)
//   S2 draw scan x3     : e_next of every chunk per (chain, draw)
//   P3 sample_replay    : lane = (chain, chunk): filter + RTS means in registers once, then every draw walks the
//                         registers backwards with the same normals and streams ms + e out (reads y, var)
// y is read twice and var three times per CALL whatever n_draws is; the output is n_draws * T * N floats written once.
#include <hip/hip_runtime.h>

#include "eks_internal.hpp"
#include "eks_sample_lane.hpp"

namespace eks {

#ifndef EKS_SAMPLE_CHUNK
#define EKS_SAMPLE_CHUNK 32
#endif
constexpr int kSampleChunk = EKS_SAMPLE_CHUNK;   // frames per lane: 3 * B VGPRs hold (ms, G, sd) of the chunk in P3

struct SampleMap {
  int nt_log2;   // log2 of chains per wave row (min(64, pow2ceil(N)))
  int ntile;     // ceil(N / NT)
};

__device__ __forceinline__ bool sample_coords(const SampleMap& L, int N, int nc, int& n, int& j) {
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int tile = wave % L.ntile, cg = wave / L.ntile;
  const int nt = 1 << L.nt_log2;
  n = tile * nt + (lane & (nt - 1));
  j = cg * (64 >> L.nt_log2) + (lane >> L.nt_log2);
  return n < N && j < nc;
}

template <int B, bool UNIT>
__global__ __launch_bounds__(256) void sample_summarize_kernel(SampleMap L, SampleWs W, DiagModel M, SampleCall c) {
  int n, j;
  if (!sample_coords(L, W.N, W.nc, n, j)) return;
  sample_summarize_lane<B, UNIT>(W, M, c, n, j);
}

template <int B, bool UNIT, bool INJ>
__global__ __launch_bounds__(256) void sample_beta_kernel(SampleMap L, SampleWs W, DiagModel M, SampleCall c) {
  int n, j;
  if (!sample_coords(L, W.N, W.nc, n, j)) return;
  sample_beta_lane<B, UNIT, INJ>(W, M, c, n, j);
}

template <int B, bool UNIT, bool INJ>
__global__ __launch_bounds__(256) void sample_replay_kernel(SampleMap L, SampleWs W, DiagModel M, SampleCall c) {
  int n, j;
  if (!sample_coords(L, W.N, W.nc, n, j)) return;
  sample_replay_lane<B, UNIT, INJ>(W, M, c, n, j);
}

// scans: one thread per (group, chain) or per chain, chains fastest
__global__ __launch_bounds__(256) void sample_kalman_reduce_kernel(SampleWs W) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < W.ng * W.N) kalman_group_reduce(W, idx % W.N, idx / W.N);
}
__global__ __launch_bounds__(64) void sample_kalman_scan_kernel(SampleWs W, DiagModel M) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= W.N) return;
  float m, P;
  load_chain_prior(M, n, m, P);
  kalman_group_scan(W, n, m, P);
}
__global__ __launch_bounds__(256) void sample_kalman_apply_kernel(SampleWs W) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < W.ng * W.N) kalman_group_apply(W, idx % W.N, idx / W.N);
}
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
static inline size_t plane(size_t rows, int N) { return align_up(rows * (size_t)N * sizeof(float), 256); }

static void sample_geometry(int T, int& nc, int& gs, int& ng) {
  nc = (T + kSampleChunk - 1) / kSampleChunk;
  gs = 1;
  while (gs * gs < nc) ++gs;
  ng = (nc + gs - 1) / gs;
}

size_t diag_sample_workspace_bytes(int T, int N, int n_draws) {
  int nc, gs, ng;
  sample_geometry(T, nc, gs, ng);
  return 10 * plane(nc, N) + plane((size_t)n_draws * nc, N) + 10 * plane(ng, N) + plane((size_t)n_draws * ng, N);
}

int diag_sample(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, int n_draws, uint64_t seed,
                int first_keypoint, int first_draw, const float* noise, float* ms, float* draws, void* ws,
                size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, N = d.n_keypoints * d.state_dim;
  if (ws_bytes < diag_sample_workspace_bytes(T, N, n_draws)) return EKS_ERR_WORKSPACE;
  SampleWs W;
  sample_geometry(T, W.nc, W.gs, W.ng);
  W.N = N;
  W.n_draws = n_draws;
  // every launch indexes its threads with an int
  if ((size_t)n_draws * W.ng * N >= (1u << 30) || (size_t)W.nc * N >= (1u << 30)) return EKS_ERR_SHAPE;
  char* at = static_cast<char*>(ws);
  auto take = [&](size_t rows) {
    float* p = reinterpret_cast<float*>(at);
    at += plane(rows, N);
    return p;
  };
  W.eA = take(W.nc); W.eb = take(W.nc); W.eC = take(W.nc); W.eEta = take(W.nc); W.eJ = take(W.nc);
  W.pm = take(W.nc); W.pP = take(W.nc); W.sEta = take(W.nc); W.sJ = take(W.nc);
  W.gam = take(W.nc);
  W.beta = take((size_t)n_draws * W.nc);
  W.gA = take(W.ng); W.gb = take(W.ng); W.gC = take(W.ng); W.gEta = take(W.ng); W.gJ = take(W.ng);
  W.gm = take(W.ng); W.gP = take(W.ng); W.gsEta = take(W.ng); W.gsJ = take(W.ng);
  W.hG = take(W.ng);
  W.hB = take((size_t)n_draws * W.ng);

  SampleMap L;
  L.nt_log2 = 0;
  while ((1 << L.nt_log2) < N && L.nt_log2 < 6) ++L.nt_log2;
  L.ntile = (N + (1 << L.nt_log2) - 1) >> L.nt_log2;
  const int cpw = 64 >> L.nt_log2;                               // chunks per wave
  const long waves = (long)L.ntile * ((W.nc + cpw - 1) / cpw);
  const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  const SampleCall c{y, var, noise, ms, draws, T, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (uint32_t)first_keypoint * (uint32_t)d.state_dim, (uint32_t)first_draw};
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0, inj = noise != nullptr;
  constexpr int B = kSampleChunk;
  const unsigned gN = (unsigned)(((size_t)W.ng * N + 255) / 256), dgN = (unsigned)(((size_t)n_draws * W.ng * N + 255) / 256);

  {
    ProfScope ps("sample_summarize", st);
    if (unit) hipLaunchKernelGGL((sample_summarize_kernel<B, true>), grid, block, 0, st, L, W, M, c);
    else hipLaunchKernelGGL((sample_summarize_kernel<B, false>), grid, block, 0, st, L, W, M, c);
  }
  {
    ProfScope ps("sample_kalman_scan", st);
    hipLaunchKernelGGL(sample_kalman_reduce_kernel, dim3(gN), dim3(256), 0, st, W);
    hipLaunchKernelGGL(sample_kalman_scan_kernel, dim3((N + 63) / 64), dim3(64), 0, st, W, M);
    hipLaunchKernelGGL(sample_kalman_apply_kernel, dim3(gN), dim3(256), 0, st, W);
  }
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
