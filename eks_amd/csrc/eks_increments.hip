// gfx950 kernels of eks_smooth_increments on scalar chains (EKS_FLAG_DIAG_MODEL): eks_smooth plus the posterior of
// the frame-to-frame increment (lag1, dmean, dV; formulas in eks_increments_lane.hpp).  No reference counterpart.
//   I1 increments_summarize : lane = (chain, chunk of B frames): the chunk's filter element (reads y, var)
//   S1 kalman scan x3       : belief entering / information after every chunk (grouped, lanes along chains; the
//                             sampler's kalman_group_* bodies and SampleWs planes, eks_sample_lane.hpp)
//   I2 increments_replay    : lane = (chain, chunk): filter in registers, fuse, RTS backwards; the five outputs stream
//                             out once, 256-byte rows per wave, non-temporal (reads y, var)
// y and var are read twice, every requested output is written once.  General models: eks_dense.hip, dense_increments.
#include <hip/hip_runtime.h>

#include "eks_increments_lane.hpp"
#include "eks_internal.hpp"

namespace eks {

constexpr int kIncrementsChunk = 32;   // frames per lane: 2 * B VGPRs hold (mf, Pf) of the chunk in I2

// lanes along chains; N < 64 packs 64 / NT chunks of NT = pow2ceil(N) chains into a wave (as eks_sample.hip)
struct IncrementsMap {
  int nt_log2;
  int ntile;     // ceil(N / NT)
};

__device__ __forceinline__ bool increments_coords(const IncrementsMap& L, int N, int nc, int& n, int& j) {
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int tile = wave % L.ntile, cg = wave / L.ntile;
  const int nt = 1 << L.nt_log2;
  n = tile * nt + (lane & (nt - 1));
  j = cg * (64 >> L.nt_log2) + (lane >> L.nt_log2);
  return n < N && j < nc;
}

template <int B, bool UNIT>
__global__ __launch_bounds__(256) void increments_summarize_kernel(IncrementsMap L, SampleWs W, DiagModel M,
                                                                   SampleCall c) {
  int n, j;
  if (!increments_coords(L, W.N, W.nc, n, j)) return;
  sample_summarize_lane<B, UNIT>(W, M, c, n, j);
}

template <int B, bool UNIT, bool ALL>
__global__ __launch_bounds__(256) void increments_replay_kernel(IncrementsMap L, SampleWs W, DiagModel M,
                                                                IncrementsCall c) {
  int n, j;
  if (!increments_coords(L, W.N, W.nc, n, j)) return;
  increments_replay_lane<B, UNIT, ALL>(W, M, c, n, j);
}

// scan: one thread per (group, chain) or per chain, chains fastest
__global__ __launch_bounds__(256) void increments_scan_reduce_kernel(SampleWs W) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < W.ng * W.N) kalman_group_reduce(W, idx % W.N, idx / W.N);
}
__global__ __launch_bounds__(64) void increments_scan_kernel(SampleWs W, DiagModel M) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= W.N) return;
  float m, P;
  load_chain_prior(M, n, m, P);
  kalman_group_scan(W, n, m, P);
}
__global__ __launch_bounds__(256) void increments_scan_apply_kernel(SampleWs W) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < W.ng * W.N) kalman_group_apply(W, idx % W.N, idx / W.N);
}

// ------------------------------------------------------------------------------------------------------------------
static inline size_t plane(size_t rows, int N) { return align_up(rows * (size_t)N * sizeof(float), 256); }

static void increments_geometry(int T, int& nc, int& gs, int& ng) {
  nc = (T + kIncrementsChunk - 1) / kIncrementsChunk;
  gs = 1;
  while (gs * gs < nc) ++gs;
  ng = (nc + gs - 1) / gs;
}

// every launch indexes its threads with an int
bool diag_increments_covers(int T, int N) {
  int nc, gs, ng;
  increments_geometry(T, nc, gs, ng);
  return (size_t)nc * N < (1u << 30);
}

size_t diag_increments_workspace_bytes(int T, int N) {
  int nc, gs, ng;
  increments_geometry(T, nc, gs, ng);
  return 9 * plane(nc, N) + 9 * plane(ng, N);
}

int diag_increments(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, float* ms, float* Vs,
                    float* lag1, float* dmean, float* dV, void* ws, size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, N = d.n_keypoints * d.state_dim;
  if (!diag_increments_covers(T, N)) return EKS_ERR_SHAPE;
  if (ws_bytes < diag_increments_workspace_bytes(T, N)) return EKS_ERR_WORKSPACE;
  SampleWs W{};
  increments_geometry(T, W.nc, W.gs, W.ng);
  W.N = N;
  W.n_draws = 0;
  char* at = static_cast<char*>(ws);
  auto take = [&](size_t rows) {
    float* p = reinterpret_cast<float*>(at);
    at += plane(rows, N);
    return p;
  };
  W.eA = take(W.nc); W.eb = take(W.nc); W.eC = take(W.nc); W.eEta = take(W.nc); W.eJ = take(W.nc);
  W.pm = take(W.nc); W.pP = take(W.nc); W.sEta = take(W.nc); W.sJ = take(W.nc);
  W.gA = take(W.ng); W.gb = take(W.ng); W.gC = take(W.ng); W.gEta = take(W.ng); W.gJ = take(W.ng);
  W.gm = take(W.ng); W.gP = take(W.ng); W.gsEta = take(W.ng); W.gsJ = take(W.ng);

  IncrementsMap L;
  L.nt_log2 = 0;
  while ((1 << L.nt_log2) < N && L.nt_log2 < 6) ++L.nt_log2;
  L.ntile = (N + (1 << L.nt_log2) - 1) >> L.nt_log2;
  const int cpw = 64 >> L.nt_log2;                               // chunks per wave
  const long waves = (long)L.ntile * ((W.nc + cpw - 1) / cpw);
  const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  const SampleCall cs{y, var, nullptr, nullptr, nullptr, T, 0u, 0u, 0u, 0u};
  const IncrementsCall c{y, var, ms, Vs, lag1, dmean, dV, T};
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0;
  const bool all = ms && Vs && lag1 && dmean && dV;
  constexpr int B = kIncrementsChunk;
  const unsigned gN = (unsigned)(((size_t)W.ng * N + 255) / 256);

  {
    ProfScope ps("increments_summarize", st);
    if (unit) hipLaunchKernelGGL((increments_summarize_kernel<B, true>), grid, block, 0, st, L, W, M, cs);
    else hipLaunchKernelGGL((increments_summarize_kernel<B, false>), grid, block, 0, st, L, W, M, cs);
  }
  {
    ProfScope ps("increments_scan", st);
    hipLaunchKernelGGL(increments_scan_reduce_kernel, dim3(gN), dim3(256), 0, st, W);
    hipLaunchKernelGGL(increments_scan_kernel, dim3((N + 63) / 64), dim3(64), 0, st, W, M);
    hipLaunchKernelGGL(increments_scan_apply_kernel, dim3(gN), dim3(256), 0, st, W);
  }
  {
    ProfScope ps("increments_replay", st);
    if (unit && all) hipLaunchKernelGGL((increments_replay_kernel<B, true, true>), grid, block, 0, st, L, W, M, c);
    else if (unit) hipLaunchKernelGGL((increments_replay_kernel<B, true, false>), grid, block, 0, st, L, W, M, c);
    else if (all) hipLaunchKernelGGL((increments_replay_kernel<B, false, true>), grid, block, 0, st, L, W, M, c);
    else hipLaunchKernelGGL((increments_replay_kernel<B, false, false>), grid, block, 0, st, L, W, M, c);
  }
  return hip_status(hipGetLastError());
}

}  // namespace eks
