// gfx950 kernels of eks_em_stats on scalar chains (EKS_FLAG_DIAG_MODEL) and of eks_em_scale_step: the E-step
// statistic Sw = sum_t E[w_t w_t^T | y] of the model eks_smooth runs (formulas in eks_em_lane.hpp) and the closed-form
// M-step for the process-noise scale.  No reference counterpart.
//   E1 em_summarize  : lane = (chain, chunk of B frames): the chunk's filter element (reads y, var)
//   S1 kalman scan x3: belief entering / information after every chunk (grouped, lanes along chains; the sampler's
//                      kalman_group_* bodies and SampleWs planes, eks_sample_lane.hpp)
//   E2 em_replay     : lane = (chain, chunk): filter in registers, fuse, RTS backwards; one float64 partial per lane
//                      goes to a [chunk][chain] plane (reads y, var; writes nothing of length T)
//   E3 em_reduce     : per chain, the chunk partials summed in a fixed order that depends on the number of chunks
//                      alone - no floating-point atomics: two calls, or a call on a subset of the keypoints, give the
//                      same bits.  Also the last pass of the general-model form (eks_dense.hip: dense_em).
// y and var are read twice.  General models: eks_dense.hip, dense_em.
#include <hip/hip_runtime.h>

#include "eks_em_lane.hpp"
#include "eks_em_plan.hpp"
#include "eks_internal.hpp"

namespace eks {

template <int B, bool UNIT>
__global__ __launch_bounds__(256) void em_summarize_kernel(EmMap L, SampleWs W, DiagModel M, SampleCall c) {
  int n, j;
  if (!em_coords(L, W.N, W.nc, n, j)) return;
  sample_summarize_lane<B, UNIT>(W, M, c, n, j);
}

template <int B, bool UNIT>
__global__ __launch_bounds__(256) void em_replay_kernel(EmMap L, SampleWs W, DiagModel M, EmCall c) {
  int n, j;
  if (!em_coords(L, W.N, W.nc, n, j)) return;
  em_replay_lane<B, UNIT>(W, M, c, n, j);
}

// scan: one thread per (group, chain) or per chain, chains fastest
__global__ __launch_bounds__(256) void em_scan_reduce_kernel(SampleWs W) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < W.ng * W.N) kalman_group_reduce(W, idx % W.N, idx / W.N);
}
__global__ __launch_bounds__(64) void em_scan_kernel(SampleWs W, DiagModel M) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= W.N) return;
  float m, P;
  load_chain_prior(M, n, m, P);
  kalman_group_scan(W, n, m, P);
}
__global__ __launch_bounds__(256) void em_scan_apply_kernel(SampleWs W) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < W.ng * W.N) kalman_group_apply(W, idx % W.N, idx / W.N);
}

// E3: a workgroup takes kEmCols consecutive columns (chains, or matrix entries of the general form); kEmSegs threads
// per column each sum one contiguous run of ceil(nc / kEmSegs) chunks in chunk order, then one thread per column adds
// the kEmSegs run sums in run order.  The order is a function of nc alone.
constexpr int kEmCols = 16, kEmSegs = 16;
__global__ __launch_bounds__(kEmCols* kEmSegs) void em_reduce_kernel(const double* __restrict__ part, int nc, int ne,
                                                                    double* __restrict__ Sw) {
  __shared__ double runs[kEmSegs][kEmCols];
  const int col = threadIdx.x % kEmCols, seg = threadIdx.x / kEmCols;
  const int e = blockIdx.x * kEmCols + col;
  const int per = (nc + kEmSegs - 1) / kEmSegs;
  const int j0 = seg * per, j1 = min(nc, j0 + per);
  double acc = 0.0;
  if (e < ne)
    for (int j = j0; j < j1; ++j) acc += part[(size_t)j * ne + e];
  runs[seg][col] = acc;
  __syncthreads();
  if (seg == 0 && e < ne) {
    double total = 0.0;
#pragma unroll
    for (int r = 0; r < kEmSegs; ++r) total += runs[r][col];
    Sw[e] = total;
  }
}

int em_reduce(const double* part, int nc, int ne, double* Sw, hipStream_t st) {
  ProfScope ps("em_reduce", st);
  hipLaunchKernelGGL(em_reduce_kernel, dim3((ne + kEmCols - 1) / kEmCols), dim3(kEmCols * kEmSegs), 0, st, part, nc, ne,
                     Sw);
  return hip_status(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------------------------
static inline size_t plane(size_t rows, int N) { return align_up(rows * (size_t)N * sizeof(float), 256); }
static inline size_t plane64(size_t rows, int N) { return align_up(rows * (size_t)N * sizeof(double), 256); }

static void em_geometry(int T, int& nc, int& gs, int& ng) {
  nc = (T + kEmChunk - 1) / kEmChunk;
  gs = 1;
  while (gs * gs < nc) ++gs;
  ng = (nc + gs - 1) / gs;
}

// every launch indexes its threads with an int
bool diag_em_covers(int T, int N) {
  int nc, gs, ng;
  em_geometry(T, nc, gs, ng);
  return (size_t)nc * N < (1u << 30);
}

size_t diag_em_workspace_bytes(int T, int N) {
  int nc, gs, ng;
  em_geometry(T, nc, gs, ng);
  return 9 * plane(nc, N) + 9 * plane(ng, N) + plane64(nc, N);
}

// The planes of W on the caller's workspace (W.pm, W.pP: predicted belief entering every chunk; W.sEta, W.sJ:
// information after it), the lane mapping, the grid and the float64 plane of chunk partials behind them.
void diag_em_plan(int T, int N, void* ws, EmPlan& E) {
  SampleWs& W = E.W;
  W = SampleWs{};
  em_geometry(T, W.nc, W.gs, W.ng);
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
  E.part = reinterpret_cast<double*>(at);

  EmMap& L = E.L;
  L.nt_log2 = 0;
  while ((1 << L.nt_log2) < N && L.nt_log2 < 6) ++L.nt_log2;
  L.ntile = (N + (1 << L.nt_log2) - 1) >> L.nt_log2;
  const int cpw = 64 >> L.nt_log2;                               // chunks per wave
  const long waves = (long)L.ntile * ((W.nc + cpw - 1) / cpw);
  E.grid = dim3((unsigned)((waves + 3) / 4));
}

// S1: the three scan launches over the chunk elements in W.  Also the scan of eks_smooth_tv (eks_smooth_tv.hip),
// whose elements carry a per-frame process noise the scan never sees.
int diag_em_scan(const EmPlan& E, const DiagModel& M, hipStream_t st) {
  const SampleWs& W = E.W;
  const unsigned gN = (unsigned)(((size_t)W.ng * W.N + 255) / 256);
  ProfScope ps("em_scan", st);
  hipLaunchKernelGGL(em_scan_reduce_kernel, dim3(gN), dim3(256), 0, st, W);
  hipLaunchKernelGGL(em_scan_kernel, dim3((W.N + 63) / 64), dim3(64), 0, st, W, M);
  hipLaunchKernelGGL(em_scan_apply_kernel, dim3(gN), dim3(256), 0, st, W);
  return hip_status(hipGetLastError());
}

// E1 + S1 on the caller's workspace.  Also the first two passes of eks_innovations (eks_innov.hip).
int diag_em_forward(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, void* ws, EmPlan& E,
                    hipStream_t st) {
  const int T = d.n_frames, N = d.n_keypoints * d.state_dim;
  diag_em_plan(T, N, ws, E);
  const SampleCall cs{y, var, nullptr, nullptr, nullptr, T, 0u, 0u, 0u, 0u};
  constexpr int B = kEmChunk;
  {
    ProfScope ps("em_summarize", st);
    if (d.flags & EKS_FLAG_UNIT_AC)
      hipLaunchKernelGGL((em_summarize_kernel<B, true>), E.grid, dim3(256), 0, st, E.L, E.W, M, cs);
    else hipLaunchKernelGGL((em_summarize_kernel<B, false>), E.grid, dim3(256), 0, st, E.L, E.W, M, cs);
  }
  return diag_em_scan(E, M, st);
}

int diag_em_stats(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, double* Sw, void* ws,
                  size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, N = d.n_keypoints * d.state_dim;
  if (!diag_em_covers(T, N)) return EKS_ERR_SHAPE;
  if (ws_bytes < diag_em_workspace_bytes(T, N)) return EKS_ERR_WORKSPACE;
  EmPlan E;
  const int rc = diag_em_forward(d, y, var, M, ws, E, st);
  if (rc != EKS_OK) return rc;
  const EmCall c{y, var, E.part, T};
  {
    ProfScope ps("em_replay", st);
    if (d.flags & EKS_FLAG_UNIT_AC)
      hipLaunchKernelGGL((em_replay_kernel<kEmChunk, true>), E.grid, dim3(256), 0, st, E.L, E.W, M, c);
    else hipLaunchKernelGGL((em_replay_kernel<kEmChunk, false>), E.grid, dim3(256), 0, st, E.L, E.W, M, c);
  }
  return em_reduce(E.part, E.W.nc, N, Sw, st);
}

// ==================================================================================================================
// M-step for the scale: s_new = sum_members tr(Q^-1 Sw) / sum_members D (T - 1), on log s with the stop rule
// |delta log s| < tol.  state [n_blocks][4] = {log s, last |delta log s|, iterations, done}.
// ==================================================================================================================
struct EmStep {
  const double *Q, *Sw;
  const int32_t *offs, *members;
  double lo, hi, tol;
  int max_iters, T;
  double *state, *s_keypoint;
};

// tr(Q^-1 Sw) of keypoint k; D == 0: scalar chains of width Dd (Sw [K][Dd], Q's diagonal)
template <int D>
__device__ double em_trace(const EmStep& E, int k, int Dd) {
  if constexpr (D == 0) {
    double tr = 0.0;
    for (int i = 0; i < Dd; ++i) tr += E.Sw[(size_t)k * Dd + i] / E.Q[(size_t)k * Dd * Dd + (size_t)i * (Dd + 1)];
    return tr;
  } else {
    Mat<double, D> Qm, S;
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) {
        Qm.a[a][b] = E.Q[((size_t)k * D + a) * D + b];
        S.a[a][b] = E.Sw[((size_t)k * D + a) * D + b];
      }
    const Mat<double, D> X = chol_solve_mat(chol_factor(mat_symmetrize(Qm)), mat_symmetrize(S));
    double tr = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) tr += X.a[a][a];
    return tr;
  }
}

// returns whether the block is still running after this step
template <int D>
__device__ bool em_step_block(const EmStep& E, int b, int Dd) {
  double* st = E.state + (size_t)b * 4;
  if (st[3] != 0.0 || st[2] >= (double)E.max_iters) return false;
  double num = 0.0, den = 0.0;
  for (int i = E.offs[b]; i < E.offs[b + 1]; ++i) {
    num += em_trace<D>(E, E.members[i], Dd);
    den += (double)Dd * (double)(E.T - 1);
  }
  double ls = log(num / den);
  ls = ls < E.lo ? E.lo : (ls > E.hi ? E.hi : ls);
  const bool bad = !(ls == ls);              // a NaN statistic leaves the scale where it is and never meets tol
  if (bad) ls = st[0];
  const double delta = bad ? HUGE_VAL : fabs(ls - st[0]);
  const bool done = delta < E.tol;
  st[0] = ls;
  st[1] = delta;
  st[2] += 1.0;
  st[3] = done ? 1.0 : 0.0;
  const double s = exp(ls);
  for (int i = E.offs[b]; i < E.offs[b + 1]; ++i) E.s_keypoint[E.members[i]] = s;
  return !done && st[2] < (double)E.max_iters;
}

// one thread per block of keypoints.  single: ONE workgroup walks all blocks and writes the count of those still
// running itself (no memset in front of every iteration, as adam_step); else the count is added to a zeroed counter.
template <int D>
__global__ __launch_bounds__(256) void em_scale_step_kernel(EmStep E, int nb, int Dd, int single,
                                                            int32_t* __restrict__ n_active) {
  __shared__ int running;
  if (threadIdx.x == 0) running = 0;
  __syncthreads();
  int mine = 0;
  for (int b = blockIdx.x * 256 + threadIdx.x; b < nb; b += gridDim.x * 256) mine += em_step_block<D>(E, b, Dd) ? 1 : 0;
  if (mine) atomicAdd(&running, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (single) *n_active = running;
    else if (running) atomicAdd(n_active, running);
  }
}

constexpr int kEmOneBlock = 4096;

int em_scale_step(const eks_dims_t& d, const double* Q, const double* Sw, int n_blocks, const int32_t* offs,
                  const int32_t* members, double lo, double hi, double tol, int max_iters, double* state,
                  double* s_keypoint, int32_t* n_active, hipStream_t st) {
  const EmStep E{Q, Sw, offs, members, lo, hi, tol, max_iters, d.n_frames, state, s_keypoint};
  const int single = n_blocks <= kEmOneBlock ? 1 : 0;
  if (!single) {
    const hipError_t e = hipMemsetAsync(n_active, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return hip_status(e);
  }
  const dim3 grid(single ? 1 : (n_blocks + 255) / 256), block(256);
  ProfScope ps("em_scale_step", st);
  if (d.flags & EKS_FLAG_DIAG_MODEL) {
    hipLaunchKernelGGL(em_scale_step_kernel<0>, grid, block, 0, st, E, n_blocks, d.state_dim, single, n_active);
  } else {
    EKS_DISPATCH_D(d.state_dim, {
      hipLaunchKernelGGL(em_scale_step_kernel<DD>, grid, block, 0, st, E, n_blocks, DD, single, n_active);
    })
  }
  return hip_status(hipGetLastError());
}

}  // namespace eks
