// gfx950 kernels of eks_em_stats on scalar chains (EKS_FLAG_DIAG_MODEL) and of eks_em_scale_step: the E-step
// statistic Sw = sum_t E[w_t w_t^T | y] of the model eks_smooth runs (formulas in eks_em_lane.hpp) and the closed-form
// M-step for the process-noise scale.  No reference counterpart.
//   E1 summarize     : lane = (chain, chunk of B frames): the chunk's filter element (reads y, var)    } eks_chain.hip,
//   S1 kalman scan x3: belief entering / information after every chunk (grouped, lanes along chains) } chain_forward
//   E2 em_replay     : lane = (chain, chunk): filter in registers, fuse, RTS backwards; one float64 partial per lane
//                      goes to a [chunk][chain] plane (reads y, var; writes nothing of length T)
//   E3 em_reduce     : per chain, the chunk partials summed in a fixed order that depends on the number of chunks
//                      alone - no floating-point atomics: two calls, or a call on a subset of the keypoints, give the
//                      same bits.  Also the last pass of the general-model form (eks_dense.hip: dense_em).
// y and var are read twice.  General models: eks_dense.hip, dense_em.
#include <hip/hip_runtime.h>

#include "eks_chain_plan.hpp"
#include "eks_em_lane.hpp"
#include "eks_internal.hpp"

namespace eks {

template <int B, bool UNIT>
__global__ __launch_bounds__(256) void em_replay_kernel(ChainMap L, SampleWs W, DiagModel M, EmCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  em_replay_lane<B, UNIT>(W, M, c, n, j);
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
// the planes of the forward pass and the float64 plane of chunk partials behind them; nothing of length T
size_t diag_em_workspace_bytes(int T, int N) { return chain_workspace_bytes(T, N, 0, true); }

int diag_em_stats(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, double* Sw, void* ws,
                  size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, N = d.n_keypoints * d.state_dim;
  if (!diag_chain_covers(T, N)) return EKS_ERR_SHAPE;
  if (ws_bytes < diag_em_workspace_bytes(T, N)) return EKS_ERR_WORKSPACE;
  const ChainPlan E = chain_plan(T, N, 0, true, ws);
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0;
  const SampleCall cs{y, var, nullptr, nullptr, nullptr, T, 0u, 0u, 0u, 0u};
  const int rc = chain_forward(E, M, cs, unit, "em_summarize", "em_scan", st);
  if (rc != EKS_OK) return rc;
  const EmCall c{y, var, E.part, T};
  {
    ProfScope ps("em_replay", st);
    if (unit) hipLaunchKernelGGL((em_replay_kernel<kChainChunk, true>), dim3(E.blocks), dim3(256), 0, st, E.L, E.W, M, c);
    else hipLaunchKernelGGL((em_replay_kernel<kChainChunk, false>), dim3(E.blocks), dim3(256), 0, st, E.L, E.W, M, c);
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
