// eks_sample for general linear models (dense A, C, Q; D = 1..6; the multi-camera path): Durbin & Koopman's (2002)
// simulation smoother composed from the existing smoother - correct first, not tuned.  No reference counterpart.
//   1. dense_sample_simulate : thread = (keypoint, draw), sequential in time: (x+, y+) from the ZERO-MEAN model with
//                              the data's own variances; x+ goes straight into `draws`, y+ into the stacked problem
//   2. dense_smooth          : ONE call over (n_draws + 1) K chains stacked along K: set 0 = the data (gives ms),
//                              set 1 + d = y+ of draw d with m0 = 0 (gives E[x+ | y+])
//   3. dense_sample_combine  : draws = ms + (x+ - E[x+ | y+])
// Noise width W = D + O per (draw, frame, keypoint): D state normals (chol(S0) at frame 0, chol(s Q) afterwards),
// then O observation normals.  Generator: Philox4x32-10, key = seed, counter = (frame, global keypoint, global draw,
// b), whose four words give normals 4 b .. 4 b + 3 by two Box-Muller transforms (eks_sample_lane.hpp).
// A draw costs one pass of the smoother over its own copy of the session; the workspace grows by 4 (2 O + 2 D) T K
// bytes per draw (y+, the copy of var, the stacked means and variances) plus the stacked smoother's own scratch.
// x+, y+ and the stacked smoother's means are float32, so the deviation carries their rounding, which grows with |x+|
// (unit-root dynamics) while the posterior sd does not: measured against a float64 transcription with only those
// stores rounded in tests/test_gpu_sampling_dense.py (figures in its docstring and in DESIGN.md 9c).
#include <hip/hip_runtime.h>

#include "eks_internal.hpp"
#include "eks_sample_lane.hpp"
#include "eks_smooth_robust_lane.hpp"

namespace eks {

constexpr int kDenseNoiseMax = 6 + 64;   // W = D + O with D <= 6, O <= 64 (dense_smooth's limits)

struct DenseSampleWs {
  float *yP, *varP, *msP, *VsP;            // stacked problem [T][Kp][O], [T][Kp][O], [T][Kp][D], [T][Kp][D]
  double *m0, *S0, *A, *C, *Q, *s;         // its parameters, Kp = (n_draws + 1) K chains
  void* smooth_ws;
  size_t smooth_ws_bytes;
};

// wP != nullptr: dense_sample_tv's layout - a [T][Kp] float scale plane, and dense_smooth_tv's scratch behind it
static size_t dense_sample_carve(int T, int K, int D, int O, int n_draws, char* base, DenseSampleWs* out,
                                 float** wP = nullptr) {
  const size_t Kp = ((size_t)n_draws + 1) * K;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + at : nullptr;
    at += align_up(bytes, 256);
    return p;
  };
  DenseSampleWs w;
  w.yP = (float*)take((size_t)T * Kp * O * 4);
  w.varP = (float*)take((size_t)T * Kp * O * 4);
  w.msP = (float*)take((size_t)T * Kp * D * 4);
  w.VsP = (float*)take((size_t)T * Kp * D * 4);
  w.m0 = (double*)take(Kp * D * 8);
  w.S0 = (double*)take(Kp * D * D * 8);
  w.A = (double*)take(Kp * D * D * 8);
  w.C = (double*)take(Kp * O * D * 8);
  w.Q = (double*)take(Kp * D * D * 8);
  w.s = (double*)take(Kp * 8);
  if (wP) *wP = (float*)take((size_t)T * Kp * 4);
  w.smooth_ws_bytes = wP ? dense_smooth_tv_workspace_bytes(T, (int)Kp, D, O) : dense_smooth_workspace_bytes(T, (int)Kp, D, O);
  w.smooth_ws = take(w.smooth_ws_bytes);
  if (out) *out = w;
  return at;
}

size_t dense_sample_workspace_bytes(int T, int K, int D, int O, int n_draws) {
  return dense_sample_carve(T, K, D, O, n_draws, nullptr, nullptr);
}

// normal w of (frame t, global keypoint, global draw)
__device__ __forceinline__ void dense_normals(uint32_t k0, uint32_t k1, int t, uint32_t kp, uint32_t draw, int W,
                                              float* z) {
  for (int b = 0; 4 * b < W; ++b) {
    const Philox4 w = philox4x32_10((uint32_t)t, kp, draw, (uint32_t)b, k0, k1);
    float n4[4];
    box_muller(w.x[0], w.x[1], n4[0], n4[1]);
    box_muller(w.x[2], w.x[3], n4[2], n4[3]);
    for (int i = 0; i < 4 && 4 * b + i < W; ++i) z[4 * b + i] = n4[i];
  }
}

__global__ __launch_bounds__(256) void dense_sample_noise_kernel(int T, int K, int W, int n_draws, uint32_t k0, uint32_t k1,
                                                                 uint32_t kp_base, uint32_t d_base, float* noise) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)n_draws * T * K) return;
  const int k = (int)(idx % K), t = (int)((idx / K) % T), d = (int)(idx / ((size_t)K * T));
  float z[kDenseNoiseMax];
  dense_normals(k0, k1, t, kp_base + k, d_base + d, W, z);
  for (int w = 0; w < W; ++w) noise[idx * W + w] = z[w];
}

// lower Cholesky factor of a symmetric PSD matrix (a non-positive pivot gives a zero column: a singular Q draws
// nothing along that direction)
template <int D>
__device__ void chol_psd(const double (&M)[D][D], double (&L)[D][D]) {
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) L[i][j] = 0.0;
  for (int j = 0; j < D; ++j) {
    double dj = M[j][j];
    for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k];
    if (!(dj > 0.0)) continue;
    const double r = sqrt(dj);
    L[j][j] = r;
    for (int i = j + 1; i < D; ++i) {
      double v = M[i][j];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / r;
    }
  }
}

// thread = (keypoint k, set): set 0 copies the data into the stacked problem, set 1 + d simulates draw d
template <int D>
__global__ __launch_bounds__(64) void dense_sample_simulate_kernel(int T, int K, int O, int n_draws, const float* y,
                                                                   const float* var, DenseModel M, DenseSampleWs P,
                                                                   const float* noise, float* draws, uint32_t k0,
                                                                   uint32_t k1, uint32_t kp_base, uint32_t d_base) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  const size_t Kp = ((size_t)n_draws + 1) * K;
  if ((size_t)idx >= Kp) return;
  const int k = idx % K, set = idx / K;
  // the chain's parameters in the stacked problem
  for (int i = 0; i < D; ++i) P.m0[(size_t)idx * D + i] = set == 0 ? M.m0[(size_t)k * D + i] : 0.0;
  for (int i = 0; i < D * D; ++i) {
    P.S0[(size_t)idx * D * D + i] = M.S0[(size_t)k * D * D + i];
    P.A[(size_t)idx * D * D + i] = M.A[(size_t)k * D * D + i];
    P.Q[(size_t)idx * D * D + i] = M.Q[(size_t)k * D * D + i];
  }
  for (int i = 0; i < O * D; ++i) P.C[(size_t)idx * O * D + i] = M.C[(size_t)k * O * D + i];
  P.s[idx] = M.s[k];
  if (set == 0) {
    for (int t = 0; t < T; ++t)
      for (int o = 0; o < O; ++o) {
        const size_t src = ((size_t)t * K + k) * O + o, dst = ((size_t)t * Kp + idx) * O + o;
        P.yP[dst] = y[src];
        P.varP[dst] = var[src];
      }
    return;
  }
  const int d = set - 1;
  double S0m[D][D], Qm[D][D], Am[D][D], L0[D][D], Lq[D][D];
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) {
      S0m[i][j] = M.S0[(size_t)k * D * D + i * D + j];
      Qm[i][j] = M.s[k] * M.Q[(size_t)k * D * D + i * D + j];
      Am[i][j] = M.A[(size_t)k * D * D + i * D + j];
    }
  chol_psd<D>(S0m, L0);
  chol_psd<D>(Qm, Lq);
  const double* Cm = M.C + (size_t)k * O * D;
  const int W = D + O;
  double x[D];
  for (int i = 0; i < D; ++i) x[i] = 0.0;
  float z[kDenseNoiseMax];
  for (int t = 0; t < T; ++t) {
    if (noise) {
      const float* zr = noise + (((size_t)d * T + t) * K + k) * W;
      for (int w = 0; w < W; ++w) z[w] = zr[w];
    } else {
      dense_normals(k0, k1, t, kp_base + k, d_base + d, W, z);
    }
    double xn[D];
    for (int i = 0; i < D; ++i) {
      double v = 0.0;
      if (t > 0)
        for (int j = 0; j < D; ++j) v += Am[i][j] * x[j];
      for (int j = 0; j <= i; ++j) v += (t == 0 ? L0[i][j] : Lq[i][j]) * (double)z[j];
      xn[i] = v;
    }
    for (int i = 0; i < D; ++i) {
      x[i] = xn[i];
      draws[(((size_t)d * T + t) * K + k) * D + i] = (float)x[i];
    }
    for (int o = 0; o < O; ++o) {
      double v = 0.0;
      for (int j = 0; j < D; ++j) v += Cm[o * D + j] * x[j];
      const float r = var[((size_t)t * K + k) * O + o];
      v += sqrt((double)clip_var(r)) * (double)z[D + o];
      const size_t dst = ((size_t)t * Kp + idx) * O + o;
      P.yP[dst] = (float)v;
      P.varP[dst] = r;
    }
  }
}

// draws[d][t][k][i] = ms[t][k][i] + (x+ - E[x+ | y+]); thread = (t, k, i) walks the draws
__global__ __launch_bounds__(256) void dense_sample_combine_kernel(int T, int K, int D, int n_draws, const float* msP,
                                                                   float* ms, float* draws) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)T * K * D) return;
  const int i = (int)(idx % D), k = (int)((idx / D) % K);
  const size_t t = idx / ((size_t)D * K), Kp = ((size_t)n_draws + 1) * K;
  const float m = msP[(t * Kp + k) * D + i];
  if (ms) ms[idx] = m;
  for (int d = 0; d < n_draws; ++d) {
    const size_t o = (size_t)d * T * K * D + idx;
    draws[o] = m + (draws[o] - msP[(t * Kp + (size_t)(d + 1) * K + k) * D + i]);
  }
}

int dense_sample(const eks_dims_t& d, const float* y, const float* var, const DenseModel& M, int n_draws, uint64_t seed,
                 int first_keypoint, int first_draw, const float* noise, float* ms, float* draws, void* ws,
                 size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, K = d.n_keypoints, D = d.state_dim, O = d.obs_dim;
  if (D < 1 || D > 6 || O < 1 || O > 64) return EKS_ERR_UNSUPPORTED;
  const size_t Kp = ((size_t)n_draws + 1) * K;
  if (Kp * D > (1u << 24)) return EKS_ERR_SHAPE;
  if (ws_bytes < dense_sample_workspace_bytes(T, K, D, O, n_draws)) return EKS_ERR_WORKSPACE;
  DenseSampleWs P;
  dense_sample_carve(T, K, D, O, n_draws, static_cast<char*>(ws), &P);
  {
    ProfScope ps("dense_sample_simulate", st);
    EKS_DISPATCH_D(D, hipLaunchKernelGGL((dense_sample_simulate_kernel<DD>), dim3((unsigned)((Kp + 63) / 64)), dim3(64), 0,
                                         st, T, K, O, n_draws, y, var, M, P, noise, draws, (uint32_t)seed,
                                         (uint32_t)(seed >> 32), (uint32_t)first_keypoint, (uint32_t)first_draw));
  }
  eks_dims_t dp = d;
  dp.n_keypoints = (int)Kp;
  // the caller's model flags go through to the stacked smoothing call; only the shape of its Vs is ours
  dp.flags = (d.flags & ~(uint32_t)(EKS_FLAG_DIAG_MODEL | EKS_FLAG_UNIT_AC)) | EKS_FLAG_VS_DIAG;
  const DenseModel MP{P.m0, P.S0, P.A, P.C, P.Q, P.s};
  const int rc = dense_smooth(dp, P.yP, P.varP, MP, P.msP, P.VsP, P.smooth_ws, P.smooth_ws_bytes, st);
  if (rc != EKS_OK) return rc;
  {
    ProfScope ps("dense_sample_combine", st);
    const size_t n = (size_t)T * K * D;
    hipLaunchKernelGGL(dense_sample_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, T, K, D, n_draws,
                       P.msP, ms, draws);
  }
  return hip_status(hipGetLastError());
}

// ---- eks_sample_tv: the same three steps under a per-frame process-noise scale w and observation weights lam --------
//   1. dense_sample_tv_simulate : as above with the state noise of the step INTO frame t scaled by sqrt(w_t) and the
//                                 observation noise drawn at r_eff = robust_var(var, lam); r_eff goes into varP
//   2. dense_sample_tv_scale    : the stacked problem's [T][Kp] scale plane (every set reads its keypoint's w; 1
//                                 without qscale)
//   3. dense_smooth_tv on the stacked problem, then dense_sample_combine as above
// w at frame t is qscale[t] (shared) or qscale[t][k]; row 0 is never read.
__device__ __forceinline__ float dense_tv_scale(const float* qscale, int per_keypoint, int K, int t, int k) {
  return qscale ? qscale[per_keypoint ? (size_t)t * K + k : (size_t)t] : 1.0f;
}

// thread = (frame t, stacked chain): row 0 is written as 1 (dense_smooth_tv never reads it; a NaN there stays out)
__global__ __launch_bounds__(256) void dense_sample_tv_scale_kernel(int T, int K, int n_draws, const float* qscale,
                                                                    int per_keypoint, float* wP) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t Kp = ((size_t)n_draws + 1) * K;
  if (idx >= (size_t)T * Kp) return;
  const int t = (int)(idx / Kp), k = (int)((idx % Kp) % K);
  wP[idx] = t == 0 ? 1.0f : dense_tv_scale(qscale, per_keypoint, K, t, k);
}

// thread = (keypoint k, set), as dense_sample_simulate_kernel
template <int D>
__global__ __launch_bounds__(64) void dense_sample_tv_simulate_kernel(int T, int K, int O, int n_draws, const float* y,
                                                                      const float* var, const float* qscale,
                                                                      int per_keypoint, const float* weights,
                                                                      DenseModel M, DenseSampleWs P, const float* noise,
                                                                      float* draws, uint32_t k0, uint32_t k1,
                                                                      uint32_t kp_base, uint32_t d_base) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  const size_t Kp = ((size_t)n_draws + 1) * K;
  if ((size_t)idx >= Kp) return;
  const int k = idx % K, set = idx / K;
  for (int i = 0; i < D; ++i) P.m0[(size_t)idx * D + i] = set == 0 ? M.m0[(size_t)k * D + i] : 0.0;
  for (int i = 0; i < D * D; ++i) {
    P.S0[(size_t)idx * D * D + i] = M.S0[(size_t)k * D * D + i];
    P.A[(size_t)idx * D * D + i] = M.A[(size_t)k * D * D + i];
    P.Q[(size_t)idx * D * D + i] = M.Q[(size_t)k * D * D + i];
  }
  for (int i = 0; i < O * D; ++i) P.C[(size_t)idx * O * D + i] = M.C[(size_t)k * O * D + i];
  P.s[idx] = M.s[k];
  auto r_eff = [&](size_t src) { return weights ? robust_var(var[src], weights[src]) : clip_var(var[src]); };
  if (set == 0) {
    for (int t = 0; t < T; ++t)
      for (int o = 0; o < O; ++o) {
        const size_t src = ((size_t)t * K + k) * O + o, dst = ((size_t)t * Kp + idx) * O + o;
        P.yP[dst] = y[src];
        P.varP[dst] = r_eff(src);
      }
    return;
  }
  const int d = set - 1;
  double S0m[D][D], Qm[D][D], Am[D][D], L0[D][D], Lq[D][D];
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) {
      S0m[i][j] = M.S0[(size_t)k * D * D + i * D + j];
      Qm[i][j] = M.s[k] * M.Q[(size_t)k * D * D + i * D + j];
      Am[i][j] = M.A[(size_t)k * D * D + i * D + j];
    }
  chol_psd<D>(S0m, L0);
  chol_psd<D>(Qm, Lq);
  const double* Cm = M.C + (size_t)k * O * D;
  const int W = D + O;
  double x[D];
  for (int i = 0; i < D; ++i) x[i] = 0.0;
  float z[kDenseNoiseMax];
  for (int t = 0; t < T; ++t) {
    if (noise) {
      const float* zr = noise + (((size_t)d * T + t) * K + k) * W;
      for (int w = 0; w < W; ++w) z[w] = zr[w];
    } else {
      dense_normals(k0, k1, t, kp_base + k, d_base + d, W, z);
    }
    // chol(s w_t Q) = sqrt(w_t) chol(s Q)
    const double sw = t == 0 ? 1.0 : sqrt((double)dense_tv_scale(qscale, per_keypoint, K, t, k));
    double xn[D];
    for (int i = 0; i < D; ++i) {
      double v = 0.0;
      if (t > 0)
        for (int j = 0; j < D; ++j) v += Am[i][j] * x[j];
      for (int j = 0; j <= i; ++j) v += (t == 0 ? L0[i][j] : sw * Lq[i][j]) * (double)z[j];
      xn[i] = v;
    }
    for (int i = 0; i < D; ++i) {
      x[i] = xn[i];
      draws[(((size_t)d * T + t) * K + k) * D + i] = (float)x[i];
    }
    for (int o = 0; o < O; ++o) {
      double v = 0.0;
      for (int j = 0; j < D; ++j) v += Cm[o * D + j] * x[j];
      const float r = r_eff(((size_t)t * K + k) * O + o);
      v += sqrt((double)r) * (double)z[D + o];
      const size_t dst = ((size_t)t * Kp + idx) * O + o;
      P.yP[dst] = (float)v;
      P.varP[dst] = r;
    }
  }
}

// 0 where dense_sample_tv refuses the shape with EKS_ERR_SHAPE (the caller has checked D <= 6, O <= 64)
size_t dense_sample_tv_workspace_bytes(int T, int K, int D, int O, int n_draws) {
  const size_t Kp = ((size_t)n_draws + 1) * K;
  if (Kp * D > (1u << 24) || (size_t)T * Kp >= ((size_t)1 << 38)) return 0;
  if (!dense_smooth_tv_workspace_bytes(T, (int)Kp, D, O)) return 0;
  float* wP;
  return dense_sample_carve(T, K, D, O, n_draws, nullptr, nullptr, &wP);
}

int dense_sample_tv(const eks_dims_t& d, const float* y, const float* var, const float* qscale, int per_keypoint,
                    const float* weights, const DenseModel& M, int n_draws, uint64_t seed, int first_keypoint,
                    int first_draw, const float* noise, float* ms, float* draws, void* ws, size_t ws_bytes,
                    hipStream_t st) {
  const int T = d.n_frames, K = d.n_keypoints, D = d.state_dim, O = d.obs_dim;
  if (D < 1 || D > 6 || O < 1 || O > 64) return EKS_ERR_UNSUPPORTED;
  const size_t Kp = ((size_t)n_draws + 1) * K;
  const size_t need = dense_sample_tv_workspace_bytes(T, K, D, O, n_draws);
  if (!need) return EKS_ERR_SHAPE;
  if (ws_bytes < need) return EKS_ERR_WORKSPACE;
  DenseSampleWs P;
  float* wP;
  dense_sample_carve(T, K, D, O, n_draws, static_cast<char*>(ws), &P, &wP);
  const int pk = per_keypoint ? 1 : 0;
  {
    ProfScope ps("dense_sample_tv_simulate", st);
    EKS_DISPATCH_D(D, hipLaunchKernelGGL((dense_sample_tv_simulate_kernel<DD>), dim3((unsigned)((Kp + 63) / 64)), dim3(64),
                                         0, st, T, K, O, n_draws, y, var, qscale, pk, weights, M, P, noise, draws,
                                         (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)first_keypoint,
                                         (uint32_t)first_draw));
  }
  {
    ProfScope ps("dense_sample_tv_scale", st);
    hipLaunchKernelGGL(dense_sample_tv_scale_kernel, dim3((unsigned)(((size_t)T * Kp + 255) / 256)), dim3(256), 0, st, T, K,
                       n_draws, qscale, pk, wP);
  }
  eks_dims_t dp = d;
  dp.n_keypoints = (int)Kp;
  dp.flags = (d.flags & ~(uint32_t)(EKS_FLAG_DIAG_MODEL | EKS_FLAG_UNIT_AC)) | EKS_FLAG_VS_DIAG;
  const DenseModel MP{P.m0, P.S0, P.A, P.C, P.Q, P.s};
  const int rc = dense_smooth_tv(dp, P.yP, P.varP, wP, 1, MP, P.msP, P.VsP, P.smooth_ws, P.smooth_ws_bytes, st);
  if (rc != EKS_OK) return rc;
  {
    ProfScope ps("dense_sample_combine", st);
    const size_t n = (size_t)T * K * D;
    hipLaunchKernelGGL(dense_sample_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, T, K, D, n_draws,
                       P.msP, ms, draws);
  }
  return hip_status(hipGetLastError());
}

int dense_sample_noise(int T, int K, int W, int n_draws, uint64_t seed, int first_keypoint, int first_draw, float* noise,
                       hipStream_t st) {
  const size_t total = (size_t)n_draws * T * K;
  if (W > kDenseNoiseMax || (total + 255) / 256 >= (1u << 31)) return EKS_ERR_SHAPE;
  hipLaunchKernelGGL(dense_sample_noise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, T, K, W, n_draws,
                     (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)first_keypoint, (uint32_t)first_draw, noise);
  return hip_status(hipGetLastError());
}

}  // namespace eks
