// gfx950 kernels of eks_sample_tv on scalar chains (EKS_FLAG_DIAG_MODEL): eks_sample under one process-noise scale
// per frame and one weight per observation (model, index conventions and lane bodies in eks_sample_tv_lane.hpp).  No
// reference counterpart.  eks_sample's seven launches:
//   P1 sample_tv_summarize : lane = (chain, chunk of B frames): the chunk's filter element under (r_eff, q_i)
//                            (reads y, var, weights, w)
//   S1 kalman scan x3      : eks_chain.hip's chain_scan (composing, applying and pulling back elements never sees Q)
//   P2 sample_beta_tv      : lane = (chain, chunk): filtered variances, (G_t, sd_t) in registers, Gamma once and beta
//                            for every draw (reads var, weights, w)
//   S2 draw scan x3        : eks_sample.hip's three kernels, launched from here as they are
//   P3 sample_replay_tv    : lane = (chain, chunk): filter + RTS means in registers once, then every draw walks the
//                            registers backwards and streams ms + e out (reads y, var, weights, w)
// y is read twice and var, weights and w three times per CALL whatever n_draws is.  Workspace: eks_sample's planes
// (chain_layout with n_draws); every plane is written by an earlier launch of the same call before it is read.
// General models: eks_sample_dense.hip, dense_sample_tv.
#include <hip/hip_runtime.h>

#include "eks_chain_plan.hpp"
#include "eks_internal.hpp"
#include "eks_sample_tv_lane.hpp"

namespace eks {

// S2: defined in eks_sample.hip
__global__ void sample_draw_reduce_kernel(SampleWs W);
__global__ void sample_draw_scan_kernel(SampleWs W);
__global__ void sample_draw_apply_kernel(SampleWs W);

template <int B, bool UNIT, bool HAS_W>
__global__ __launch_bounds__(256) void sample_tv_summarize_kernel(ChainMap L, SampleWs W, DiagModel M, SampleTvCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  sample_tv_summarize_lane<B, UNIT, HAS_W>(W, M, c, n, j);
}

template <int B, bool UNIT, bool INJ, bool HAS_W>
__global__ __launch_bounds__(256) void sample_beta_tv_kernel(ChainMap L, SampleWs W, DiagModel M, SampleTvCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  sample_beta_tv_lane<B, UNIT, INJ, HAS_W>(W, M, c, n, j);
}

template <int B, bool UNIT, bool INJ, bool HAS_W>
__global__ __launch_bounds__(256) void sample_replay_tv_kernel(ChainMap L, SampleWs W, DiagModel M, SampleTvCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  sample_replay_tv_lane<B, UNIT, INJ, HAS_W>(W, M, c, n, j);
}

// f(std::bool_constant<b>{}) with b as a compile-time constant
template <typename F>
static void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// eks_sample's launch-index limits (EKS_OK) or EKS_ERR_SHAPE; host arithmetic only
int diag_sample_tv_check(int T, int N, int n_draws) {
  const ChainGeometry g = chain_geometry(T, kChainChunk);
  return (size_t)n_draws * g.ng * N >= (1u << 30) || !diag_chain_covers(T, N) ? EKS_ERR_SHAPE : EKS_OK;
}

int diag_sample_tv(const eks_dims_t& d, const float* y, const float* var, const float* qscale, int per_keypoint,
                   const float* weights, const DiagModel& M, int n_draws, uint64_t seed, int first_keypoint,
                   int first_draw, const float* noise, float* ms, float* draws, void* ws, size_t ws_bytes,
                   hipStream_t st) {
  const int T = d.n_frames, N = d.n_keypoints * d.state_dim;
  if (ws_bytes < diag_sample_workspace_bytes(T, N, n_draws)) return EKS_ERR_WORKSPACE;
  const int rc = diag_sample_tv_check(T, N, n_draws);
  if (rc != EKS_OK) return rc;
  const ChainPlan P = chain_plan(T, N, n_draws, false, ws);
  const SampleWs& W = P.W;
  const dim3 grid(P.blocks), block(256);
  const ChainMap& L = P.L;
  const SampleTvCall c{y, var, qscale, weights, noise, ms, draws, T, d.n_keypoints, per_keypoint ? 1 : 0,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)first_keypoint * (uint32_t)d.state_dim,
                       (uint32_t)first_draw};
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0, inj = noise != nullptr, has_w = weights != nullptr;
  constexpr int B = kChainChunk;
  const unsigned dgN = (unsigned)(((size_t)n_draws * W.ng * N + 255) / 256);
  {
    ProfScope ps("sample_tv_summarize", st);
    with_bool(unit, [&](auto u) {
      with_bool(has_w, [&](auto w) {
        hipLaunchKernelGGL((sample_tv_summarize_kernel<B, u.value, w.value>), grid, block, 0, st, L, W, M, c);
      });
    });
  }
  const int rs = chain_scan(P, M, "sample_tv_kalman_scan", st);
  if (rs != EKS_OK) return rs;
  {
    ProfScope ps("sample_beta_tv", st);
    with_bool(unit, [&](auto u) {
      with_bool(inj, [&](auto i) {
        with_bool(has_w, [&](auto w) {
          hipLaunchKernelGGL((sample_beta_tv_kernel<B, u.value, i.value, w.value>), grid, block, 0, st, L, W, M, c);
        });
      });
    });
  }
  {
    ProfScope ps("sample_tv_draw_scan", st);
    hipLaunchKernelGGL(sample_draw_reduce_kernel, dim3(dgN), dim3(256), 0, st, W);
    hipLaunchKernelGGL(sample_draw_scan_kernel, dim3((unsigned)(((size_t)n_draws * N + 63) / 64)), dim3(64), 0, st, W);
    hipLaunchKernelGGL(sample_draw_apply_kernel, dim3(dgN), dim3(256), 0, st, W);
  }
  {
    ProfScope ps("sample_replay_tv", st);
    with_bool(unit, [&](auto u) {
      with_bool(inj, [&](auto i) {
        with_bool(has_w, [&](auto w) {
          hipLaunchKernelGGL((sample_replay_tv_kernel<B, u.value, i.value, w.value>), grid, block, 0, st, L, W, M, c);
        });
      });
    });
  }
  return hip_status(hipGetLastError());
}

}  // namespace eks
