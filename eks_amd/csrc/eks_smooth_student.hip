// gfx950 kernels and the one driver of the four Student-t smoothers on scalar chains (EKS_FLAG_DIAG_MODEL):
// eks_smooth_robust (Student-t weights on the observations), eks_smooth_robust_group (one weight per group of g
// consecutive coordinates of a keypoint), eks_smooth_jumps (Student-t scales on the process noise, one per keypoint and
// frame) and eks_smooth_heavy (both at once).  Each is n_iters Gaussian smoothing passes with a closed-form update of
// its planes between them (models and formulas: the four lane headers; the pass: eks_smooth_student_lane.hpp).  No
// reference counterpart.  Every pass is the five-launch form of eks_smooth_tv, a middle pass up to two launches more:
//   1 *_summarize           : lane = (chain, chunk of B frames): the chunk's filter element under r / lam and s q w
//                             (reads y, var, lam, w).  jumps: eks_smooth_tv's summarize body on the scale plane
//   S kalman scan x3        : eks_chain.hip's chain_scan, as it is
//   3 *_replay              : lane = (chain, chunk): filter in registers, fuse, RTS backwards.  The last pass streams
//                             ms and Vs out and updates nothing, so the planes returned are the ones ms, Vs were
//                             smoothed under, bit for bit.  A middle pass has no output code:
//       robust_replay         forms delta and stores the new weights in place (reads y, var, lam; writes lam)
//       robust_group_replay   stores delta_{t,d} into the [T][N] contribution plane (reads y, var, lam)
//       jumps_replay          stores delta_{t,d} of every step into the [T][N] contribution plane (reads y, var, w)
//       heavy_replay          one RTS loop does both: delta_{t,d} into the contribution plane, lam_new in place
//                             (reads y, var, lam, w; writes lam, contrib)
//   4 robust_group_combine  : lane = (frame, keypoint, group): sums the g contributions in float64, writes lam into the
//                             weight plane - the one launch that changes it - and max-es |lam_new - lam_old| into change
//   4 jumps_combine         : (jumps, heavy) lane = (frame, keypoint): sums the D contributions, writes the new w into
//                             the scale plane - the one launch that changes it - and max-es |u_new - u_old| into change
// eks_smooth_jumps' last pass is eks_smooth_tv itself on the plane (diag_smooth_tv: five launches).  All launches of a
// call are enqueued back to back; nothing comes back to the host between passes.  A call's first pass without input
// weights compiles without the weight loads and does not read the plane.  Without a scale plane the frames run
// eks_smooth_tv's bodies at w = 1, read from a [T] vector of ones in the workspace (eks_smooth_student_lane.hpp says
// why).  The windowed replay of eks_smooth is never taken.  General models: eks_dense.hip, dense_smooth_robust,
// dense_smooth_jumps, dense_smooth_heavy; jumps_combine also serves them, with one float64 contribution per keypoint.
// eks_smooth_heavy_fit is the same driver with the M-step for s behind every middle pass' updates: one launch of
// eks_smooth_heavy_fit.hip (heavy_fit) that reads the contribution and the scale plane once more.
#include <hip/hip_runtime.h>

#include "eks_chain_plan.hpp"
#include "eks_internal.hpp"
#include "eks_smooth_student_lane.hpp"

namespace eks {

// eks_smooth_robust: y and r of the chunk stay in registers for the weight update (-DEKS_ROBUST_RELOAD: the A/B build
// that loads them again in the backward pass; DESIGN.md 9i has both register counts and the reason for the choice)
#ifdef EKS_ROBUST_RELOAD
constexpr bool kRobustKeep = false;
#else
constexpr bool kRobustKeep = true;
#endif

template <int B, bool UNIT, bool HAS_LAM, ObsSide OBS, bool PROC>
__global__ __launch_bounds__(256) void student_summarize_kernel(ChainMap L, SampleWs W, DiagModel M, StudentCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  student_summarize_lane<B, UNIT, HAS_LAM, OBS, PROC>(W, M, c, n, j);
}

template <int B, bool UNIT>
__global__ __launch_bounds__(256) void jumps_summarize_kernel(ChainMap L, SampleWs W, DiagModel M, SmoothTvCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  smooth_tv_summarize_lane<B, UNIT>(W, M, c, n, j);
}

template <int B, bool UNIT, bool HAS_LAM, ObsSide OBS, bool PROC>
__global__ __launch_bounds__(256) void student_replay_kernel(ChainMap L, SampleWs W, DiagModel M, StudentCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  student_replay_lane<B, UNIT, HAS_LAM, OBS, PROC, (OBS == kObsInPlace && !PROC) ? kRobustKeep : true>(W, M, c, n, j);
}

template <int B, bool UNIT, int VS_ROW, bool HAS_LAM, ObsSide OBS, bool PROC>
__global__ __launch_bounds__(256) void student_last_kernel(ChainMap L, SampleWs W, DiagModel M, StudentCall c) {
  int n, j;
  if (!chain_coords(L, W.N, W.nc, n, j)) return;
  student_last_lane<B, UNIT, VS_ROW, HAS_LAM, OBS, PROC>(W, M, c, n, j);
}

// The changes of a combine launch over rows FIRST .. rows - 1 of a [rows][cols] plane, columns along the wave, into
// change[]: lane(row, col, k) does the update of one entry and returns its change and the keypoint k it belongs to.
// K <= 64: a block holds at least four lanes of every keypoint, and their changes meet in LDS before one atomic per
// keypoint and block reaches change[] (jumps, K = 4: 64 times fewer; the first launch's atomics, all against a zero,
// cost 0.33 ms of a 1.6 ms call without it).  Wider sessions have few lanes of a keypoint per block and gain nothing
// from it (K = 256: 0.127 ms per launch either way), so their lanes go to change[] directly, behind
// robust_change_max's plain load.  SLOTS >= 64 words of LDS, the first K used, and FIRST are compile-time: each kernel
// keeps the LDS it was measured with and its instructions in the order they had.
template <int SLOTS, int FIRST, typename Lane>
__device__ __forceinline__ void combine_changes(float* change, int K, int rows, int cols, Lane&& lane) {
  __shared__ unsigned smax[SLOTS];
  const bool in_lds = change && K <= 64;   // uniform over the grid
  if (in_lds) {
    if (SLOTS >= 256 || threadIdx.x < SLOTS) smax[threadIdx.x] = 0u;
    __syncthreads();
  }
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < (long)(rows - FIRST) * cols) {
    int k;
    const float ch = lane((int)(idx / cols) + FIRST, (int)(idx % cols), k);
    if (in_lds) atomicMax(&smax[k], __float_as_uint(ch));
    else if (change) robust_change_max(change + k, ch);
  }
  if (in_lds) {
    __syncthreads();
    if ((int)threadIdx.x < K && smax[threadIdx.x] != 0u)
      robust_change_max(change + threadIdx.x, __uint_as_float(smax[threadIdx.x]));
  }
}

// lane = (frame, column of the weight plane), columns along the wave: whole rows of the plane, g adjacent floats of
// the contribution row each
__global__ __launch_bounds__(256) void robust_group_combine_kernel(const float* __restrict__ contrib, int g, float* lam,
                                                                  float* change, int T, int NG, int per_keypoint,
                                                                  int K, double nu, int has_lam) {
  combine_changes<64, 0>(change, K, T, NG, [&](int t, int q, int& k) {
    k = q / per_keypoint;
    return robust_group_combine_lane(contrib, g, lam, NG, t, q, nu, has_lam);
  });
}

// lane = (frame 1 .. T-1, keypoint), keypoints along the wave: whole rows of the scale plane
template <typename C>
__global__ __launch_bounds__(256) void jumps_combine_kernel(const C* __restrict__ contrib, int nd, float* scales,
                                                           float* change, int T, int K, double nu, double nu_d) {
  combine_changes<256, 1>(change, K, T, K, [&](int t, int col, int& k) {
    k = col;
    return jumps_combine_lane<C>(contrib, nd, scales, K, t, k, nu, nu_d);
  });
}

int jumps_combine(const void* contrib, bool f64, int nd, float* scales, float* change, int T, int K, double nu,
                  int D, hipStream_t st) {
  if (T < 2) return EKS_OK;
  const long lanes = (long)(T - 1) * K;
  const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
  ProfScope ps("jumps_combine", st);
  if (f64)
    hipLaunchKernelGGL(jumps_combine_kernel<double>, grid, block, 0, st, static_cast<const double*>(contrib), nd, scales,
                       change, T, K, nu, nu + (double)D);
  else
    hipLaunchKernelGGL(jumps_combine_kernel<float>, grid, block, 0, st, static_cast<const float*>(contrib), nd, scales,
                       change, T, K, nu, nu + (double)D);
  return hip_status(hipGetLastError());
}

// the scale plane a call works on: ones everywhere, or (scales_in) the caller's values with row 0 set to 1
int jumps_init_plane(float* plane, int T, int K, int scales_in, float* change, hipStream_t st) {
  const size_t n = scales_in ? (size_t)K : (size_t)T * (size_t)K;
  hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(plane), 0x3f800000, n, st);   // 1.0f
  if (e == hipSuccess && change) e = hipMemsetAsync(change, 0, (size_t)K * sizeof(float), st);
  return hip_status(e);
}

// what an entry point is, beyond <OBS, PROC>
struct StudentSpec {
  const char *summarize, *scan, *replay, *combine;   // the profile's scope names (combine: kObsGrouped's)
  int g;                       // coordinates per weight (1 unless kObsGrouped)
  double nu_obs, nu_proc;
  float* weights;              // the caller's planes, or null: the workspace's
  int weights_in;
  float* scales;
  int scales_in;
  float* change;               // [K] per updated side, observations first; or null
};

// one pass: summarize, scan, replay
template <bool UNIT, bool HAS_LAM, ObsSide OBS, bool PROC>
static int launch_student_pass(const StudentSpec& s, bool last, int vs_row, const ChainPlan& E, const DiagModel& M,
                               const StudentCall& c, hipStream_t st) {
  const dim3 grid(E.blocks), block(256);
  {
    ProfScope ps(s.summarize, st);
    if constexpr (OBS == kObsFixed)
      hipLaunchKernelGGL((jumps_summarize_kernel<kChainChunk, UNIT>), grid, block, 0, st, E.L, E.W, M,
                         SmoothTvCall{c.y, c.var, c.scales, nullptr, nullptr, c.T, c.K, 1});
    else
      hipLaunchKernelGGL((student_summarize_kernel<kChainChunk, UNIT, HAS_LAM, OBS, PROC>), grid, block, 0, st, E.L, E.W,
                         M, c);
  }
  const int rc = chain_scan(E, M, s.scan, st);
  if (rc != EKS_OK) return rc;
  ProfScope ps(s.replay, st);
  if constexpr (OBS != kObsFixed) {   // kObsFixed: the last pass is diag_smooth_tv
    if (last) {
      with_vs_row(vs_row, [&](auto r) {
        hipLaunchKernelGGL((student_last_kernel<kChainChunk, UNIT, decltype(r)::value, HAS_LAM, OBS, PROC>), grid, block,
                           0, st, E.L, E.W, M, c);
      });
      return EKS_OK;
    }
  }
  hipLaunchKernelGGL((student_replay_kernel<kChainChunk, UNIT, HAS_LAM, OBS, PROC>), grid, block, 0, st, E.L, E.W, M, c);
  return EKS_OK;
}

// the UNIT x HAS_LAM selection
template <ObsSide OBS, bool PROC>
static int select_student_pass(const StudentSpec& s, bool unit, bool has_lam, bool last, int vs_row, const ChainPlan& E,
                               const DiagModel& M, const StudentCall& c, hipStream_t st) {
  if constexpr (OBS != kObsFixed) {
    if (has_lam)
      return unit ? launch_student_pass<true, true, OBS, PROC>(s, last, vs_row, E, M, c, st)
                  : launch_student_pass<false, true, OBS, PROC>(s, last, vs_row, E, M, c, st);
  }
  return unit ? launch_student_pass<true, false, OBS, PROC>(s, last, vs_row, E, M, c, st)
              : launch_student_pass<false, false, OBS, PROC>(s, last, vs_row, E, M, c, st);
}

// The workspace: eks_em_stats' (its float64 plane stays unused), then the tail - the weight plane [T][lam_cols], the
// scale source ([T][K] plane, or the [T] vector of ones) and the [T][N] contribution plane, each on 256 bytes and
// absent at 0 columns.  The planes are there whether or not the caller passes planes of their own.  Offsets from the
// workspace's start.
struct StudentLayout {
  size_t lam, scales, contrib, total;
};
static StudentLayout student_layout(int T, int N, int lam_cols, int scale_cols, int contrib_cols) {
  const auto plane = [T](int cols) { return align_up((size_t)T * (size_t)cols * sizeof(float), 256); };
  StudentLayout l;
  l.lam = align_up(diag_em_workspace_bytes(T, N), 256);
  l.scales = l.lam + plane(lam_cols);
  l.contrib = l.scales + plane(scale_cols);
  l.total = l.contrib + plane(contrib_cols);
  return l;
}
template <ObsSide OBS, bool PROC>
static StudentLayout student_layout(int T, int K, int D, int g) {
  const int N = K * D;
  return student_layout(T, N, OBS == kObsFixed ? 0 : N / g, PROC ? K : 1, OBS == kObsGrouped || PROC ? N : 0);
}

// fit: eks_smooth_heavy_fit's M-step for s behind every middle pass' updates (eks_smooth_heavy_fit.hip), or null.  With
// it change is [3][K] - weights, scales, log s - whatever OBS is, and a Gaussian process side (nu_proc = +inf) skips
// the combine launch: its plane of ones is already there.
template <ObsSide OBS, bool PROC>
static int student_smooth(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M,
                          const StudentSpec& s, int n_iters, float* ms, float* Vs, void* ws, size_t ws_bytes,
                          hipStream_t st, const HeavyFit* fit = nullptr) {
  static_assert(!(OBS == kObsGrouped && PROC), "one contribution plane: a pass stores either side's delta into it");
  const int T = d.n_frames, K = d.n_keypoints, D = d.state_dim, N = K * D, NG = N / s.g;
  int rc = diag_smooth_tv_check(d);
  if (rc != EKS_OK) return rc;
  const StudentLayout lay = student_layout<OBS, PROC>(T, K, D, s.g);
  if (ws_bytes < lay.total + (fit ? heavy_fit_part_bytes(T, K) : 0)) return EKS_ERR_WORKSPACE;
  const ChainPlan E = chain_plan(T, N, 0, true, ws);
  char* base = static_cast<char*>(ws);
  float* lam = s.weights ? s.weights : reinterpret_cast<float*>(base + lay.lam);
  float* scales = s.scales ? s.scales : reinterpret_cast<float*>(base + lay.scales);
  float* contrib = reinterpret_cast<float*>(base + lay.contrib);
  {
    hipError_t e = hipSuccess;
    if constexpr (PROC) rc = jumps_init_plane(scales, T, K, s.scales_in, nullptr, st);
    else e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(scales), 0x3f800000, (size_t)T, st);   // 1.0f
    if (rc != EKS_OK) return rc;
    // a single pass without input weights smooths under ones and returns them; a group's weight has no owning lane
    // (student_last_lane), so it is set here
    if (OBS == kObsGrouped && e == hipSuccess && n_iters == 1 && !s.weights_in)
      e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(lam), 0x3f800000, (size_t)T * (size_t)NG, st);
    if (e == hipSuccess && s.change)
      e = hipMemsetAsync(s.change, 0, (size_t)(fit ? 3 : (OBS != kObsFixed) + PROC) * (size_t)K * sizeof(float), st);
    if (e != hipSuccess) return hip_status(e);
    if (fit) rc = heavy_fit_begin(base + lay.total, T, K, st);
    if (rc != EKS_OK) return rc;
  }
  const bool unit = (d.flags & EKS_FLAG_UNIT_AC) != 0;
  const int vs_row = (d.flags & EKS_FLAG_VS_DIAG) ? 0 : D;
  for (int it = 0; it < n_iters; ++it) {
    const bool last = it == n_iters - 1, has_lam = OBS != kObsFixed && (it > 0 || s.weights_in);
    // eks_smooth_tv itself on the plane: the scales returned are the ones ms, Vs were smoothed under, bit for bit
    if (OBS == kObsFixed && last) return diag_smooth_tv(d, y, var, scales, 1, M, ms, Vs, ws, ws_bytes, st);
    // change: the last update of either plane is that of the pass before the last
    float* ch = it == n_iters - 2 ? s.change : nullptr;
    float* ch_proc = ch && (OBS != kObsFixed || fit) ? ch + K : ch;
    const StudentCall c{y, var, lam, scales, contrib, ch, ms, Vs, T, K, (float)s.nu_obs, (float)(s.nu_obs + 1.0),
                        (float)((s.nu_obs + 1.0) / s.nu_obs), NG, s.g};
    rc = select_student_pass<OBS, PROC>(s, unit, has_lam, last, vs_row, E, M, c, st);
    if (rc != EKS_OK) return rc;
    if (last) break;
    if constexpr (OBS == kObsGrouped) {
      const long lanes = (long)T * NG;
      ProfScope ps(s.combine, st);
      hipLaunchKernelGGL(robust_group_combine_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, contrib,
                         s.g, lam, ch, T, NG, D / s.g, K, s.nu_obs, has_lam ? 1 : 0);
    }
    if constexpr (PROC) {
      if (!(fit && fit->proc_gauss)) {
        rc = jumps_combine(contrib, false, D, scales, ch_proc, T, K, s.nu_proc, D, st);
        if (rc != EKS_OK) return rc;
      }
      if (fit) {
        rc = heavy_fit_step(contrib, false, D, scales, T, K, D, fit->lo, fit->hi, base + lay.total, fit->s,
                            s.change ? s.change + 2 * K : nullptr, st);
        if (rc != EKS_OK) return rc;
      }
    }
  }
  return hip_status(hipGetLastError());
}

size_t diag_smooth_robust_workspace_bytes(int T, int N) { return student_layout<kObsInPlace, false>(T, N, 1, 1).total; }
size_t diag_smooth_robust_group_workspace_bytes(int T, int N, int g) {
  return student_layout<kObsGrouped, false>(T, N, 1, g).total;
}
size_t diag_smooth_jumps_workspace_bytes(int T, int K, int D) {
  return student_layout<kObsFixed, true>(T, K, D, 1).total;
}
size_t diag_smooth_heavy_workspace_bytes(int T, int K, int D) {
  return student_layout<kObsInPlace, true>(T, K, D, 1).total;
}

int diag_smooth_robust(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, double nu, int n_iters,
                       float* weights, int weights_in, float* change, float* ms, float* Vs, void* ws, size_t ws_bytes,
                       hipStream_t st) {
  const StudentSpec s{"robust_summarize", "robust_scan", "robust_replay", nullptr, 1, nu, 0.0, weights, weights_in,
                      nullptr, 0, change};
  return student_smooth<kObsInPlace, false>(d, y, var, M, s, n_iters, ms, Vs, ws, ws_bytes, st);
}

int diag_smooth_robust_group(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, double nu,
                             int g, int n_iters, float* weights, int weights_in, float* change, float* ms, float* Vs,
                             void* ws, size_t ws_bytes, hipStream_t st) {
  const StudentSpec s{"robust_group_summarize", "robust_group_scan", "robust_group_replay", "robust_group_combine", g,
                      nu, 0.0, weights, weights_in, nullptr, 0, change};
  return student_smooth<kObsGrouped, false>(d, y, var, M, s, n_iters, ms, Vs, ws, ws_bytes, st);
}

int diag_smooth_jumps(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, double nu, int n_iters,
                      float* scales, int scales_in, float* change, float* ms, float* Vs, void* ws, size_t ws_bytes,
                      hipStream_t st) {
  const StudentSpec s{"jumps_summarize", "jumps_scan", "jumps_replay", nullptr, 1, 1.0, nu, nullptr, 0, scales,
                      scales_in, change};
  return student_smooth<kObsFixed, true>(d, y, var, M, s, n_iters, ms, Vs, ws, ws_bytes, st);
}

int diag_smooth_heavy(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, double nu_obs,
                      double nu_proc, int n_iters, float* weights, float* scales, int planes_in, float* change,
                      float* ms, float* Vs, void* ws, size_t ws_bytes, hipStream_t st) {
  const StudentSpec s{"heavy_summarize", "heavy_scan", "heavy_replay", nullptr, 1, nu_obs, nu_proc, weights,
                      planes_in & 1, scales, planes_in & 2, change};
  return student_smooth<kObsInPlace, true>(d, y, var, M, s, n_iters, ms, Vs, ws, ws_bytes, st);
}

// eks_smooth_heavy_fit on scalar chains: the driver above with the M-step for s.  A finite nu_obs runs the heavy
// kernels, nu_obs = +inf eks_smooth_jumps' (no weight plane; the caller's, if any, comes back as ones).  The size is the
// wider of the two layouts plus the fit's region ([slabs][K] partial sums, tile tickets), whatever the nu.
size_t diag_smooth_heavy_fit_workspace_bytes(int T, int K, int D) {
  return student_layout<kObsInPlace, true>(T, K, D, 1).total + heavy_fit_part_bytes(T, K);
}

int diag_smooth_heavy_fit(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, double* s_out,
                          double nu_obs, double nu_proc, int n_iters, double lo, double hi, float* weights,
                          float* scales, int planes_in, float* change, float* ms, float* Vs, void* ws, size_t ws_bytes,
                          hipStream_t st) {
  const HeavyFit fit{s_out, lo, hi, !(nu_proc <= 1.7e308)};
  if (nu_obs <= 1.7e308) {
    const StudentSpec s{"heavy_summarize", "heavy_scan", "heavy_replay", nullptr, 1, nu_obs, nu_proc, weights,
                        planes_in & 1, scales, planes_in & 2, change};
    return student_smooth<kObsInPlace, true>(d, y, var, M, s, n_iters, ms, Vs, ws, ws_bytes, st, &fit);
  }
  if (ws_bytes < diag_smooth_heavy_fit_workspace_bytes(d.n_frames, d.n_keypoints, d.state_dim)) return EKS_ERR_WORKSPACE;
  if (weights) {
    const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(weights), 0x3f800000,
                                           (size_t)d.n_frames * (size_t)d.n_keypoints * (size_t)d.state_dim, st);   // 1.0f
    if (e != hipSuccess) return hip_status(e);
  }
  const StudentSpec s{"jumps_summarize", "jumps_scan", "jumps_replay", nullptr, 1, 1.0, nu_proc, nullptr, 0, scales,
                      planes_in & 2, change};
  return student_smooth<kObsFixed, true>(d, y, var, M, s, n_iters, ms, Vs, ws, ws_bytes, st, &fit);
}

}  // namespace eks
