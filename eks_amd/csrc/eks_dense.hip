// gfx950 kernels for the general (D, O) smoother: multicam linear path, D = n_latent (3..6),
// O = 2 * n_cameras (reference eks/multicam_smoother.py:409-443), and the pupil smoother's final
// pass (D = 3, O = 8).  Same three-phase chunked scan as the scalar-chain path, with float64 small
// matrices in registers; chunk elements are built predict-first (eks_dense_lane.hpp):
//   D1 dense_summarize : lane = (keypoint, chunk) -> element (A, b, C, eta, J); chunk 0's lane also
//                        updates the prior with frame 0 (the belief the scan starts from)
//   D2 dense_scan_*    : block-parallel scan of the chunk elements (general element composition
//                        through Cholesky / Woodbury forms, eks_dense_math.hpp delem_combine);
//                        forward and reverse scans run side by side in one workgroup
//   D3 dense_replay    : lane = (keypoint, chunk): exact filter, fuse, RTS; filtered beliefs go
//                        through a per-lane scratch record stream (these problems are tiny:
//                        BASELINE config 4 is 4 keypoints x 50k frames, latency- not HBM-bound)
// Seven more features run D1 -> D2 -> a replay kernel of their own on this organisation (increments, tv, robust, jumps,
// heavy, EM statistics, innovations).  Their host side is written once: checks, layout and tail (DensePass, dense_pass_begin,
// dense_generic_workspace_bytes) and the launches (dense_prelude, dense_tv_prelude, dense_pass_launch).  The kernels'
// opening lines are not shared, on measurement: DESIGN.md 9k.
// The losses of this path (eks_nll, eks_ar1_nll) live in eks_loss_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "eks_dense_lane.hpp"
#include "eks_em_lane.hpp"
#include "eks_increments_lane.hpp"
#include "eks_innov_lane.hpp"
#include "eks_internal.hpp"
#include "eks_smooth_heavy_lane.hpp"
#include "eks_smooth_jumps_lane.hpp"
#include "eks_smooth_robust_group_lane.hpp"
#include "eks_smooth_robust_lane.hpp"
#include "eks_smooth_tv_lane.hpp"

namespace eks {

struct DenseGeom {
  int K, T, O;
  int B, nc;      // frames per replay lane, number of replay chunks
  int Bs, ncs;    // frames per chunk ELEMENT (summarize / scan), number of elements; B % Bs == 0,
                  // (B / Bs) divides 64 so a replay chunk's elements never straddle a scan block
};

// Sweeps of the extended filter (eks_ekf_smooth) are enqueued without host round trips: a sweep's
// kernels return at once when the previous sweep already met the tolerance.
struct Gate {
  const double* resid;   // largest change of a linearisation point in the previous sweep, or null
  double tol;
  __device__ bool closed() const { return resid != nullptr && *resid <= tol; }
};

template <int D, typename Obs>
__global__ __launch_bounds__(64) void dense_summarize_kernel(DenseGeom G, DenseModelPtrs M,
                                                            const double* __restrict__ s, Obs obs,
                                                            double* __restrict__ elems,
                                                            double* __restrict__ first, Gate gate) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G.K * G.ncs || gate.closed()) return;
  const int k = idx % G.K, j = idx / G.K;
  Mat<double, D> F, sQ;
  bool fid;
  load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
  const int t0 = j * G.Bs, len = min(G.Bs, G.T - t0);
  const DElem<double, D> e = dense_smooth_element_obs<D>(obs, k, t0, len, F, sQ, fid);
  store_delem<double, D>(elems + (size_t)idx * delem_doubles<D>(), e);
  if (j == 0) {   // the belief the scan starts from: the prior updated with frame 0
    Vec<double, D> m;
    Mat<double, D> P;
    load_prior<D>(M, k, m, P);
    double xl[D];   // the extended filter linearises frame 0 at the prior mean
#pragma unroll
    for (int a = 0; a < D; ++a) xl[a] = m.a[a];
    belief_update_obs<D>(obs, k, 0, xl, m, P);
    dense_store_rec<D>(first + (size_t)k * (D + D * D), 1, m, P);
  }
}

// ---- scan of the chunk elements, block-parallel like the scalar path (eks_diag.hip K2):
//   DS1 scan   : block = (keypoint, 64 consecutive chunks), 128 threads: threads 0..63 run a
//                Hillis-Steele inclusive FORWARD scan of the block's elements in LDS while threads
//                64..127 run the inclusive REVERSE scan in a second LDS array (the two are
//                independent, so the depth is 6 compositions, not 12); both are written out per
//                chunk, the forward total is the block aggregate
//   DS2 blocks : per keypoint, the same two-sided scan over the block aggregates
//   (replay)   : each replay lane applies its exclusive prefix (the inclusive prefix of chunk i-1)
//                to the block's incoming belief and pulls the block's outgoing information back
//                through its exclusive suffix (the inclusive suffix of chunk i+1) - one apply and
//                one pull-back per lane instead of a third scan kernel.
constexpr int kDenseCB = 64;

template <int D>
__global__ __launch_bounds__(2 * kDenseCB) void dense_scan_kernel(DenseGeom G,
                                                                  const double* __restrict__ elems,
                                                                  double* __restrict__ pre,
                                                                  double* __restrict__ suf,
                                                                  double* __restrict__ agg, Gate gate) {
  constexpr int NV = delem_doubles<D>();
  __shared__ double lds[2 * kDenseCB * NV];
  if (gate.closed()) return;
  const int k = blockIdx.x, blk = blockIdx.y;
  const bool rev = threadIdx.x >= kDenseCB;
  const int i = threadIdx.x - (rev ? kDenseCB : 0);
  const int j = blk * kDenseCB + i;
  const bool live = j < G.ncs;
  double* mine = lds + (rev ? kDenseCB * NV : 0);
  DElem<double, D> e = live ? load_delem<double, D>(elems + ((size_t)j * G.K + k) * NV)
                            : delem_identity<double, D>();
  // records field-major in LDS (stride kDenseCB between fields: conflict-free; record-major rows of 34
  // doubles put every 8th lane on the same banks); the smoother's scans need no log-likelihood term
  store_delem<double, D>(mine + i, e, kDenseCB);
  __syncthreads();
  for (int off = 1; off < kDenseCB; off <<= 1) {
    const bool has = rev ? (i + off < kDenseCB) : (i >= off);
    DElem<double, D> other;
    if (has) other = load_delem<double, D>(mine + (rev ? i + off : i - off), kDenseCB);
    __syncthreads();
    if (has) e = rev ? delem_combine<double, D, false>(e, other) : delem_combine<double, D, false>(other, e);
    store_delem<double, D>(mine + i, e, kDenseCB);
    __syncthreads();
  }
  if (live) store_delem<double, D>((rev ? suf : pre) + ((size_t)j * G.K + k) * NV, e);
  if (!rev && i == kDenseCB - 1) store_delem<double, D>(agg + ((size_t)blk * G.K + k) * NV, e);
}

// DS2: one workgroup per keypoint scans the block aggregates the same way (threads 0..63 forward,
// 64..127 reverse), 64 aggregates per round with the running belief / information carried from
// round to round (the forward half walks the rounds upwards, the reverse half downwards).
template <int D>
__global__ __launch_bounds__(2 * kDenseCB) void dense_scan_blocks_kernel(DenseGeom G, int nblk,
                                                                         const double* __restrict__ first,
                                                                         const double* __restrict__ agg,
                                                                         double* __restrict__ bprior,
                                                                         double* __restrict__ bsuffix,
                                                                         Gate gate) {
  constexpr int REC = D + D * D;
  constexpr int NV = delem_doubles<D>();
  __shared__ double lds[2 * kDenseCB * NV];
  if (gate.closed()) return;
  const int k = blockIdx.x;
  const bool rev = threadIdx.x >= kDenseCB;
  const int i = threadIdx.x - (rev ? kDenseCB : 0);
  double* mine = lds + (rev ? kDenseCB * NV : 0);
  // every thread of a half carries its own copy of the running state (same arithmetic, same value)
  Vec<double, D> cv = vec_zero<double, D>();
  Mat<double, D> cM = mat_zero<double, D>();
  if (!rev) dense_load_rec<D>(first + (size_t)k * REC, 1, cv, cM);
  const int rounds = (nblk + kDenseCB - 1) / kDenseCB;
  for (int r = 0; r < rounds; ++r) {
    const int q = (rev ? rounds - 1 - r : r) * kDenseCB + i;
    const bool live = q < nblk;
    DElem<double, D> e = live ? load_delem<double, D>(agg + ((size_t)q * G.K + k) * NV)
                              : delem_identity<double, D>();
    store_delem<double, D>(mine + i, e, kDenseCB);
    __syncthreads();
    for (int off = 1; off < kDenseCB; off <<= 1) {
      const bool has = rev ? (i + off < kDenseCB) : (i >= off);
      DElem<double, D> other;
      if (has) other = load_delem<double, D>(mine + (rev ? i + off : i - off), kDenseCB);
      __syncthreads();
      if (has) e = rev ? delem_combine<double, D, false>(e, other) : delem_combine<double, D, false>(other, e);
      store_delem<double, D>(mine + i, e, kDenseCB);
      __syncthreads();
    }
    Vec<double, D> v = cv;
    Mat<double, D> Mx = cM;
    if (!rev) {
      if (i > 0) delem_apply(load_delem<double, D>(mine + (i - 1), kDenseCB), v, Mx);
      delem_apply(load_delem<double, D>(mine + (kDenseCB - 1), kDenseCB), cv, cM);
    } else {
      if (i + 1 < kDenseCB) delem_back(load_delem<double, D>(mine + (i + 1), kDenseCB), v, Mx);
      delem_back(load_delem<double, D>(mine, kDenseCB), cv, cM);
    }
    if (live) dense_store_rec<D>((rev ? bsuffix : bprior) + ((size_t)q * G.K + k) * REC, 1, v, Mx);
    __syncthreads();
  }
}

// What a replay lane starts from, for the lane of keypoint k whose frames are covered by the elements ea .. eb (the
// extended filter's half-chunk elements; one element, ea == eb == the chunk, everywhere else): (m, P) the filtered
// belief of the frame before element ea - the block's incoming belief through the exclusive prefix of ea inside its
// block of 64, or the prior itself for chunk 0, which replays frame 0's update - and (eta, J) what all frames after
// element eb say about its last frame - the block's outgoing information pulled back through the exclusive suffix of
// eb.  suf == bsuffix == nullptr (a forward-only kernel): eta and J are left alone.
template <int D>
__device__ __forceinline__ void dense_chunk_boundary(const DenseGeom& G, const DenseModelPtrs& M, int k, int ea, int eb,
                                                     const double* __restrict__ pre, const double* __restrict__ suf,
                                                     const double* __restrict__ bprior,
                                                     const double* __restrict__ bsuffix, Vec<double, D>& m,
                                                     Mat<double, D>& P, Vec<double, D>& eta, Mat<double, D>& J) {
  constexpr int REC = D + D * D;
  constexpr int NV = delem_doubles<D>();
  const int blk = ea / kDenseCB, ia = ea % kDenseCB, ib = eb % kDenseCB;
  dense_load_rec<D>(bprior + ((size_t)blk * G.K + k) * REC, 1, m, P);
  if (bsuffix) dense_load_rec<D>(bsuffix + ((size_t)blk * G.K + k) * REC, 1, eta, J);   // (both in flight together)
  if (ia > 0) delem_apply(load_delem<double, D>(pre + ((size_t)(ea - 1) * G.K + k) * NV), m, P);
  if (bsuffix && ib + 1 < kDenseCB && eb + 1 < G.ncs)
    delem_back(load_delem<double, D>(suf + ((size_t)(eb + 1) * G.K + k) * NV), eta, J);
  if (ea == 0) load_prior<D>(M, k, m, P);
}

template <int D, bool EKF, typename Obs, bool SCORE = false>
__global__ __launch_bounds__(64) void dense_replay_kernel(DenseGeom G, DenseModelPtrs M,
                                                         const double* __restrict__ s, Obs obs,
                                                         const double* __restrict__ pre,
                                                         const double* __restrict__ suf,
                                                         const double* __restrict__ bprior,
                                                         const double* __restrict__ bsuffix,
                                                         double* __restrict__ filt,
                                                         float* __restrict__ ms,
                                                         float* __restrict__ Vs, int vs_diag,
                                                         double* __restrict__ xlin,
                                                         double* __restrict__ ll_chunk,
                                                         double* __restrict__ resid, Gate gate) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G.K * G.nc || gate.closed()) return;
  constexpr int REC = D + D * D;
  const int k = idx % G.K, j = idx / G.K;
  Mat<double, D> F, sQ;
  bool fid;
  load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
  Vec<double, D> m, eta;
  Mat<double, D> P, J;
  // this lane's frames are covered by the elements ea .. eb (one element on the linear path)
  const int sub = G.B / G.Bs;
  const int ea = j * sub;
  dense_chunk_boundary<D>(G, M, k, ea, min(ea + sub - 1, G.ncs - 1), pre, suf, bprior, bsuffix, m, P, eta, J);
  const int t0 = j * G.B, len = min(G.B, G.T - t0);
  double ll = 0.0, ch = 0.0;
  dense_replay_chunk_obs<D, EKF, Obs, SCORE>(obs, G.K, k, t0, len, F, sQ, fid, m, P, eta, J,
                                             filt ? filt + (size_t)t0 * REC * G.K + k : nullptr, ms, Vs,
                                             vs_diag != 0, EKF ? xlin + ((size_t)k * G.T + t0) * D : nullptr, &ll,
                                             &ch, (size_t)G.K);
  if constexpr (SCORE) {                 // per-chunk partial sums, [chunk][keypoint]: ll_chunk, then resid as the score
    ll_chunk[idx] = ll;
    resid[idx] = ch;
  }
  if constexpr (EKF) {
    ll_chunk[idx] = ll;
    // non-negative doubles order like their bit patterns; a NaN (diverged linearisation) has the
    // largest pattern and keeps the following sweeps open
    atomicMax(reinterpret_cast<unsigned long long*>(resid),
              (unsigned long long)__double_as_longlong(ch != ch ? 1e300 : ch));
  }
}

// ------------------------------------------------------------------------------------------
constexpr int kDenseSmoothChunk = 32;   // frames per lane in the smoother (the scan is parallel)

// Frames per lane for a (T, K) problem.  Shorter chunks buy lanes and cut the sequential depth of
// summarize / replay; the two-level scan costs about the same up to 64 x 64 chunks per keypoint.
// Linear path: 16 frames while that does not oversubscribe the device (measured on BASELINE config
// 4, T = 50 000 x K = 4: 0.202 ms at 32, 0.148 at 16, 0.154 at 8), else 32.  Extended filter: 32
// (its sweeps converge chunk-wise: 16-frame chunks are shorter than the filter's memory and need
// 8+ sweeps where 32-frame chunks need 3).  EKS_DENSE_CHUNK overrides (measurement knob).
static int dense_chunk(int T, int K, bool ekf = false) {
  const int forced = knob_int(KNOB_DENSE_CHUNK, 0);
  if (forced >= 2 && forced <= 256) return forced;
  if (ekf) return kDenseSmoothChunk;
  return (long long)K * ((T + 15) / 16) <= (1 << 18) ? 16 : kDenseSmoothChunk;
}

// Which organisation a (T, K, D, O) smoothing problem takes, and its workspace:
//   wave : narrow sessions, eks_dense_wave.hip
//   runs : keypoint-major kernels with the per-lane scan, eks_dense_wide.hip - chunk elements, the belief /
//          information pair per chunk, the scan's upper levels, two partial sums per lane (SCORE form): no
//          per-frame stream (288 GB hold 50 000 frames x ~170 000 keypoints of D = 3 this way; the generic layout's
//          float64 filtered-belief stream alone would take 96 B per keypoint-frame)
//   else : the generic kernels (any D <= 6, O <= 64; also the keypoint-major kernels with the tree scan behind
//          EKS_DENSE_TREE_SCAN) with prefix / suffix elements per chunk and the filtered-belief stream
enum DensePath { kDenseWave, kDenseRuns, kDenseGeneric };
static DensePath dense_path(int T, int K, int D, int O) {
  if (dense_wave_covers(T, K, D, O)) return kDenseWave;
  if (dense_wide_covers(D, O, dense_chunk(T, K)) && !knob_int(KNOB_DENSE_TREE_SCAN, 0)) return kDenseRuns;
  return kDenseGeneric;
}
struct RunsLayout {
  double *elems, *chunk_in, *chunk_out, *scratch, *first, *part_ll, *part_score;
  size_t bytes;
};
static RunsLayout runs_layout(int K, int D, int nc, char* base) {
  const size_t nv = 3 * D * D + 2 * D + 1, rec = D + D * D;
  RunsLayout L;
  size_t off = 0;
  auto take = [&](size_t doubles) {
    double* p = reinterpret_cast<double*>(base + off);
    off += align_up(doubles * 8, 256);
    return p;
  };
  L.elems = take((size_t)nc * K * nv);
  L.chunk_in = take((size_t)nc * K * rec);
  L.chunk_out = take((size_t)nc * K * rec);
  L.scratch = take(dense_wide_scan_scratch_doubles(K, D, nc));
  L.first = take((size_t)K * rec);
  L.part_ll = take((size_t)nc * K);
  L.part_score = take((size_t)nc * K);
  L.bytes = off;
  return L;
}

struct GenericLayout {     // chunk elements, their inclusive prefix / suffix per chunk, block aggregates and
  double *elems, *pre, *suf, *agg, *bprior, *bsuffix, *filt, *first;   // boundaries, the filtered-belief stream
  size_t bytes;
};
static GenericLayout generic_layout(int T, int K, int D, int nc, char* base) {
  const size_t nv = 3 * D * D + 2 * D + 1, rec = D + D * D;
  const size_t nblk = (nc + kDenseCB - 1) / kDenseCB;
  GenericLayout L;
  size_t off = 0;
  auto take = [&](size_t doubles) {
    double* p = reinterpret_cast<double*>(base + off);
    off += align_up(doubles * 8, 256);
    return p;
  };
  L.elems = take((size_t)nc * K * nv);
  L.pre = take((size_t)nc * K * nv);
  L.suf = take((size_t)nc * K * nv);
  L.agg = take(nblk * K * nv);
  L.bprior = take(nblk * K * rec);
  L.bsuffix = take(nblk * K * rec);
  L.filt = take((size_t)T * K * rec);
  L.first = take((size_t)K * rec);
  L.bytes = off;
  return L;
}

// One element per replay chunk (every driver but the pinhole filter's half-chunk elements).
static DenseGeom dense_geom(int T, int K, int O, int B) {
  const int nc = (T + B - 1) / B;
  return DenseGeom{K, T, O, B, nc, B, nc};
}

// D2: both scan levels over the elements in L.elems.
template <int D>
static void dense_scan_launch(const DenseGeom& G, const GenericLayout& L, const Gate& gate, hipStream_t st) {
  const int nblk = (G.ncs + kDenseCB - 1) / kDenseCB;
  hipLaunchKernelGGL(dense_scan_kernel<D>, dim3(G.K, nblk), dim3(2 * kDenseCB), 0, st, G, L.elems, L.pre, L.suf, L.agg,
                     gate);
  hipLaunchKernelGGL(dense_scan_blocks_kernel<D>, dim3(G.K), dim3(2 * kDenseCB), 0, st, G, nblk, L.first, L.agg,
                     L.bprior, L.bsuffix, gate);
}

// D1 + D2, what every driver of the generic organisation runs before its own replay kernel: chunk elements of `obs`,
// then the scan, each under its profile scope (string literals: ProfScope keeps the pointer).
template <int D, typename Obs>
static void dense_prelude(const DenseGeom& G, const DenseModelPtrs& M, const double* s, const Obs& obs,
                          const GenericLayout& L, const Gate& gate, const char* summarize_scope,
                          const char* scan_scope, hipStream_t st) {
  {
    ProfScope ps(summarize_scope, st);
    hipLaunchKernelGGL((dense_summarize_kernel<D, Obs>), dim3((G.K * G.ncs + 63) / 64), dim3(64), 0, st, G, M, s,
                       obs, L.elems, L.first, gate);
  }
  ProfScope ps(scan_scope, st);
  dense_scan_launch<D>(G, L, gate, st);
}

// ---- the features that always take the generic organisation (correct first, like the dense sampler, whatever
// dense_path would pick for eks_smooth): increments, tv, robust, jumps, EM statistics, innovations ------------------
// Each is dense_pass_begin, dense_prelude and one dense_pass_launch of its replay kernel (that pair per iteration for
// the iterated ones); its workspace is the generic layout - with the filtered-belief stream over `filt_frames` frames:
// T, or 0 for a forward-only pass - and a tail of its own behind it.
static int dense_nc(int T, int K) {
  const int B = dense_chunk(T, K);
  return (T + B - 1) / B;
}
static size_t dense_plane_bytes(size_t count, size_t elem) { return align_up(count * elem, 256); }

// 0 where dense_pass_begin refuses the shape.
static size_t dense_generic_workspace_bytes(int filt_frames, int K, int D, int O, int T, size_t tail_bytes) {
  if (D < 1 || D > 6 || O < 1 || O > 64) return 0;
  const int nc = dense_nc(T, K);
  if ((long long)K * nc >= (1 << 30)) return 0;
  return generic_layout(filt_frames, K, D, nc, nullptr).bytes + tail_bytes;   // (the layout ends 256-aligned)
}

struct DensePass {
  DenseGeom G;
  DenseModelPtrs M;
  const double* s;
  GenericLayout L;
  int lanes;
  char* tail;       // the pass's own region behind the layout
};
static int dense_pass_begin(const eks_dims_t& d, const DenseModel& Mm, int filt_frames, size_t tail_bytes, void* ws,
                            size_t ws_bytes, DensePass& P) {
  const int T = d.n_frames, K = d.n_keypoints, D = d.state_dim, O = d.obs_dim;
  if (D < 1 || D > 6 || O < 1 || O > 64) return EKS_ERR_UNSUPPORTED;
  P.G = dense_geom(T, K, O, dense_chunk(T, K));
  if ((long long)K * P.G.nc >= (1 << 30)) return EKS_ERR_SHAPE;   // every launch indexes its threads with an int
  P.L = generic_layout(filt_frames, K, D, P.G.nc, static_cast<char*>(ws));
  if (ws_bytes < P.L.bytes + tail_bytes) return EKS_ERR_WORKSPACE;
  P.M = DenseModelPtrs{Mm.m0, Mm.S0, Mm.A, Mm.C, Mm.Q};
  P.s = Mm.s;
  P.lanes = K * P.G.nc;
  P.tail = static_cast<char*>(ws) + P.L.bytes;
  return EKS_OK;
}

// One launch of a replay kernel, lane = (keypoint, chunk), under its profile scope (a string literal: ProfScope keeps
// the pointer).  `args`: the kernel's arguments after (G, M, s).
template <typename... KArgs, typename... Args>
static void dense_pass_launch(const DensePass& P, const char* scope, hipStream_t st, void (*kernel)(KArgs...),
                              const Args&... args) {
  ProfScope ps(scope, st);
  kernel<<<dim3((P.lanes + 63) / 64), dim3(64), 0, st>>>(P.G, P.M, P.s, args...);
}
constexpr Gate kGateOpen{nullptr, 0.0};

size_t dense_smooth_workspace_bytes(int T, int K, int D, int O) {
  const int B = dense_chunk(T, K), nc = (T + B - 1) / B;
  switch (dense_path(T, K, D, O)) {
    case kDenseWave: return dense_wave_workspace_bytes(T, K, D);
    case kDenseRuns: return runs_layout(K, D, nc, nullptr).bytes;
    default: return generic_layout(T, K, D, nc, nullptr).bytes;
  }
}

int dense_smooth(const eks_dims_t& d, const float* y, const float* var, const DenseModel& Mm,
                 float* ms, float* Vs, void* ws, size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, K = d.n_keypoints, D = d.state_dim, O = d.obs_dim;
  if (D < 1 || D > 6 || O < 1 || O > 64) return EKS_ERR_UNSUPPORTED;
  if (ws_bytes < dense_smooth_workspace_bytes(T, K, D, O)) return EKS_ERR_WORKSPACE;
  // narrow sessions (configs[3]: 4 keypoints) are depth-bound: two launches with the scan in wave
  // shuffles and the filtered beliefs in LDS (eks_dense_wave.hip); wide ones stream keypoint-major
  const DensePath path = dense_path(T, K, D, O);
  if (path == kDenseWave) return dense_wave_smooth(d, y, var, Mm, ms, Vs, ws, ws_bytes, st);
  const DenseGeom G = dense_geom(T, K, O, dense_chunk(T, K));
  const DenseModelPtrs M{Mm.m0, Mm.S0, Mm.A, Mm.C, Mm.Q};
  if (path == kDenseRuns) {
    const RunsLayout L = runs_layout(K, D, G.nc, static_cast<char*>(ws));
    const int vs_diag = (d.flags & EKS_FLAG_VS_DIAG) ? 1 : 0;
    int rc;
    {
      ProfScope ps("dense_summarize", st);
      rc = dense_wide_summarize(T, K, D, O, G.B, G.nc, M, Mm.s, y, var, nullptr, L.elems, 1, L.first, st);
      if (rc != EKS_OK) return rc;
    }
    {
      ProfScope ps("dense_scan", st);
      rc = dense_wide_scan(K, D, G.nc, L.elems, L.first, L.scratch, L.chunk_in, L.chunk_out, st);
      if (rc != EKS_OK) return rc;
    }
    ProfScope ps("dense_replay", st);
    return dense_wide_replay(T, K, D, O, G.B, G.nc, M, Mm.s, y, var, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr, nullptr, L.chunk_in, L.chunk_out, ms, Vs, vs_diag, st);
  }
  const GenericLayout L = generic_layout(T, K, D, G.nc, static_cast<char*>(ws));
  const int lanes = K * G.nc;
  const int vs_diag = (d.flags & EKS_FLAG_VS_DIAG) ? 1 : 0;
  const Gate open{nullptr, 0.0};
  EKS_DISPATCH_D(D, {
    const LinearObs<DD> obs = make_linear_obs<DD>(y, var, K, O, M);
    if (dense_wide_covers(D, O, G.B)) {
      // (EKS_DENSE_TREE_SCAN: the keypoint-major summarize / replay around the tree scan of whole elements)
      int rc;
      {
        ProfScope ps("dense_summarize", st);
        rc = dense_wide_summarize(T, K, D, O, G.B, G.nc, M, Mm.s, y, var, nullptr, L.elems, 0, L.first, st);
        if (rc != EKS_OK) return rc;
      }
      {
        ProfScope ps("dense_scan", st);
        dense_scan_launch<DD>(G, L, open, st);
      }
      ProfScope ps("dense_replay", st);
      rc = dense_wide_replay(T, K, D, O, G.B, G.nc, M, Mm.s, y, var, nullptr, nullptr, nullptr, L.pre, L.suf, L.bprior,
                             L.bsuffix, nullptr, nullptr, ms, Vs, vs_diag, st);
      if (rc != EKS_OK) return rc;
    } else {
      dense_prelude<DD>(G, M, Mm.s, obs, L, open, "dense_summarize", "dense_scan", st);
      ProfScope ps("dense_replay", st);
      hipLaunchKernelGGL((dense_replay_kernel<DD, false, LinearObs<DD>>), dim3((lanes + 63) / 64), dim3(64), 0, st, G, M,
                         Mm.s, obs, L.pre, L.suf, L.bprior, L.bsuffix, L.filt, ms, Vs, vs_diag, nullptr, nullptr,
                         nullptr, open);
    }
  })
  return hip_status(hipGetLastError());
}

// ---- eks_smooth_increments: a replay that also emits lag1, dmean and dV (eks_increments_lane.hpp) -------------------
template <int D, typename Obs>
__global__ __launch_bounds__(64) void dense_increments_kernel(DenseGeom G, DenseModelPtrs M,
                                                             const double* __restrict__ s, Obs obs,
                                                             const double* __restrict__ pre,
                                                             const double* __restrict__ suf,
                                                             const double* __restrict__ bprior,
                                                             const double* __restrict__ bsuffix,
                                                             double* __restrict__ filt, DenseIncrementsOut out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G.K * G.nc) return;
  constexpr int REC = D + D * D;
  const int k = idx % G.K, j = idx / G.K;
  Mat<double, D> F, sQ;
  bool fid;
  load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
  Vec<double, D> m, eta;
  Mat<double, D> P, J;
  dense_chunk_boundary<D>(G, M, k, j, j, pre, suf, bprior, bsuffix, m, P, eta, J);   // one element per lane (Bs == B)
  const int t0 = j * G.B, len = min(G.B, G.T - t0);
  dense_increments_chunk<D, Obs>(obs, G.K, k, t0, len, F, sQ, fid, m, P, eta, J, filt + (size_t)t0 * REC * G.K + k, out,
                                 (size_t)G.K);
}

size_t dense_increments_workspace_bytes(int T, int K, int D, int O) {
  return dense_generic_workspace_bytes(T, K, D, O, T, 0);
}

int dense_increments(const eks_dims_t& d, const float* y, const float* var, const DenseModel& Mm, float* ms, float* Vs,
                     float* lag1, float* dmean, float* dV, void* ws, size_t ws_bytes, hipStream_t st) {
  DensePass P;
  const int rc = dense_pass_begin(d, Mm, d.n_frames, 0, ws, ws_bytes, P);
  if (rc != EKS_OK) return rc;
  const DenseIncrementsOut out{ms, Vs, lag1, dmean, dV, (d.flags & EKS_FLAG_VS_DIAG) != 0, d.n_frames};
  EKS_DISPATCH_D(d.state_dim, {
    const LinearObs<DD> obs = make_linear_obs<DD>(y, var, P.G.K, P.G.O, P.M);
    dense_prelude<DD>(P.G, P.M, P.s, obs, P.L, kGateOpen, "dense_increments_summarize", "dense_increments_scan", st);
    dense_pass_launch(P, "dense_increments_replay", st, dense_increments_kernel<DD, LinearObs<DD>>, obs, P.L.pre,
                      P.L.suf, P.L.bprior, P.L.bsuffix, P.L.filt, out);
  })
  return hip_status(hipGetLastError());
}

// ---- eks_smooth_tv: w_t s Q per frame in summarize and replay (eks_smooth_tv_lane.hpp: dense_tv_element,
// dense_tv_replay_chunk); the scan composes elements and never sees Q ------------------------------------------------
template <int D>
__global__ __launch_bounds__(64) void dense_tv_summarize_kernel(DenseGeom G, DenseModelPtrs M,
                                                               const double* __restrict__ s, LinearObs<D> obs,
                                                               const float* __restrict__ qscale, int per_keypoint,
                                                               double* __restrict__ elems, double* __restrict__ first) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G.K * G.ncs) return;
  const int k = idx % G.K, j = idx / G.K;
  Mat<double, D> F, sQ;
  bool fid;
  load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
  const DenseNoiseScale ns = per_keypoint ? DenseNoiseScale{qscale, G.K, k} : DenseNoiseScale{qscale, 1, 0};
  const int t0 = j * G.Bs, len = min(G.Bs, G.T - t0);
  const DElem<double, D> e = dense_tv_element<D>(obs, ns, k, t0, len, F, sQ, fid);
  store_delem<double, D>(elems + (size_t)idx * delem_doubles<D>(), e);
  if (j == 0) {   // the belief the scan starts from: the prior updated with frame 0 (no predict, no w)
    Vec<double, D> m;
    Mat<double, D> P;
    load_prior<D>(M, k, m, P);
    belief_update_obs<D>(obs, k, 0, nullptr, m, P);
    dense_store_rec<D>(first + (size_t)k * (D + D * D), 1, m, P);
  }
}

// dense_prelude under the scale plane qscale: [T] shared, or [T][K] per keypoint.
template <int D>
static void dense_tv_prelude(const DensePass& P, const LinearObs<D>& obs, const float* qscale, int per_keypoint,
                             const char* summarize_scope, const char* scan_scope, hipStream_t st) {
  dense_pass_launch(P, summarize_scope, st, dense_tv_summarize_kernel<D>, obs, qscale, per_keypoint, P.L.elems,
                    P.L.first);
  ProfScope ps(scan_scope, st);
  dense_scan_launch<D>(P.G, P.L, kGateOpen, st);
}

template <int D>
__global__ __launch_bounds__(64) void dense_tv_replay_kernel(DenseGeom G, DenseModelPtrs M,
                                                            const double* __restrict__ s, LinearObs<D> obs,
                                                            const float* __restrict__ qscale, int per_keypoint,
                                                            const double* __restrict__ pre,
                                                            const double* __restrict__ suf,
                                                            const double* __restrict__ bprior,
                                                            const double* __restrict__ bsuffix,
                                                            double* __restrict__ filt, float* __restrict__ ms,
                                                            float* __restrict__ Vs, int vs_diag) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G.K * G.nc) return;
  constexpr int REC = D + D * D;
  const int k = idx % G.K, j = idx / G.K;
  Mat<double, D> F, sQ;
  bool fid;
  load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
  const DenseNoiseScale ns = per_keypoint ? DenseNoiseScale{qscale, G.K, k} : DenseNoiseScale{qscale, 1, 0};
  Vec<double, D> m, eta;
  Mat<double, D> P, J;
  dense_chunk_boundary<D>(G, M, k, j, j, pre, suf, bprior, bsuffix, m, P, eta, J);   // one element per lane (Bs == B)
  const int t0 = j * G.B, len = min(G.B, G.T - t0);
  dense_tv_replay_chunk<D>(obs, ns, G.K, k, t0, len, F, sQ, fid, m, P, eta, J, filt + (size_t)t0 * REC * G.K + k, ms, Vs,
                           vs_diag != 0, (size_t)G.K);
}

size_t dense_smooth_tv_workspace_bytes(int T, int K, int D, int O) {
  return dense_generic_workspace_bytes(T, K, D, O, T, 0);
}

int dense_smooth_tv(const eks_dims_t& d, const float* y, const float* var, const float* qscale, int per_keypoint,
                    const DenseModel& Mm, float* ms, float* Vs, void* ws, size_t ws_bytes, hipStream_t st) {
  DensePass P;
  const int rc = dense_pass_begin(d, Mm, d.n_frames, 0, ws, ws_bytes, P);
  if (rc != EKS_OK) return rc;
  const int vs_diag = (d.flags & EKS_FLAG_VS_DIAG) ? 1 : 0, pk = per_keypoint ? 1 : 0;
  EKS_DISPATCH_D(d.state_dim, {
    const LinearObs<DD> obs = make_linear_obs<DD>(y, var, P.G.K, P.G.O, P.M);
    dense_tv_prelude<DD>(P, obs, qscale, pk, "dense_tv_summarize", "dense_tv_scan", st);
    dense_pass_launch(P, "dense_tv_replay", st, dense_tv_replay_kernel<DD>, obs, qscale, pk, P.L.pre, P.L.suf,
                      P.L.bprior, P.L.bsuffix, P.L.filt, ms, Vs, vs_diag);
  })
  return hip_status(hipGetLastError());
}

// ---- eks_smooth_robust: n_iters passes under r / lam ----------------------------------------------------------------
// The prelude runs on an observation source that divides r by lam[t][k][o] (eks_smooth_robust_lane.hpp: RobustObs); the
// replay updates the weights in place (middle passes) or writes ms, Vs (the last).  Tail: one [T][K][O] float plane of
// weights, used when the caller passes none.
template <int D>
__global__ __launch_bounds__(64) void dense_robust_replay_kernel(DenseGeom G, DenseModelPtrs M,
                                                                const double* __restrict__ s, RobustObs<D> obs,
                                                                float* lam, double nu, int last, float* change,
                                                                const double* __restrict__ pre,
                                                                const double* __restrict__ suf,
                                                                const double* __restrict__ bprior,
                                                                const double* __restrict__ bsuffix,
                                                                double* __restrict__ filt, float* __restrict__ ms,
                                                                float* __restrict__ Vs, int vs_diag) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G.K * G.nc) return;
  constexpr int REC = D + D * D;
  const int k = idx % G.K, j = idx / G.K;
  Mat<double, D> F, sQ;
  bool fid;
  load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
  Vec<double, D> m, eta;
  Mat<double, D> P, J;
  dense_chunk_boundary<D>(G, M, k, j, j, pre, suf, bprior, bsuffix, m, P, eta, J);   // one element per lane (Bs == B)
  const int t0 = j * G.B, len = min(G.B, G.T - t0);
  const double ch = dense_robust_replay_chunk<D>(obs, lam, nu, last != 0, k, t0, len, F, sQ, fid, m, P, eta, J,
                                                 filt + (size_t)t0 * REC * G.K + k, ms, Vs, vs_diag != 0, (size_t)G.K);
  if (change && !last) robust_change_max(change + k, (float)ch);
}

static size_t dense_robust_tail_bytes(int T, int K, int O) {
  return dense_plane_bytes((size_t)T * K * O, sizeof(float));
}
size_t dense_smooth_robust_workspace_bytes(int T, int K, int D, int O) {
  return dense_generic_workspace_bytes(T, K, D, O, T, dense_robust_tail_bytes(T, K, O));
}

// ---- eks_smooth_robust_group: dense_smooth_robust with one weight per group of g coordinates -------------------------
// The observation source reads lam[t][k][o / g] (eks_smooth_robust_group_lane.hpp: RobustGroupObs); the replay's emit
// step holds every delta_o of its keypoint and frame, sums them per group and writes lam[t][k][G] in place: no combine
// launch.  Tail: one [T][K][O / g] float plane of weights, used when the caller passes none.
template <int D>
__global__ __launch_bounds__(64) void dense_robust_group_replay_kernel(DenseGeom G, DenseModelPtrs M,
                                                                      const double* __restrict__ s,
                                                                      RobustGroupObs<D> obs, float* lam, double nu,
                                                                      int last, float* change,
                                                                      const double* __restrict__ pre,
                                                                      const double* __restrict__ suf,
                                                                      const double* __restrict__ bprior,
                                                                      const double* __restrict__ bsuffix,
                                                                      double* __restrict__ filt, float* __restrict__ ms,
                                                                      float* __restrict__ Vs, int vs_diag) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G.K * G.nc) return;
  constexpr int REC = D + D * D;
  const int k = idx % G.K, j = idx / G.K;
  Mat<double, D> F, sQ;
  bool fid;
  load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
  Vec<double, D> m, eta;
  Mat<double, D> P, J;
  dense_chunk_boundary<D>(G, M, k, j, j, pre, suf, bprior, bsuffix, m, P, eta, J);   // one element per lane (Bs == B)
  const int t0 = j * G.B, len = min(G.B, G.T - t0);
  const double ch = dense_robust_group_replay_chunk<D>(obs, lam, nu, last != 0, k, t0, len, F, sQ, fid, m, P, eta, J,
                                                       filt + (size_t)t0 * REC * G.K + k, ms, Vs, vs_diag != 0,
                                                       (size_t)G.K);
  if (change && !last) robust_change_max(change + k, (float)ch);
}

size_t dense_smooth_robust_group_workspace_bytes(int T, int K, int D, int O, int g) {
  return dense_generic_workspace_bytes(T, K, D, O, T, dense_robust_tail_bytes(T, K, O / g));
}

// One driver for both, on the observation source: RobustObs (g = 1) or RobustGroupObs.  They differ in how the source
// is made, in the plane's width O / g and in the replay kernel.
template <template <int> class Obs>
static int dense_smooth_robust_on(const eks_dims_t& d, const float* y, const float* var, const DenseModel& Mm, double nu,
                                  int g, int n_iters, float* weights, int weights_in, float* change, float* ms,
                                  float* Vs, void* ws, size_t ws_bytes, const char* summarize_scope,
                                  const char* scan_scope, const char* replay_scope, hipStream_t st) {
  constexpr bool kGrouped = std::is_same<Obs<1>, RobustGroupObs<1>>::value;
  const int T = d.n_frames, K = d.n_keypoints, O = d.obs_dim;
  DensePass P;
  const int rc = dense_pass_begin(d, Mm, T, dense_robust_tail_bytes(T, K, O / g), ws, ws_bytes, P);
  if (rc != EKS_OK) return rc;
  float* lam = weights ? weights : reinterpret_cast<float*>(P.tail);
  const int vs_diag = (d.flags & EKS_FLAG_VS_DIAG) ? 1 : 0;
  if (change) {
    const hipError_t e = hipMemsetAsync(change, 0, (size_t)K * sizeof(float), st);
    if (e != hipSuccess) return hip_status(e);
  }
  EKS_DISPATCH_D(d.state_dim, {
    for (int it = 0; it < n_iters; ++it) {
      const int last = it == n_iters - 1;
      const float* lam_in = (it > 0 || weights_in) ? lam : nullptr;
      Obs<DD> obs;
      if constexpr (kGrouped) obs = make_robust_group_obs<DD>(y, var, lam_in, K, O, g, P.M);
      else obs = make_robust_obs<DD>(y, var, lam_in, K, O, P.M);
      dense_prelude<DD>(P.G, P.M, P.s, obs, P.L, kGateOpen, summarize_scope, scan_scope, st);
      const auto replay = [&](auto kernel) {
        dense_pass_launch(P, replay_scope, st, kernel, obs, lam, nu, last, it == n_iters - 2 ? change : nullptr, P.L.pre,
                          P.L.suf, P.L.bprior, P.L.bsuffix, P.L.filt, ms, Vs, vs_diag);
      };
      if constexpr (kGrouped) replay(dense_robust_group_replay_kernel<DD>);
      else replay(dense_robust_replay_kernel<DD>);
    }
  })
  return hip_status(hipGetLastError());
}

int dense_smooth_robust(const eks_dims_t& d, const float* y, const float* var, const DenseModel& Mm, double nu,
                        int n_iters, float* weights, int weights_in, float* change, float* ms, float* Vs, void* ws,
                        size_t ws_bytes, hipStream_t st) {
  return dense_smooth_robust_on<RobustObs>(d, y, var, Mm, nu, 1, n_iters, weights, weights_in, change, ms, Vs, ws,
                                           ws_bytes, "dense_robust_summarize", "dense_robust_scan",
                                           "dense_robust_replay", st);
}

int dense_smooth_robust_group(const eks_dims_t& d, const float* y, const float* var, const DenseModel& Mm, double nu,
                              int g, int n_iters, float* weights, int weights_in, float* change, float* ms, float* Vs,
                              void* ws, size_t ws_bytes, hipStream_t st) {
  return dense_smooth_robust_on<RobustGroupObs>(d, y, var, Mm, nu, g, n_iters, weights, weights_in, change, ms, Vs, ws,
                                                ws_bytes, "dense_robust_group_summarize", "dense_robust_group_scan",
                                                "dense_robust_group_replay", st);
}

// ---- eks_smooth_jumps: n_iters passes of dense_smooth_tv's organisation under the scale plane -----------------------
// A middle pass: the prelude under the plane, a replay (eks_smooth_jumps_lane.hpp) that writes delta_t into a [T][K]
// float64 plane, and eks_smooth_student.hip's combine launch, the only one that changes the scales.  The last pass is
// dense_smooth_tv itself, on the front of the same workspace.  Tail: the [T][K] float scale plane (used when the caller
// passes none), then the delta plane.
template <int D>
__global__ __launch_bounds__(64) void dense_jumps_replay_kernel(DenseGeom G, DenseModelPtrs M,
                                                               const double* __restrict__ s, LinearObs<D> obs,
                                                               const float* __restrict__ scales,
                                                               const double* __restrict__ pre,
                                                               const double* __restrict__ suf,
                                                               const double* __restrict__ bprior,
                                                               const double* __restrict__ bsuffix,
                                                               double* __restrict__ filt, double* __restrict__ delta) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G.K * G.nc) return;
  constexpr int REC = D + D * D;
  const int k = idx % G.K, j = idx / G.K;
  Mat<double, D> F, sQ;
  bool fid;
  load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
  const DenseNoiseScale ns{scales, G.K, k};
  Vec<double, D> m, eta;
  Mat<double, D> P, J;
  dense_chunk_boundary<D>(G, M, k, j, j, pre, suf, bprior, bsuffix, m, P, eta, J);   // one element per lane (Bs == B)
  const int t0 = j * G.B, len = min(G.B, G.T - t0);
  dense_jumps_replay_chunk<D>(obs, ns, G.K, k, t0, len, F, sQ, fid, m, P, eta, J, filt + (size_t)t0 * REC * G.K + k,
                              delta, (size_t)G.K);
}

static size_t dense_jumps_scale_bytes(int T, int K) { return dense_plane_bytes((size_t)T * K, sizeof(float)); }
static size_t dense_jumps_tail_bytes(int T, int K) {
  return dense_jumps_scale_bytes(T, K) + dense_plane_bytes((size_t)T * K, sizeof(double));
}
size_t dense_smooth_jumps_workspace_bytes(int T, int K, int D, int O) {
  return dense_generic_workspace_bytes(T, K, D, O, T, dense_jumps_tail_bytes(T, K));
}

int dense_smooth_jumps(const eks_dims_t& d, const float* y, const float* var, const DenseModel& Mm, double nu,
                       int n_iters, float* scales, int scales_in, float* change, float* ms, float* Vs, void* ws,
                       size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, K = d.n_keypoints;
  DensePass P;
  int rc = dense_pass_begin(d, Mm, T, dense_jumps_tail_bytes(T, K), ws, ws_bytes, P);
  if (rc != EKS_OK) return rc;
  float* plane = scales ? scales : reinterpret_cast<float*>(P.tail);
  double* delta = reinterpret_cast<double*>(P.tail + dense_jumps_scale_bytes(T, K));
  rc = jumps_init_plane(plane, T, K, scales_in, change, st);
  if (rc != EKS_OK) return rc;
  EKS_DISPATCH_D(d.state_dim, {
    const LinearObs<DD> obs = make_linear_obs<DD>(y, var, K, P.G.O, P.M);
    for (int it = 0; it + 1 < n_iters; ++it) {
      dense_tv_prelude<DD>(P, obs, plane, 1, "dense_jumps_summarize", "dense_jumps_scan", st);
      dense_pass_launch(P, "dense_jumps_replay", st, dense_jumps_replay_kernel<DD>, obs, plane, P.L.pre, P.L.suf,
                        P.L.bprior, P.L.bsuffix, P.L.filt, delta);
      rc = jumps_combine(delta, true, 1, plane, it == n_iters - 2 ? change : nullptr, T, K, nu, DD, st);
      if (rc != EKS_OK) return rc;
    }
  })
  return dense_smooth_tv(d, y, var, plane, 1, Mm, ms, Vs, ws, ws_bytes, st);
}

// ---- eks_smooth_heavy: n_iters passes under r / lam AND the scale plane ---------------------------------------------
// dense_tv_summarize_kernel on RobustObs, the scan, a replay (eks_smooth_heavy_lane.hpp) that updates the weights in
// place and writes delta_t into a [T][K] float64 plane, and the combine launch; the last pass writes ms, Vs under both
// planes.  Tail: the [T][K][O] float weight plane and the [T][K] float scale plane (each used when the caller passes
// none), then the delta plane.
template <int D>
__global__ __launch_bounds__(64) void dense_heavy_summarize_kernel(DenseGeom G, DenseModelPtrs M,
                                                                  const double* __restrict__ s, RobustObs<D> obs,
                                                                  const float* __restrict__ scales,
                                                                  double* __restrict__ elems,
                                                                  double* __restrict__ first) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G.K * G.ncs) return;
  const int k = idx % G.K, j = idx / G.K;
  Mat<double, D> F, sQ;
  bool fid;
  load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
  const DenseNoiseScale ns{scales, G.K, k};
  const int t0 = j * G.Bs, len = min(G.Bs, G.T - t0);
  const DElem<double, D> e = dense_tv_element<D>(obs, ns, k, t0, len, F, sQ, fid);
  store_delem<double, D>(elems + (size_t)idx * delem_doubles<D>(), e);
  if (j == 0) {   // the belief the scan starts from: the prior updated with frame 0 (no predict, no w)
    Vec<double, D> m;
    Mat<double, D> P;
    load_prior<D>(M, k, m, P);
    belief_update_obs<D>(obs, k, 0, nullptr, m, P);
    dense_store_rec<D>(first + (size_t)k * (D + D * D), 1, m, P);
  }
}

template <int D>
__global__ __launch_bounds__(64) void dense_heavy_replay_kernel(DenseGeom G, DenseModelPtrs M,
                                                               const double* __restrict__ s, RobustObs<D> obs,
                                                               const float* scales, float* lam, double nu, int last,
                                                               float* change, const double* __restrict__ pre,
                                                               const double* __restrict__ suf,
                                                               const double* __restrict__ bprior,
                                                               const double* __restrict__ bsuffix,
                                                               double* __restrict__ filt, double* __restrict__ delta,
                                                               float* __restrict__ ms, float* __restrict__ Vs,
                                                               int vs_diag) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G.K * G.nc) return;
  constexpr int REC = D + D * D;
  const int k = idx % G.K, j = idx / G.K;
  Mat<double, D> F, sQ;
  bool fid;
  load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
  const DenseNoiseScale ns{scales, G.K, k};
  Vec<double, D> m, eta;
  Mat<double, D> P, J;
  dense_chunk_boundary<D>(G, M, k, j, j, pre, suf, bprior, bsuffix, m, P, eta, J);   // one element per lane (Bs == B)
  const int t0 = j * G.B, len = min(G.B, G.T - t0);
  const double ch = dense_heavy_replay_chunk<D>(obs, ns, lam, nu, last != 0, k, t0, len, F, sQ, fid, m, P, eta, J,
                                                filt + (size_t)t0 * REC * G.K + k, delta, ms, Vs, vs_diag != 0,
                                                (size_t)G.K);
  if (change && !last) robust_change_max(change + k, (float)ch);
}

static size_t dense_heavy_tail_bytes(int T, int K, int O) {
  return dense_robust_tail_bytes(T, K, O) + dense_jumps_tail_bytes(T, K);
}
size_t dense_smooth_heavy_workspace_bytes(int T, int K, int D, int O) {
  return dense_generic_workspace_bytes(T, K, D, O, T, dense_heavy_tail_bytes(T, K, O));
}

// fit: eks_smooth_heavy_fit's M-step for s behind every middle pass' updates (eks_smooth_heavy_fit.hip), or null; with
// it the tail ends with the fit's region (partial sums, tile tickets), change is [3][K] and a Gaussian process side skips the combine
static int dense_heavy_run(const eks_dims_t& d, const float* y, const float* var, const DenseModel& Mm, double nu_obs,
                           double nu_proc, int n_iters, float* weights, float* scales, int planes_in, float* change,
                           float* ms, float* Vs, void* ws, size_t ws_bytes, hipStream_t st, const HeavyFit* fit) {
  const int T = d.n_frames, K = d.n_keypoints, O = d.obs_dim;
  DensePass P;
  int rc = dense_pass_begin(d, Mm, T, dense_heavy_tail_bytes(T, K, O) + (fit ? heavy_fit_part_bytes(T, K) : 0), ws,
                            ws_bytes, P);
  if (rc != EKS_OK) return rc;
  char* fit_ws = P.tail + dense_heavy_tail_bytes(T, K, O);
  char* tail = P.tail;
  float* lam = weights ? weights : reinterpret_cast<float*>(tail);
  tail += dense_robust_tail_bytes(T, K, O);
  float* plane = scales ? scales : reinterpret_cast<float*>(tail);
  double* delta = reinterpret_cast<double*>(tail + dense_jumps_scale_bytes(T, K));
  rc = jumps_init_plane(plane, T, K, planes_in & 2, nullptr, st);
  if (rc != EKS_OK) return rc;
  if (change) {
    const hipError_t e = hipMemsetAsync(change, 0, (fit ? 3 : 2) * (size_t)K * sizeof(float), st);
    if (e != hipSuccess) return hip_status(e);
  }
  if (fit) rc = heavy_fit_begin(fit_ws, T, K, st);
  if (rc != EKS_OK) return rc;
  const int vs_diag = (d.flags & EKS_FLAG_VS_DIAG) ? 1 : 0;
  EKS_DISPATCH_D(d.state_dim, {
    for (int it = 0; it < n_iters; ++it) {
      const int last = it == n_iters - 1;
      float* ch = it == n_iters - 2 ? change : nullptr;
      const RobustObs<DD> obs = make_robust_obs<DD>(y, var, (it > 0 || (planes_in & 1)) ? lam : nullptr, K, O, P.M);
      dense_pass_launch(P, "dense_heavy_summarize", st, dense_heavy_summarize_kernel<DD>, obs, plane, P.L.elems,
                        P.L.first);
      {
        ProfScope ps("dense_heavy_scan", st);
        dense_scan_launch<DD>(P.G, P.L, kGateOpen, st);
      }
      dense_pass_launch(P, "dense_heavy_replay", st, dense_heavy_replay_kernel<DD>, obs, plane, lam, nu_obs, last, ch,
                        P.L.pre, P.L.suf, P.L.bprior, P.L.bsuffix, P.L.filt, delta, ms, Vs, vs_diag);
      if (!last && !(fit && fit->proc_gauss)) {
        rc = jumps_combine(delta, true, 1, plane, ch ? ch + K : nullptr, T, K, nu_proc, DD, st);
        if (rc != EKS_OK) return rc;
      }
      if (!last && fit) {
        rc = heavy_fit_step(delta, true, 1, plane, T, K, DD, fit->lo, fit->hi, fit_ws, fit->s,
                            change ? change + 2 * K : nullptr, st);
        if (rc != EKS_OK) return rc;
      }
    }
  })
  return hip_status(hipGetLastError());
}

int dense_smooth_heavy(const eks_dims_t& d, const float* y, const float* var, const DenseModel& Mm, double nu_obs,
                       double nu_proc, int n_iters, float* weights, float* scales, int planes_in, float* change,
                       float* ms, float* Vs, void* ws, size_t ws_bytes, hipStream_t st) {
  return dense_heavy_run(d, y, var, Mm, nu_obs, nu_proc, n_iters, weights, scales, planes_in, change, ms, Vs, ws,
                         ws_bytes, st, nullptr);
}

// eks_smooth_heavy_fit on general models: nu_obs finite (the entry refuses +inf), nu_proc finite or +inf; Mm.s == s_out
size_t dense_smooth_heavy_fit_workspace_bytes(int T, int K, int D, int O) {
  const size_t base = dense_smooth_heavy_workspace_bytes(T, K, D, O);
  return base ? base + heavy_fit_part_bytes(T, K) : 0;
}

int dense_smooth_heavy_fit(const eks_dims_t& d, const float* y, const float* var, const DenseModel& Mm, double* s_out,
                           double nu_obs, double nu_proc, int n_iters, double lo, double hi, float* weights,
                           float* scales, int planes_in, float* change, float* ms, float* Vs, void* ws, size_t ws_bytes,
                           hipStream_t st) {
  const HeavyFit fit{s_out, lo, hi, !(nu_proc <= 1.7e308)};
  return dense_heavy_run(d, y, var, Mm, nu_obs, nu_proc, n_iters, weights, scales, planes_in, change, ms, Vs, ws,
                         ws_bytes, st, &fit);
}

// ---- eks_em_stats: dense_increments' organisation with the outputs replaced by a sum --------------------------------
// The replay accumulates the chunk's share of Sw = sum_t E[w_t w_t^T | y] in float64 (eks_em_lane.hpp: dense_em_chunk),
// then eks_em.hip's fixed-order reduce.  Tail: the [chunk][keypoint] plane of D x D (or D, with VS_DIAG) partials.
template <int D, typename Obs>
__global__ __launch_bounds__(64) void dense_em_kernel(DenseGeom G, DenseModelPtrs M, const double* __restrict__ s,
                                                     Obs obs, const double* __restrict__ pre,
                                                     const double* __restrict__ suf,
                                                     const double* __restrict__ bprior,
                                                     const double* __restrict__ bsuffix, double* __restrict__ filt,
                                                     double* __restrict__ part, int diag) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G.K * G.nc) return;
  constexpr int REC = D + D * D;
  const int k = idx % G.K, j = idx / G.K;
  Mat<double, D> F, sQ;
  bool fid;
  load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
  Vec<double, D> m, eta;
  Mat<double, D> P, J;
  dense_chunk_boundary<D>(G, M, k, j, j, pre, suf, bprior, bsuffix, m, P, eta, J);   // one element per lane (Bs == B)
  const int t0 = j * G.B, len = min(G.B, G.T - t0);
  const int w = diag ? D : D * D;
  dense_em_chunk<D, Obs>(obs, k, t0, len, F, sQ, fid, m, P, eta, J, filt + (size_t)t0 * REC * G.K + k, (size_t)G.K,
                         part + (size_t)idx * w, diag != 0);
}

static size_t dense_em_tail_bytes(int T, int K, int D) {
  return dense_plane_bytes((size_t)dense_nc(T, K) * K * D * D, sizeof(double));
}
size_t dense_em_workspace_bytes(int T, int K, int D, int O) {
  return dense_generic_workspace_bytes(T, K, D, O, T, dense_em_tail_bytes(T, K, D));
}

int dense_em_stats(const eks_dims_t& d, const float* y, const float* var, const DenseModel& Mm, double* Sw, void* ws,
                   size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, K = d.n_keypoints, D = d.state_dim;
  DensePass P;
  const int rc = dense_pass_begin(d, Mm, T, dense_em_tail_bytes(T, K, D), ws, ws_bytes, P);
  if (rc != EKS_OK) return rc;
  double* part = reinterpret_cast<double*>(P.tail);
  const int diag = (d.flags & EKS_FLAG_VS_DIAG) ? 1 : 0;
  EKS_DISPATCH_D(D, {
    const LinearObs<DD> obs = make_linear_obs<DD>(y, var, K, P.G.O, P.M);
    dense_prelude<DD>(P.G, P.M, P.s, obs, P.L, kGateOpen, "dense_em_summarize", "dense_em_scan", st);
    dense_pass_launch(P, "dense_em_replay", st, dense_em_kernel<DD, LinearObs<DD>>, obs, P.L.pre, P.L.suf, P.L.bprior,
                      P.L.bsuffix, P.L.filt, part, diag);
  })
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_status(e);
  // partials [chunk][keypoint][w]: column (k, entry) of the reduce is Sw's own flat index
  return em_reduce(part, P.G.nc, K * (diag ? D : D * D), Sw, st);
}

// ---- eks_innovations: dense_em's organisation, forward only ---------------------------------------------------------
// The replay walks every chunk forwards from the belief that entered it (eks_innov_lane.hpp: dense_innov_chunk):
// innovations, their variances, nis and the frame's log-likelihood stream out; then eks_em.hip's fixed-order reduce.
// No filtered-belief stream.  Tail: the chunks' log-likelihoods [chunk][keypoint].
template <int D, typename Obs>
__global__ __launch_bounds__(64) void dense_innov_kernel(DenseGeom G, DenseModelPtrs M, const double* __restrict__ s,
                                                        Obs obs, const double* __restrict__ pre,
                                                        const double* __restrict__ bprior, DenseInnovOut out,
                                                        double* __restrict__ part) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G.K * G.nc) return;
  const int k = idx % G.K, j = idx / G.K;
  Mat<double, D> F, sQ;
  bool fid;
  load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
  Vec<double, D> m, eta;
  Mat<double, D> P, J;
  dense_chunk_boundary<D>(G, M, k, j, j, pre, nullptr, bprior, nullptr, m, P, eta, J);   // forward boundary only
  const int t0 = j * G.B, len = min(G.B, G.T - t0);
  const double ll = dense_innov_chunk<D, Obs>(obs, G.K, G.O, k, t0, len, F, sQ, fid, m, P, out);
  if (part) part[idx] = ll;
}

static size_t dense_innov_tail_bytes(int T, int K) {
  return dense_plane_bytes((size_t)dense_nc(T, K) * K, sizeof(double));
}
size_t dense_innovations_workspace_bytes(int T, int K, int D, int O) {
  return dense_generic_workspace_bytes(0, K, D, O, T, dense_innov_tail_bytes(T, K));
}

int dense_innovations(const eks_dims_t& d, const float* y, const float* var, const DenseModel& Mm, float* innov,
                      float* innov_var, float* nis, float* frame_ll, double* loglik, void* ws, size_t ws_bytes,
                      hipStream_t st) {
  const int T = d.n_frames, K = d.n_keypoints;
  DensePass P;
  const int rc = dense_pass_begin(d, Mm, 0, dense_innov_tail_bytes(T, K), ws, ws_bytes, P);
  if (rc != EKS_OK) return rc;
  double* part = loglik ? reinterpret_cast<double*>(P.tail) : nullptr;
  const DenseInnovOut out{innov, innov_var, nis, frame_ll};
  EKS_DISPATCH_D(d.state_dim, {
    const LinearObs<DD> obs = make_linear_obs<DD>(y, var, K, P.G.O, P.M);
    dense_prelude<DD>(P.G, P.M, P.s, obs, P.L, kGateOpen, "dense_innov_summarize", "dense_innov_scan", st);
    dense_pass_launch(P, "dense_innov_replay", st, dense_innov_kernel<DD, LinearObs<DD>>, obs, P.L.pre, P.L.bprior, out,
                      part);
  })
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_status(e);
  if (!loglik) return EKS_OK;
  return em_reduce(part, P.G.nc, K, loglik, st);   // partials [chunk][keypoint]
}

// ---- SCORE form: the optimiser's loss and its derivative from the smoother's own kernels ---------------
// nll[k], d nll / d log s [k] of the constant-R filter loss at Mm.s[k] (eks/core.py:640-652), for Q positive
// definite: the value from the exact filter inside the replay kernels, the derivative from the smoothing
// distribution (Fisher's identity; eks_dense_wave.hip has the formula).  Narrow sessions take the wave kernels,
// wider ones the keypoint-major kernels with the per-lane scan; other shapes have no SCORE form (the caller keeps
// the dual-number kernels of eks_loss.hip).
bool dense_score_covers(int T, int K, int D, int O) {
  (void)K;
  return T >= 2 && D >= 1 && D <= 6 && O >= 1 && O <= 64 && !knob_int(KNOB_DENSE_DUAL_GRAD, 0);
}
size_t dense_score_workspace_bytes(int T, int K, int D, int O) { return dense_smooth_workspace_bytes(T, K, D, O); }
int dense_score(const eks_dims_t& d, const float* y, const double* rconst, const DenseModel& Mm, double* nll,
                double* dnll, void* ws, size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, K = d.n_keypoints, D = d.state_dim, O = d.obs_dim;
  if (!dense_score_covers(T, K, D, O)) return EKS_ERR_UNSUPPORTED;
  if (ws_bytes < dense_score_workspace_bytes(T, K, D, O)) return EKS_ERR_WORKSPACE;
  const DensePath path = dense_path(T, K, D, O);
  if (path == kDenseWave) return dense_wave_score(d, y, rconst, Mm, nll, dnll, ws, ws_bytes, st);
  const int B = dense_chunk(T, K), nc = (T + B - 1) / B;
  const DenseModelPtrs M{Mm.m0, Mm.S0, Mm.A, Mm.C, Mm.Q};
  if (path == kDenseGeneric) {
    // any D <= 6, O <= 64: the generic kernels with constant variances (layout of dense_smooth: prefix / suffix
    // elements per chunk, the filtered-belief stream; per-chunk partial sums where the chunk elements were - they
    // are dead once the scan has run)
    const DenseGeom G = dense_geom(T, K, O, B);
    const GenericLayout L = generic_layout(T, K, D, nc, static_cast<char*>(ws));
    double* part_ll = L.elems;
    double* part_score = L.elems + (size_t)nc * K;
    const int lanes = K * nc;
    const Gate open{nullptr, 0.0};
    EKS_DISPATCH_D(D, {
      const ConstLinearObs<DD> obs = make_const_linear_obs<DD>(y, rconst, K, O, M);
      dense_prelude<DD>(G, M, Mm.s, obs, L, open, "dense_score_summarize", "dense_score_scan", st);
      ProfScope ps("dense_score_replay", st);
      hipLaunchKernelGGL((dense_replay_kernel<DD, false, ConstLinearObs<DD>, true>), dim3((lanes + 63) / 64), dim3(64),
                         0, st, G, M, Mm.s, obs, L.pre, L.suf, L.bprior, L.bsuffix, L.filt, nullptr, nullptr, 0,
                         nullptr, part_ll, part_score, open);
    })
    const int rc0 = hip_status(hipGetLastError());
    if (rc0 != EKS_OK) return rc0;
    return dense_score_finish(K, nc, part_ll, part_score, nll, dnll, st);
  }
  const RunsLayout L = runs_layout(K, D, nc, static_cast<char*>(ws));
  int rc;
  {
    ProfScope ps("dense_score_summarize", st);
    rc = dense_wide_summarize(T, K, D, O, B, nc, M, Mm.s, y, nullptr, rconst, L.elems, 1, L.first, st);
    if (rc != EKS_OK) return rc;
  }
  {
    ProfScope ps("dense_score_scan", st);
    rc = dense_wide_scan(K, D, nc, L.elems, L.first, L.scratch, L.chunk_in, L.chunk_out, st);
    if (rc != EKS_OK) return rc;
  }
  {
    ProfScope ps("dense_score_replay", st);
    rc = dense_wide_replay(T, K, D, O, B, nc, M, Mm.s, y, nullptr, rconst, L.part_ll, L.part_score, nullptr, nullptr,
                           nullptr, nullptr, L.chunk_in, L.chunk_out, nullptr, nullptr, 0, st);
    if (rc != EKS_OK) return rc;
  }
  return dense_score_finish(K, nc, L.part_ll, L.part_score, nll, dnll, st);
}

// ---- extended Kalman filter / smoother with calibrated pinhole cameras ------------------------
// Reference: run_kalman_smoother(h_fn=...) (eks/core.py:188-190, :274-295) as driven by the
// calibrated branch of eks/multicam_smoother.py:369-407; D = 3, O = 2 * n_cams.
//
// The extended filter linearises frame t at its own predicted mean, which makes the recursion
// sequential in the reference.  Here it is solved as a fixed point instead: with linearisation
// points X fixed the model is a linear one with time-varying observation rows, which the chunked
// scan handles in parallel over (chain, chunk); the replay then runs the TRUE extended filter
// inside each chunk from the chunk's entry belief and writes its predicted means back as the new
// X.  At the fixed point (entry beliefs consistent with X) the result IS the sequential extended
// filter; every sweep makes at least one more chunk exact, in practice 2-4 sweeps reach 1e-10
// because the filter forgets its entry belief within a few frames.  Sweeps are gated on the
// device (Gate), so the whole solve is one enqueue without host round trips.
constexpr int kEkfMaxSweeps = 64;
// The replay lanes keep 32-frame chunks (the sweeps converge chunk-wise) but the chunk ELEMENTS are
// built over half chunks: twice the lanes and half the sequential depth in the summarize kernel.
constexpr int kEkfSub = 2;

__global__ __launch_bounds__(64) void ekf_finish_kernel(int K, int nc, int n_sweeps, double tol,
                                                       const double* __restrict__ ll_chunk,
                                                       const double* __restrict__ resid,
                                                       double* __restrict__ nll,
                                                       double* __restrict__ info) {
  const int k = blockIdx.x, i = threadIdx.x;
  double acc = 0.0;
  for (int j = i; j < nc; j += 64) acc += ll_chunk[(size_t)j * K + k];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (i == 0) {
    if (nll) nll[k] = -acc;
    if (k == 0 && info) {
      int ran = 1;
      while (ran < n_sweeps && !(resid[ran - 1] <= tol)) ++ran;
      info[0] = (double)ran;          // filter sweeps executed
      info[1] = resid[ran - 1];       // largest relative change of a linearisation point in the last
    }
  }
}

// the residual of the last filter sweep that ran (the slots of the sweeps gated after it are still zero) -> resid[slot]
__global__ void ekf_last_resid_kernel(int n_sweeps, double tol, double* __restrict__ resid, int slot) {
  int ran = 1;
  while (ran < n_sweeps && !(resid[ran - 1] <= tol)) ++ran;
  resid[slot] = resid[ran - 1];
}

static size_t ekf_ws_layout(int T, int K, bool smooth, double** ptrs, char* base) {
  constexpr int D = 3;
  const int B = dense_chunk(T, K, true), nc = (T + B - 1) / B;
  const int Bs = B % kEkfSub == 0 ? B / kEkfSub : B, ncs = (T + Bs - 1) / Bs;
  const int nblk = (ncs + kDenseCB - 1) / kDenseCB;
  const size_t nv = 3 * D * D + 2 * D + 1, rec = D + D * D;
  const size_t sizes[10] = {(size_t)ncs * K * nv * 8,  (size_t)ncs * K * nv * 8,
                            (size_t)ncs * K * nv * 8,  (size_t)nblk * K * nv * 8,
                            (size_t)nblk * K * rec * 8, (size_t)nblk * K * rec * 8,
                            smooth ? (size_t)T * K * rec * 8 : 0, (size_t)K * rec * 8,
                            (size_t)nc * K * 8,         (size_t)(kEkfMaxSweeps + 2) * 8};
  size_t off = 0;
  for (int i = 0; i < 10; ++i) {
    if (ptrs) ptrs[i] = reinterpret_cast<double*>(base + off);
    off += align_up(sizes[i], 256);
  }
  return off;
}

size_t ekf_smooth_workspace_bytes(int T, int K, int smooth) {
  return ekf_ws_layout(T, K, smooth != 0, nullptr, nullptr);
}

int ekf_smooth(const eks_dims_t& d, int n_data_keypoints, const float* y, const float* var,
               const double* rconst, const DenseModel& Mm, const double* cams, int n_cams,
               double* xlin, int max_sweeps, double tol, float* ms, float* Vs, double* nll,
               double* info, void* ws, size_t ws_bytes, hipStream_t st) {
  const int T = d.n_frames, K = d.n_keypoints, D = d.state_dim, O = d.obs_dim, Kd = n_data_keypoints;
  if (D != 3 || n_cams < 1 || O != 2 * n_cams || Kd < 1 || K % Kd != 0) return EKS_ERR_UNSUPPORTED;
  if (max_sweeps < 1 || max_sweeps > kEkfMaxSweeps) return EKS_ERR_SHAPE;
  if ((var == nullptr) == (rconst == nullptr)) return EKS_ERR_SHAPE;
  const bool smooth = ms != nullptr;
  if (ws_bytes < ekf_smooth_workspace_bytes(T, K, smooth)) return EKS_ERR_WORKSPACE;
  double* w[10];
  ekf_ws_layout(T, K, smooth, w, static_cast<char*>(ws));
  double *elems = w[0], *pre = w[1], *suf = w[2], *agg = w[3], *bprior = w[4], *bsuffix = w[5],
         *filt = w[6], *first = w[7], *ll_chunk = w[8], *resid = w[9];
  DenseGeom G{K, T, O, dense_chunk(T, K, true), 0, 0, 0};
  G.nc = (T + G.B - 1) / G.B;
  G.Bs = G.B % kEkfSub == 0 ? G.B / kEkfSub : G.B;
  G.ncs = (T + G.Bs - 1) / G.Bs;
  const int nblk = (G.ncs + kDenseCB - 1) / kDenseCB, lanes = K * G.nc, lanes_k1 = K * G.ncs;
  const DenseModelPtrs M{Mm.m0, Mm.S0, Mm.A, nullptr, Mm.Q};
  const PinholeObs obs{y, ObsNoise{var, rconst}, Kd, O, T, cams, xlin};
  const int vs_diag = (d.flags & EKS_FLAG_VS_DIAG) ? 1 : 0;
  const dim3 sgrid(K, nblk);
  hipError_t e = hipMemsetAsync(resid, 0, (kEkfMaxSweeps + 2) * 8, st);
  if (e != hipSuccess) return hip_status(e);
  // (build_gate: the element / scan kernels of the sweep; replay_gate: its replay)
  auto sweep = [&](const Gate& build_gate, const Gate& replay_gate, double* resid_out, bool with_smoother) {
    hipLaunchKernelGGL((dense_summarize_kernel<3, PinholeObs>), dim3((lanes_k1 + 63) / 64), dim3(64), 0,
                       st, G, M, Mm.s, obs, elems, first, build_gate);
    hipLaunchKernelGGL(dense_scan_kernel<3>, sgrid, dim3(2 * kDenseCB), 0, st, G, elems, pre, suf, agg,
                       build_gate);
    hipLaunchKernelGGL(dense_scan_blocks_kernel<3>, dim3(K), dim3(2 * kDenseCB), 0, st, G, nblk,
                       first, agg, bprior, bsuffix, build_gate);
    hipLaunchKernelGGL((dense_replay_kernel<3, true, PinholeObs>), dim3((lanes + 63) / 64), dim3(64),
                       0, st, G, M, Mm.s, obs, pre, suf, bprior, bsuffix, with_smoother ? filt : nullptr,
                       with_smoother ? ms : nullptr, Vs, vs_diag, xlin, ll_chunk, resid_out, replay_gate);
  };
  {
    ProfScope ps("ekf_filter_sweeps", st);
    for (int i = 0; i < max_sweeps; ++i) {
      const Gate g{i > 0 ? resid + i - 1 : nullptr, tol};
      sweep(g, g, resid + i, false);
    }
  }
  if (smooth) {
    // Once the filter sweeps have met the tolerance (the last sweep that ran moved no linearisation point by more
    // than tol; the slots of the sweeps gated after it are still zero) the elements, prefixes and suffixes in the
    // workspace ARE the converged ones - rebuilt at the new points they would differ by ~tol (1e-10 against 1e-5 bars) -
    // so the smoothing sweep is its replay alone (round 5: three launches and a third of a sweep's time less); it
    // rebuilds them only when the sweeps ran out unconverged.  The shortcut is for tight tolerances only: with a loose
    // caller tol (1e-2, say) "converged" points may still be 1e-2 from the elements in the workspace, so the rebuild is
    // skipped only below 1e-8.
    ProfScope ps("ekf_smooth_sweep", st);
    hipLaunchKernelGGL(ekf_last_resid_kernel, dim3(1), dim3(1), 0, st, max_sweeps, tol, resid, kEkfMaxSweeps + 1);
    sweep(Gate{resid + kEkfMaxSweeps + 1, tol < 1e-8 ? tol : 1e-8}, Gate{nullptr, 0.0}, resid + kEkfMaxSweeps, true);
  }
  hipLaunchKernelGGL(ekf_finish_kernel, dim3(K), dim3(64), 0, st, K, G.nc, max_sweeps, tol, ll_chunk,
                     resid, nll, info);
  return hip_status(hipGetLastError());
}

// ---- one sweep of the extended filter for a user-supplied emission function -----------------------
// Reference: run_kalman_smoother(h_fn=...) (eks/core.py:159-177, :188-190) for any differentiable h.  A kernel
// cannot call the user's (Python) function, so the host tabulates its linearisation at the points X of the
// sweep (AffineObs: J [T][K][O][D], c = h(X) - J X [T][K][O]) and this runs the linear time-varying filter of
// those tables on the generic kernels: elements, the two-level scan, then the replay, which writes the
// filter's predicted means back into xlin (the next sweep's X) and the largest relative change of a point.
// The host repeats tabulate + sweep until the change is below its tolerance (eks_amd/core.py); at that fixed
// point the result is the sequential extended filter.  With the tables fixed the scan is exact, so the number
// of sweeps does not depend on the frames per lane and the chunk length is chosen for the cost of a sweep.
static int affine_chunk(int T, int K) { return dense_chunk(T, K); }

// The generic layout (its filtered-belief stream only with the smoother) and two tail regions: the chunks'
// log-likelihoods and the sweep's largest change of a linearisation point.
struct AffineLayout {
  GenericLayout g;
  double *ll_chunk, *resid;
  size_t bytes;
};
static AffineLayout affine_layout(int T, int K, int D, bool smooth, char* base) {
  const int B = affine_chunk(T, K), nc = (T + B - 1) / B;
  AffineLayout L;
  L.g = generic_layout(smooth ? T : 0, K, D, nc, base);
  L.ll_chunk = reinterpret_cast<double*>(base + L.g.bytes);
  L.resid = reinterpret_cast<double*>(base + L.g.bytes + align_up((size_t)nc * K * 8, 256));
  L.bytes = L.g.bytes + align_up((size_t)nc * K * 8, 256) + align_up(8, 256);
  return L;
}

size_t ekf_affine_workspace_bytes(int T, int K, int D, int smooth) {
  return affine_layout(T, K, D, smooth != 0, nullptr).bytes;
}

__global__ __launch_bounds__(64) void affine_finish_kernel(int K, int nc, const double* __restrict__ ll_chunk,
                                                          const double* __restrict__ resid,
                                                          double* __restrict__ nll, double* __restrict__ change) {
  const int k = blockIdx.x, i = threadIdx.x;
  double acc = 0.0;
  for (int j = i; j < nc; j += 64) acc += ll_chunk[(size_t)j * K + k];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (i == 0) {
    if (nll) nll[k] = -acc;
    if (k == 0 && change) change[0] = resid[0];
  }
}

int ekf_affine_sweep(const eks_dims_t& d, int n_data_keypoints, const float* y, const float* var,
                     const double* rconst, const DenseModel& Mm, const double* jac, const double* off,
                     double* xlin, float* ms, float* Vs, double* nll, double* change, void* ws, size_t ws_bytes,
                     hipStream_t st) {
  const int T = d.n_frames, K = d.n_keypoints, D = d.state_dim, O = d.obs_dim, Kd = n_data_keypoints;
  if (D < 1 || D > 6 || O < 1 || O > 64 || Kd < 1 || K % Kd != 0) return EKS_ERR_UNSUPPORTED;
  if (jac == nullptr || off == nullptr) return EKS_ERR_SHAPE;
  if ((var == nullptr) == (rconst == nullptr)) return EKS_ERR_SHAPE;
  const bool smooth = ms != nullptr;
  if (ws_bytes < ekf_affine_workspace_bytes(T, K, D, smooth)) return EKS_ERR_WORKSPACE;
  const AffineLayout A = affine_layout(T, K, D, smooth, static_cast<char*>(ws));
  const GenericLayout& L = A.g;
  double *ll_chunk = A.ll_chunk, *resid = A.resid;
  const DenseGeom G = dense_geom(T, K, O, affine_chunk(T, K));
  const int lanes = K * G.nc;
  const DenseModelPtrs M{Mm.m0, Mm.S0, Mm.A, nullptr, Mm.Q};
  const int vs_diag = (d.flags & EKS_FLAG_VS_DIAG) ? 1 : 0;
  const Gate open{nullptr, 0.0};
  hipError_t e = hipMemsetAsync(resid, 0, 8, st);
  if (e != hipSuccess) return hip_status(e);
  EKS_DISPATCH_D(D, {
    const AffineObs<DD> obs = make_affine_obs<DD>(y, var, rconst, K, Kd, O, jac, off);
    dense_prelude<DD>(G, M, Mm.s, obs, L, open, "ekf_affine_summarize", "ekf_affine_scan", st);
    {
      ProfScope ps("ekf_affine_replay", st);
      hipLaunchKernelGGL((dense_replay_kernel<DD, true, AffineObs<DD>>), dim3((lanes + 63) / 64), dim3(64), 0, st, G,
                         M, Mm.s, obs, L.pre, L.suf, L.bprior, L.bsuffix, smooth ? L.filt : nullptr, ms, Vs, vs_diag,
                         xlin, ll_chunk, resid, open);
    }
  })
  hipLaunchKernelGGL(affine_finish_kernel, dim3(K), dim3(64), 0, st, K, G.nc, ll_chunk, resid, nll, change);
  return hip_status(hipGetLastError());
}

}  // namespace eks

EKS_DEFINE_TOUCH(dense)
