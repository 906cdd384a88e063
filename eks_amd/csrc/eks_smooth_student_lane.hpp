// The mean-field pass of the four Student-t smoothers on scalar chains (eks_smooth_student.hip), shared unchanged with
// tests/host_sim/{robust,robust_group,jumps,heavy}_sim.cpp (plain loops).  No reference counterpart.
//
// eks_smooth_robust, eks_smooth_robust_group, eks_smooth_jumps and eks_smooth_heavy run n_iters Gaussian smoothing
// passes - summarize, scan, replay - under a plane of observation weights lam (r_eff = clip_var(r / lam)), a plane of
// process-noise scales w (q_eff = s q w), or both, and between passes replace the planes in closed form from the pass's
// own smoothed posterior.  Models, formulas, accuracy limits and the helpers live where they were:
//   eks_smooth_robust_lane.hpp        lam per observation; robust_var, robust_weight, robust_change_max, the chunk loads
//   eks_smooth_robust_group_lane.hpp  lam per group of g coordinates; kGroupMissing, the combine lane
//   eks_smooth_jumps_lane.hpp         w per keypoint and frame; rts_step_jumps, load_chunk_scale, the combine lane
//   eks_smooth_heavy_lane.hpp         both at once, and why one pass may update both
// What differs between the four is what a pass READS and what a middle pass UPDATES; both are compile-time:
//   ObsSide  kObsFixed    no weight plane at all (eks_smooth_jumps)
//            kObsInPlace  lam [T][N], chain n its own column; a middle replay stores lam_new over the B frames it read,
//                         which no other lane of the launch touches (eks_smooth_robust, eks_smooth_heavy)
//            kObsGrouped  lam [T][N / g], chain n column n / g; the g chains of a group sit in different lanes, possibly
//                         in different blocks, so a middle replay stores delta_{t,d} into the [T][N] contribution plane
//                         (kGroupMissing where the frame's variance sits at the ceiling) and the combine launch that
//                         follows is the one that changes the weights (eks_smooth_robust_group)
//   PROC     false        the noise scale is the [T] vector of ones
//            true         w [T][K], chain n column n / D, read only; a middle replay stores rts_step_jumps' delta_{t,d}
//                         into the [T][N] contribution plane under the ownership rule - the step from frame t0 + i to
//                         t0 + i + 1 stores delta of frame t0 + i + 1, so the transition into the following chunk belongs
//                         to THIS chunk and the phantom step past frame T-1 stores nothing - and jumps_combine changes
//                         the scales (eks_smooth_jumps, eks_smooth_heavy)
// The last pass streams ms, Vs out and updates nothing: the planes returned are the ones the outputs were smoothed
// under.  eks_smooth_jumps' middle summarize is smooth_tv_summarize_lane and its last pass eks_smooth_tv itself.
#pragma once
#include "eks_smooth_heavy_lane.hpp"
#include "eks_smooth_robust_group_lane.hpp"

namespace eks {

enum ObsSide { kObsFixed, kObsInPlace, kObsGrouped };

struct StudentCall {
  const float *y, *var;
  float* lam;              // the weight plane, read (HAS_LAM); written in place by a kObsInPlace middle pass
  const float* scales;     // the scale source: PROC the [T][K] plane, else the [T] vector of 1.0f (see below)
  float* contrib;          // [T][N]: delta_{t,d} of a middle pass (kObsGrouped: rows 0 .. T-1; PROC: rows 1 .. T-1)
  float* change;           // [K]: max |lam_new - lam_old| of this pass (kObsInPlace), or null
  float *ms, *Vs;          // written by the last pass only
  int T, K;
  float nu, nu1, lam_max;  // nu_obs, nu_obs + 1 and (nu_obs + 1) / nu_obs, each rounded once from float64
  int lam_stride, lam_div; // kObsGrouped's weight view: N / g columns, chain n reads column n / g
};

// Without a scale plane the frames run eks_smooth_tv's bodies (load_chunk_noise, summarize_loaded_tv, filter_loaded_tv,
// rts_step on with_q) at the noise scale w = 1, read from a vector of ones like any other qscale.  The values are those
// of the constant-q bodies (q_s * 1.0f is exact); what the loads buy is eks_smooth_tv's BITS on the device.  With q_s a
// plain operand the compiler contracts `C rg + q_s` around C rg where eks_smooth_tv's `C rg + q_s w` is contracted
// around q_s w (UNIT chains: ms 1 - 1024 ulp apart, measured), and a single w passed as an argument is shared by all
// frames, which changes the multiply's use count and with it the same choice.  The loads hit one cache line per chunk.
template <bool PROC>
EKS_HD NoiseScale student_noise_scale(const StudentCall& c, int D, int n) {
  return PROC ? NoiseScale{c.scales, c.K, n / D, c.T} : NoiseScale{c.scales, 1, 0, c.T};
}

// the chunk's weights into registers.  The view is compile-time: the own-column forms read [t][n] of W.N columns as
// they always did - a division by a run-time 1 is twenty instructions - and only kObsGrouped divides.
template <int B, ObsSide OBS, bool FULL>
EKS_HD void student_load_weights(const StudentCall& c, int N, int n, int t0, int len, float (&lv)[B]) {
  if constexpr (OBS == kObsGrouped) load_chunk_weights<B, FULL>(c.lam, c.lam_stride, n / c.lam_div, t0, len, lv);
  else load_chunk_weights<B, FULL>(c.lam, N, n, t0, len, lv);
}

// T1: element of chunk j of chain n under r_eff and q_s w.  HAS_LAM == false (a call's first pass without input
// weights): lam is 1 and the plane is not read - summarize_loaded_tv on (y, var) itself.  The body is written out for
// FULL and not, as smooth_tv_summarize_lane's is: under the replays' forward(auto full) idiom every instantiation
// came out 60 instructions shorter and six of the twelve 1 - 2 VGPRs away from where they were measured.
template <int B, bool UNIT, bool HAS_LAM, ObsSide OBS, bool PROC>
EKS_HD void student_summarize_lane(const SampleWs& W, const DiagModel& M, const StudentCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const NoiseScale ns = student_noise_scale<PROC>(c, M.D, n);
  float yy[B], rr[B], lv[B], qv[B];
  Elem<float> e;
  if (len == B) {
    load_chunk<B, true>(c.y, c.var, W.N, n, t0, len, yy, rr);
    load_chunk_noise<B, true>(ns, t0, len, p.q_s, qv);
    if constexpr (HAS_LAM) {
      student_load_weights<B, OBS, true>(c, W.N, n, t0, len, lv);
      reweight_chunk<B, true>(rr, lv, len);
    }
    e = summarize_loaded_tv<B, UNIT, true>(yy, rr, qv, len, p);
  } else {
    load_chunk<B>(c.y, c.var, W.N, n, t0, len, yy, rr);
    load_chunk_noise<B>(ns, t0, len, p.q_s, qv);
    if constexpr (HAS_LAM) {
      student_load_weights<B, OBS, false>(c, W.N, n, t0, len, lv);
      reweight_chunk<B>(rr, lv, len);
    }
    e = summarize_loaded_tv<B, UNIT>(yy, rr, qv, len, p);
  }
  const size_t o = (size_t)j * W.N + n;
  W.eA[o] = e.A; W.eb[o] = e.b; W.eC[o] = e.C; W.eEta[o] = e.eta; W.eJ[o] = e.J;
}

// T3, last pass: replay of chunk j of chain n: filter in registers under r_eff and q_s w, fuse, RTS backwards; ms / Vs
// stream out through PointerStore and every plane stays.  Full chunks load and filter without per-frame predicates
// (DESIGN.md 9f); the backward pass is the predicated one.
template <int B, bool UNIT, int VS_ROW, bool HAS_LAM, ObsSide OBS, bool PROC>
EKS_HD void student_last_lane(const SampleWs& W, const DiagModel& M, const StudentCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const size_t o = (size_t)j * W.N + n;
  const NoiseScale ns = student_noise_scale<PROC>(c, M.D, n);
  float v0[B], v1[B], lv[B], qv[B];
  float m = W.pm[o], P = W.pP[o];
  auto forward = [&](auto full) {
    constexpr bool FULL = decltype(full)::value;
    load_chunk<B, FULL>(c.y, c.var, W.N, n, t0, len, v0, v1);
    load_chunk_noise<B, FULL>(ns, t0, len, p.q_s, qv);
    if constexpr (HAS_LAM) {
      student_load_weights<B, OBS, FULL>(c, W.N, n, t0, len, lv);
      reweight_chunk<B, FULL>(v1, lv, len);
    }
    filter_loaded_tv<B, UNIT, FULL>(v0, v1, qv, len, p, m, P);
  };
  if (len == B) forward(std::true_type{});
  else forward(std::false_type{});
  fuse_info(m, P, W.sEta[o], W.sJ[o]);
  smooth_rows_tv<B, UNIT>(v0, v1, qv, len, p, m, P, PointerStore<VS_ROW>{c.ms, c.Vs, W.N, n, n % M.D, t0});
  // a pass that never read the weights writes the ones it smoothed under.  kObsInPlace: every lane into its own
  // column; a group's weight has g lanes and no owner, so there the driver sets the plane before the launch.
  if constexpr (!HAS_LAM && OBS == kObsInPlace) {
#pragma unroll
    for (int i = 0; i < B; ++i)
      if (i < len) (c.lam + (size_t)(t0 + i) * (size_t)W.N)[(unsigned)n] = 1.0f;
  }
}

// T3, middle pass: the same forward pass and fuse, then ONE backward loop with no output code at all.  Per frame:
//   PROC         rts_step_jumps walks from frame t0 + i + 1 to t0 + i and returns delta_{t0+i+1,d}, stored under the
//                ownership rule; else rts_step;
//   !kObsFixed   from the belief just advanced to frame t0 + i, delta_obs = ((y - c m)^2 + c^2 P) / r, which
//                kObsInPlace turns into lam_new, stored in place, with the lane's largest |lam_new - lam_old| going
//                to change[keypoint] when the call asks for it (the last update only), and kObsGrouped stores.
// delta_obs needs y_t and r_t again after (v0, v1) have become (mf, Pf).  KEEP: they stay in registers (2 B more
// VGPRs); else they are loaded again in the backward pass, frame by frame (the rows were read by this lane moments
// ago) - eks_smooth_robust's A/B pair, DESIGN.md 9i.
template <int B, bool UNIT, bool HAS_LAM, ObsSide OBS, bool PROC, bool KEEP = true>
EKS_HD void student_replay_lane(const SampleWs& W, const DiagModel& M, const StudentCall& c, int n, int j) {
  // eks_smooth_heavy holds y, var, lam, w and the kept y0, r0 - six arrays a lane - and its replay sits at 244 / 250
  // VGPRs for two waves per SIMD: it has no seventh array qv, forms q_s w per frame in both loops and runs
  // filter_step in a loop of its own.  eks_smooth_jumps has the room: it builds qv and calls filter_loaded_tv.
  constexpr bool kQPerFrame = PROC && OBS != kObsFixed;
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const size_t o = (size_t)j * W.N + n;
  const NoiseScale ns = student_noise_scale<PROC>(c, M.D, n);
  float v0[B], v1[B], lv[B], wv[B], y0[B], r0[B], qv[B];
  float m = W.pm[o], P = W.pP[o];
  auto forward = [&](auto full) {
    constexpr bool FULL = decltype(full)::value;
    load_chunk<B, FULL>(c.y, c.var, W.N, n, t0, len, v0, v1);
    if constexpr (PROC) load_chunk_scale<B, FULL>(ns, t0, len, wv);
    else load_chunk_noise<B, FULL>(ns, t0, len, p.q_s, qv);   // w = 1 through the loads: eks_smooth_tv's bits (above)
    if constexpr (HAS_LAM) student_load_weights<B, OBS, FULL>(c, W.N, n, t0, len, lv);
    if constexpr (OBS != kObsFixed && KEEP) {
#pragma unroll
      for (int i = 0; i < B; ++i)
        if (FULL || i < len) { y0[i] = v0[i]; r0[i] = clip_var(v1[i]); }
    }
    if constexpr (HAS_LAM) reweight_chunk<B, FULL>(v1, lv, len);
    if constexpr (kQPerFrame) {
#pragma unroll
      for (int i = 0; i < B; ++i) {
        if (FULL || i < len) {
          const float r = clip_var(v1[i]);
          float mf, Pf;
          filter_step<float, UNIT>(m, P, v0[i], r, with_q(p, p.q_s * wv[i]), mf, Pf);
          v0[i] = mf;
          v1[i] = Pf;
        }
      }
    } else {
      if constexpr (PROC) {
#pragma unroll
        for (int i = 0; i < B; ++i)
          if (FULL || i < len) qv[i] = p.q_s * wv[i];
      }
      filter_loaded_tv<B, UNIT, FULL>(v0, v1, qv, len, p, m, P);
    }
  };
  if (len == B) forward(std::true_type{});
  else forward(std::false_type{});
  fuse_info(m, P, W.sEta[o], W.sJ[o]);
  const PointerRows rows{c.y, c.var, W.N, n, t0};
  float* out = c.contrib + (size_t)(PROC ? t0 + 1 : t0) * (size_t)W.N + (unsigned)n;
  const int left = c.T - (t0 + 1);
  float ch = 0.0f;
#pragma unroll
  for (int i = B - 1; i >= 0; --i) {
    if (i < len) {
      if constexpr (PROC) {
        const float dj = rts_step_jumps<float, UNIT>(m, P, v0[i], v1[i], with_q(p, p.q_s * wv[i]), wv[i]);
        if (i < left) out[(size_t)i * (size_t)W.N] = dj;
      } else {
        rts_step<float, UNIT>(m, P, v0[i], v1[i], with_q(p, qv[i]));
      }
      if constexpr (OBS != kObsFixed) {
        const float y = KEEP ? y0[i] : rows.load_y(i);
        const float r = KEEP ? r0[i] : clip_var(rows.load_var(i));
        const float d = UNIT ? (y - m) : (y - p.c * m);
        const float delta = (d * d + (UNIT ? P : p.c * p.c * P)) * rcp(r);
        if constexpr (OBS == kObsGrouped) {
          out[(size_t)i * (size_t)W.N] = r >= kVarCeil ? kGroupMissing : delta;
        } else {
          const float lam_new = robust_weight(c.nu, c.nu1, c.lam_max, delta);
          ch = fmaxf(ch, fabsf(lam_new - (HAS_LAM ? lv[i] : 1.0f)));
          (c.lam + (size_t)(t0 + i) * (size_t)W.N)[(unsigned)n] = lam_new;
        }
      }
    }
  }
  if constexpr (OBS == kObsInPlace) {
    if (c.change) robust_change_max(c.change + n / M.D, ch);
  }
}

}  // namespace eks
