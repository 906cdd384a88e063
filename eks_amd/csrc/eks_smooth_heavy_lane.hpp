// Lane-level bodies of eks_smooth_heavy (eks_smooth_heavy.hip: scalar chains; eks_dense.hip: dense_smooth_heavy),
// shared unchanged with tests/host_sim/heavy_sim.cpp (plain loops).  No reference counterpart.
//
// The smoother under Student-t noise on BOTH sides: eks_smooth_robust's weight per scalar observation and
// eks_smooth_jumps' scale per keypoint and frame,
//     y_t | x_t, lam_t ~ N(c x_t, r_t / lam_t),     lam_t ~ Gamma(nu_obs / 2, rate nu_obs / 2),    r_t = clip_var(var_t),
//     eps_t | u_t      ~ N(0, s Q / u_t),           u_t   ~ Gamma(nu_proc / 2, rate nu_proc / 2),  t = 1 .. T-1,
// by mean field over q(x) q(lam) q(u).  One pass smooths under r_eff = clip_var(r / lam) and w = 1 / u and, unless it
// is the call's last pass, sets BOTH updates from that one smoothed posterior:
//     lam = (nu_obs + 1) / (nu_obs + delta_obs)     (eks_smooth_robust_lane.hpp: robust_weight, its clamps),
//     w   = (nu_proc + delta_proc) / (nu_proc + D)  (eks_smooth_jumps_lane.hpp: rts_step_jumps, jumps_combine_lane).
// Given q(x) the two factors do not meet in the bound, so updating both after one pass is coordinate ascent.
//
// Who writes what in a middle replay: a lane stores lam_new into its own B frames of the weight plane (read before
// they are written, by no other lane of the launch) and delta_{t,d} into the contribution plane under
// eks_smooth_jumps' ownership rule (the step from frame t0 + i to t0 + i + 1 belongs to THIS chunk).  The scale plane
// is read only; the combine launch that follows is the one that changes it.
#pragma once
#include "eks_smooth_jumps_lane.hpp"

namespace eks {

struct HeavyCall {
  const float *y, *var;
  float* lam;            // [T][N]: the weights, read (HAS_LAM) and written in place
  const float* scales;   // [T][K]: w, read only
  float* contrib;        // [T][N]: delta_{t,d}, rows 1 .. T-1 written by a middle pass
  float* change;         // [K]: max |lam_new - lam_old| of this pass, or null
  float *ms, *Vs;        // written by the last pass only
  int T, K;
  float nu, nu1, lam_max;   // nu_obs, nu_obs + 1 and (nu_obs + 1) / nu_obs, each rounded once from float64
};

// T1: element of chunk j of chain n under r_eff and q_s w: robust_summarize_lane's body with the keypoint's column
// of the scale plane in the place of the vector of ones.
template <int B, bool UNIT, bool HAS_LAM>
EKS_HD void heavy_summarize_lane(const SampleWs& W, const DiagModel& M, const HeavyCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const NoiseScale ns{c.scales, c.K, n / M.D, c.T};
  float yy[B], rr[B], lv[B], qv[B];
  Elem<float> e;
  if (len == B) {
    load_chunk<B, true>(c.y, c.var, W.N, n, t0, len, yy, rr);
    load_chunk_noise<B, true>(ns, t0, len, p.q_s, qv);
    if constexpr (HAS_LAM) {
      load_chunk_weights<B, true>(c.lam, W.N, n, t0, len, lv);
      reweight_chunk<B, true>(rr, lv, len);
    }
    e = summarize_loaded_tv<B, UNIT, true>(yy, rr, qv, len, p);
  } else {
    load_chunk<B>(c.y, c.var, W.N, n, t0, len, yy, rr);
    load_chunk_noise<B>(ns, t0, len, p.q_s, qv);
    if constexpr (HAS_LAM) {
      load_chunk_weights<B>(c.lam, W.N, n, t0, len, lv);
      reweight_chunk<B>(rr, lv, len);
    }
    e = summarize_loaded_tv<B, UNIT>(yy, rr, qv, len, p);
  }
  const size_t o = (size_t)j * W.N + n;
  W.eA[o] = e.A; W.eb[o] = e.b; W.eC[o] = e.C; W.eEta[o] = e.eta; W.eJ[o] = e.J;
}

// T3, last pass: robust_replay_lane's LAST form under the scale plane: ms / Vs stream out through PointerStore, both
// planes stay (a pass that never read the weights writes the ones it smoothed under).
template <int B, bool UNIT, int VS_ROW, bool HAS_LAM>
EKS_HD void heavy_last_lane(const SampleWs& W, const DiagModel& M, const HeavyCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const size_t o = (size_t)j * W.N + n;
  const NoiseScale ns{c.scales, c.K, n / M.D, c.T};
  float v0[B], v1[B], lv[B], qv[B];
  float m = W.pm[o], P = W.pP[o];
  auto forward = [&](auto full) {
    constexpr bool FULL = decltype(full)::value;
    load_chunk<B, FULL>(c.y, c.var, W.N, n, t0, len, v0, v1);
    load_chunk_noise<B, FULL>(ns, t0, len, p.q_s, qv);
    if constexpr (HAS_LAM) {
      load_chunk_weights<B, FULL>(c.lam, W.N, n, t0, len, lv);
      reweight_chunk<B, FULL>(v1, lv, len);
    }
    filter_loaded_tv<B, UNIT, FULL>(v0, v1, qv, len, p, m, P);
  };
  if (len == B) forward(std::true_type{});
  else forward(std::false_type{});
  fuse_info(m, P, W.sEta[o], W.sJ[o]);
  smooth_rows_tv<B, UNIT>(v0, v1, qv, len, p, m, P, PointerStore<VS_ROW>{c.ms, c.Vs, W.N, n, n % M.D, t0});
  if constexpr (!HAS_LAM) {
#pragma unroll
    for (int i = 0; i < B; ++i)
      if (i < len) (c.lam + (size_t)(t0 + i) * (size_t)W.N)[(unsigned)n] = 1.0f;
  }
}

// T3, middle pass: no output code.  Forward under r_eff and q_s w (the product formed per frame, as
// jumps_replay_lane's backward loop does: y, var, lam, w and the kept y0, r0 are the six arrays a lane holds), fuse,
// then ONE backward loop: rts_step_jumps walks from frame t0 + i + 1 to t0 + i and returns delta_{t0+i+1,d}; from the
// belief it leaves on frame t0 + i the loop forms eks_smooth_robust's delta and stores lam_new in place.  y and
// clip_var(var) stay in registers for it (y0, r0: at 244 / 250 VGPRs the kernel keeps two waves per SIMD, so
// eks_smooth_robust's reload form was not needed).
template <int B, bool UNIT, bool HAS_LAM>
EKS_HD void heavy_replay_lane(const SampleWs& W, const DiagModel& M, const HeavyCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const size_t o = (size_t)j * W.N + n;
  const NoiseScale ns{c.scales, c.K, n / M.D, c.T};
  float v0[B], v1[B], lv[B], wv[B], y0[B], r0[B];
  float m = W.pm[o], P = W.pP[o];
  auto forward = [&](auto full) {
    constexpr bool FULL = decltype(full)::value;
    load_chunk<B, FULL>(c.y, c.var, W.N, n, t0, len, v0, v1);
    load_chunk_scale<B, FULL>(ns, t0, len, wv);
    if constexpr (HAS_LAM) load_chunk_weights<B, FULL>(c.lam, W.N, n, t0, len, lv);
#pragma unroll
    for (int i = 0; i < B; ++i)
      if (FULL || i < len) { y0[i] = v0[i]; r0[i] = clip_var(v1[i]); }
    if constexpr (HAS_LAM) reweight_chunk<B, FULL>(v1, lv, len);
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
  };
  if (len == B) forward(std::true_type{});
  else forward(std::false_type{});
  fuse_info(m, P, W.sEta[o], W.sJ[o]);
  float* out = c.contrib + (size_t)(t0 + 1) * (size_t)W.N + (unsigned)n;
  const int left = c.T - (t0 + 1);
  float ch = 0.0f;
#pragma unroll
  for (int i = B - 1; i >= 0; --i) {
    if (i < len) {
      const float dj = rts_step_jumps<float, UNIT>(m, P, v0[i], v1[i], with_q(p, p.q_s * wv[i]), wv[i]);
      if (i < left) out[(size_t)i * (size_t)W.N] = dj;
      const float d = UNIT ? (y0[i] - m) : (y0[i] - p.c * m);
      const float delta = (d * d + (UNIT ? P : p.c * p.c * P)) * rcp(r0[i]);
      const float lam_new = robust_weight(c.nu, c.nu1, c.lam_max, delta);
      ch = fmaxf(ch, fabsf(lam_new - (HAS_LAM ? lv[i] : 1.0f)));
      (c.lam + (size_t)(t0 + i) * (size_t)W.N)[(unsigned)n] = lam_new;
    }
  }
  if (c.change) robust_change_max(c.change + n / M.D, ch);
}

// ------------------------------------------------------------------------------------------------------------------
// General (D, O) models, float64 in the lane: the forward pass of dense_jumps_replay_chunk on RobustObs, then the
// shared backward walker - to i = -1 in a middle pass, where the transition callback forms delta_t of frame
// t0 + i + 1 (dense_jumps_replay_chunk's expression) and the emit step the weights of the chunk's own frames
// (dense_robust_replay_chunk's); to i = 0 in the last pass, which writes ms / Vs and no plane (ones into lam_out when
// obs.lam is null).  Returns the lane's largest |lam_new - lam_old|.
// ------------------------------------------------------------------------------------------------------------------
template <int D>
EKS_HD double dense_heavy_replay_chunk(const RobustObs<D>& obs, const DenseNoiseScale& ns, float* lam_out, double nu,
                                       bool last, int k, int t0, int len, const Mat<double, D>& F,
                                       const Mat<double, D>& sQ, bool f_identity, Vec<double, D> m, Mat<double, D> P,
                                       const Vec<double, D>& eta_s, const Mat<double, D>& J_s,
                                       double* __restrict__ filt, double* __restrict__ delta, float* __restrict__ ms,
                                       float* __restrict__ Vs, bool vs_diag, size_t fs) {
  constexpr int REC = D + D * D;
  const int K = obs.K, O = obs.O;
  const Vec<double, D> m_in = m;
  const Mat<double, D> P_in = P;
  for (int i = 0; i < len; ++i) {
    const int t = t0 + i;
    if (t > 0) dense_predict(F, mat_scaled<D>(sQ, ns.at(t)), f_identity, m, P);
    belief_update_obs<D>(obs, k, t, nullptr, m, P);
    dense_store_rec<D>(filt + (size_t)i * REC * fs, fs, m, P);
  }
  double ch = 0.0;
  auto emit = [&](int i, const Vec<double, D>& mo, const Mat<double, D>& Po) {
    const size_t ko = (size_t)(t0 + i) * K + k, row = ko * O;
    if (last) {
      dense_store_vec<D>(ms, ko, mo);
      dense_store_mat<D>(Vs, ko, Po, vs_diag);
      if (!obs.lam)
        for (int o = 0; o < O; ++o) lam_out[row + o] = 1.0f;
      return;
    }
    for (int o = 0; o < O; ++o) {
      const Vec<double, D> h = load_obs_row<double, D>(obs.M, k, O, o);
      const float v = obs.var[row + o];
      const double d = (double)obs.y[row + o] - dot(h, mo);
      const double dl = (d * d + dot(h, mat_vec(Po, h))) / (double)clip_var(v);
      const float lam_new = fminf(fmaxf((float)((nu + 1.0) / (nu + dl)), kLamFloor), (float)((nu + 1.0) / nu));
      const float lam_old = obs.lam ? obs.lam[row + o] : 1.0f;
      ch = fmax(ch, (double)fabsf(lam_new - lam_old));
      lam_out[row + o] = lam_new;
    }
  };
  dense_backward_walk<D>(
      t0, len, last ? 0 : -1, F, [&](int i) { return mat_scaled<D>(sQ, ns.at(t0 + i + 1)); }, f_identity, m_in, P_in, m,
      P, eta_s, J_s, filt, fs, [&](const Vec<double, D>& m_s, const Mat<double, D>& P_s) { emit(len - 1, m_s, P_s); },
      [&](int i, const DenseTransition<D>& tr) {
        if (!last) {
          const double w = ns.at(t0 + i + 1);
          const Mat<double, D> Ht = chol_solve_mat(tr.Lp, mat_scaled<D>(sQ, w));     // Pp^-1 (s w Q)
          Mat<double, D> S = tr.P_next;                                              // P' + dm dm'
#pragma unroll
          for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b < D; ++b) S.a[a][b] += tr.dm.a[a] * tr.dm.a[b];
          const Mat<double, D> X = chol_solve_mat(tr.Lp, S);                         // Pp^-1 (P' + dm dm')
          double acc = 0.0;
#pragma unroll
          for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b < D; ++b)
              acc += X.a[a][b] * Ht.a[b][a] + tr.Z.a[a][b] * (f_identity ? (a == b ? 1.0 : 0.0) : F.a[a][b]);
          delta[(size_t)(t0 + i + 1) * K + k] = w * acc;
        }
        if (i >= 0) emit(i, tr.m_s, tr.P_s);   // i = -1: frame t0 - 1 belongs to the chunk before
      });
  return ch;
}

}  // namespace eks
