// Lane-level bodies of eks_smooth_heavy (eks_smooth_student.hip: scalar chains; eks_dense.hip: dense_smooth_heavy),
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
