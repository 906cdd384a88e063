// Lane-level bodies of eks_smooth_robust_group (eks_smooth_student.hip: scalar chains and the combine kernel;
// eks_dense.hip: dense_smooth_robust_group), shared unchanged with tests/host_sim/robust_group_sim.cpp (plain loops).
// No reference counterpart.
//
// eks_smooth_robust with ONE weight per group of g consecutive observed coordinates (a view of a multi-camera keypoint,
// the x and y of a single-camera one), the multivariate Student-t of Agamennoni, Nieto and Nebot (2012):
//     y_{t,G} | x_t, lam_{t,G} ~ N(C_G x_t, diag(r_{t,o}) / lam_{t,G}),   lam_{t,G} ~ Gamma(nu / 2, rate nu / 2).
// One pass smooths under r_eff = clip_var(r_{t,o} / lam_{t,G(o)}) - eks_smooth_robust's bodies - and, unless it is the
// call's last pass, replaces every weight by
//     lam_{t,G} = (nu + g_obs) / (nu + sum_{o in G, observed} delta_{t,o}),   delta as in eks_smooth_robust_lane.hpp,
// where a coordinate at the variance ceiling (kVarCeil: a missing observation) is not evidence and leaves the Gamma
// factor: g_obs = g wherever the group is observed, and a group with nothing observed keeps its prior mean, 1.
// lam: float [T][K][O / g], frame-major.  On scalar chains O = D and chain n reads column n / g of a [T][N / g] plane.
//
// The g chains of a group sit in different lanes, possibly in different blocks: the replay stores delta_{t,d} into a
// float [T][N] contribution plane (a missing coordinate stores kGroupMissing) and the weight plane changes only in the
// combine launch that follows it (eks_smooth_jumps_lane.hpp has the race argument).  Accuracy limit: that of
// eks_smooth_robust's delta.
#pragma once
#include "eks_smooth_robust_lane.hpp"

namespace eks {

constexpr float kGroupMissing = -1.0f;   // a contribution that is no evidence (delta itself is never negative)

// the weight from a group's sum (float64: the lanes are few, and the weight is rounded ONCE, into the plane)
EKS_HD float robust_group_weight(double nu, int g_obs, double sum) {
  if (g_obs == 0) return 1.0f;
  const double top = nu + (double)g_obs;
  return (float)fmin(fmax(top / (nu + sum), (double)kLamFloor), top / nu);
}

// Combine, lane = (frame t, column q of the weight plane = keypoint and group): the g contributions are adjacent in
// the contribution row; they are summed in float64 in index order.  Returns |lam_new - lam_old| for the caller's max
// into change[keypoint]; has_lam == 0: the pass smoothed under ones and the plane holds nothing yet.
EKS_HD float robust_group_combine_lane(const float* __restrict__ contrib, int g, float* lam, int NG, int t, int q,
                                       double nu, int has_lam) {
  const size_t o = (size_t)t * (size_t)NG + (unsigned)q;
  const float* cg = contrib + o * (size_t)g;
  double sum = 0.0;
  int g_obs = 0;
  for (int i = 0; i < g; ++i) {
    const float ci = cg[i];
    if (ci < 0.0f) continue;   // kGroupMissing
    sum += (double)ci;
    ++g_obs;
  }
  const float lam_new = robust_group_weight(nu, g_obs, sum);
  const float lam_old = has_lam ? lam[o] : 1.0f;
  lam[o] = lam_new;
  return fabsf(lam_new - lam_old);
}

// ------------------------------------------------------------------------------------------------------------------
// General (D, O) models with diagonal R_t, float64 in the lane: eks_smooth_robust's organisation with the weight of
// coordinate o read at lam[t][k][o / g], and an emit step that sums the frame's delta_o per group, in coordinate
// order, and writes lam[t][k][G].  A lane owns the weights of its own frames: in place, no combine launch.
// ------------------------------------------------------------------------------------------------------------------
template <int D>
struct RobustGroupObs {
  const float *y, *var;     // [T][K][O]
  const float* lam;         // [T][K][O / g], or null: every weight is 1
  int K, O, g;
  DenseModelPtrs M;
  template <typename Fn>
  EKS_HD void visit(int t, int k, const double* /*xl*/, Fn&& fn) const {
    const size_t tk = (size_t)t * K + k, row = tk * O, lrow = tk * (size_t)(O / g);
    for (int o = 0; o < O; ++o) {
      const double r = (double)clip_var(var[row + o]);
      fn(load_obs_row<double, D>(M, k, O, o), (double)y[row + o],
         lam ? fmin(fmax(r / (double)lam[lrow + o / g], (double)kVarFloor), (double)kVarCeil) : r);
    }
  }
};

template <int D>
EKS_HD RobustGroupObs<D> make_robust_group_obs(const float* y, const float* var, const float* lam, int K, int O, int g,
                                               const DenseModelPtrs& M) {
  return RobustGroupObs<D>{y, var, lam, K, O, g, M};
}

// Arguments as dense_robust_replay_chunk (eks_smooth_robust_lane.hpp).
template <int D>
EKS_HD double dense_robust_group_replay_chunk(const RobustGroupObs<D>& obs, float* lam_out, double nu, bool last,
                                              int k, int t0, int len, const Mat<double, D>& F,
                                              const Mat<double, D>& sQ, bool f_identity, Vec<double, D> m,
                                              Mat<double, D> P, const Vec<double, D>& eta_s,
                                              const Mat<double, D>& J_s, double* __restrict__ filt,
                                              float* __restrict__ ms, float* __restrict__ Vs, bool vs_diag, size_t fs) {
  const int K = obs.K, O = obs.O, g = obs.g, OG = O / g;
  const Vec<double, D> m_in = m;
  const Mat<double, D> P_in = P;
  dense_forward_chunk<D, false>(obs, k, t0, len, F, sQ, f_identity, m, P, filt, fs);
  double ch = 0.0;
  auto emit = [&](int i, const Vec<double, D>& mo, const Mat<double, D>& Po) {
    const size_t ko = (size_t)(t0 + i) * K + k, row = ko * O, lrow = ko * (size_t)OG;
    if (last) {
      dense_store_vec<D>(ms, ko, mo);
      dense_store_mat<D>(Vs, ko, Po, vs_diag);
      if (!obs.lam)
        for (int q = 0; q < OG; ++q) lam_out[lrow + q] = 1.0f;
      return;
    }
    for (int q = 0; q < OG; ++q) {
      double sum = 0.0;
      int g_obs = 0;
      for (int o = q * g; o < (q + 1) * g; ++o) {
        const float r = clip_var(obs.var[row + o]);
        if (r >= kVarCeil) continue;
        const Vec<double, D> h = load_obs_row<double, D>(obs.M, k, O, o);
        const double d = (double)obs.y[row + o] - dot(h, mo);
        sum += (d * d + dot(h, mat_vec(Po, h))) / (double)r;
        ++g_obs;
      }
      const float lam_new = robust_group_weight(nu, g_obs, sum);
      const float lam_old = obs.lam ? obs.lam[lrow + q] : 1.0f;
      ch = fmax(ch, (double)fabsf(lam_new - lam_old));
      lam_out[lrow + q] = lam_new;
    }
  };
  dense_backward_chunk<D>(
      t0, len, 0, F, sQ, f_identity, m_in, P_in, m, P, eta_s, J_s, filt, fs,
      [&](const Vec<double, D>& m_s, const Mat<double, D>& P_s) { emit(len - 1, m_s, P_s); },
      [&](int i, const DenseTransition<D>& tr) { emit(i, tr.m_s, tr.P_s); });
  return ch;
}

}  // namespace eks
