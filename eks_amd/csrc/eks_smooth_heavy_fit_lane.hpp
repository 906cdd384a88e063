// Lane-level bodies of eks_smooth_heavy_fit's M-step for the smoothing parameter (eks_smooth_heavy_fit.hip), shared
// unchanged with tests/host_sim/heavy_fit_sim.cpp (plain loops).  No reference counterpart.
//
// A middle pass of eks_smooth_heavy has smoothed under (lam, w = 1 / u, s), stored delta_{t,d} = E[eps' (s Q)^-1 eps]
// into the contribution plane and made its updates of lam and u.  With q(x) and the new q(u) held the bound is
// maximised over s by
//     S_k = sum_{t=1}^{T-1} u_new[t,k] delta[t,k],     s_new = s S_k / n,   n = D (T - 1),
// on log s clipped to [lo, hi].  delta_t is the float64 sum of the keypoint's nd contributions in jumps_combine_lane's
// order (nd = D floats on scalar chains, one double on general models), u = 1.0 / (double)scales[t][k] as the combine
// launch stored it for the next pass.  A side with nu = +inf is Gaussian: its combine launch is skipped, the plane
// stays at ones and S_k is the E-step statistic tr(Q^-1 Sw) / s of eks_em_stats.  A chain with s q = 0 keeps
// rts_step_jumps' convention - its contribution is w - so it counts u w = 1 per frame towards S_k.
//
// The order of the sum is fixed and depends on t alone, never on K, so two calls give the same bits and a call on a
// subset of the keypoints gives that subset's bits (eks_em_stats' contract):
//   sub-slab  kFitSub consecutive rows, added in order from 0.0                 (heavy_fit_sub_lane)
//   slab      kFitSubs consecutive sub-slabs = kFitSlab rows, added in order    (heavy_fit_slab_lane)
//   S_k       the slabs, added in order (heavy_fit_sum_lane); then the step     (heavy_fit_apply_lane)
// Rows count from t = 1: slab j holds rows 1 + j kFitSlab .. ; rows past T - 1 add nothing.  No floating-point atomics
// anywhere.
#pragma once
#include "eks_smooth_jumps_lane.hpp"

namespace eks {

constexpr int kFitSub = 16;                     // rows one lane adds in order
constexpr int kFitSubs = 64;                    // sub-slabs of a slab
constexpr int kFitSlab = kFitSub * kFitSubs;    // R: rows of a slab

inline int heavy_fit_slabs(int T) { return T < 2 ? 0 : (T - 1 + kFitSlab - 1) / kFitSlab; }

// rows t_first .. t_first + kFitSub - 1 (those below T) of keypoint k.  ND: nd at compile time (0: the run-time nd) -
// the same sums in the same order with the inner loop unrolled; a sub-slab that lies wholly below T runs unpredicated.
template <typename C, int ND = 0>
EKS_HD double heavy_fit_sub_lane(const C* __restrict__ contrib, int nd, const float* __restrict__ scales, int K, int T,
                                 int k, long t_first) {
  const int n = ND ? ND : nd;
  const auto term = [&](long t) {
    const size_t o = (size_t)t * (size_t)K + (unsigned)k;
    double delta = 0.0;
#pragma unroll
    for (int d = 0; d < n; ++d) delta += (double)contrib[o * (size_t)n + d];
    return (1.0 / (double)scales[o]) * delta;
  };
  double acc = 0.0;
  if (t_first + kFitSub <= (long)T) {
    double v[kFitSub];
#pragma unroll
    for (int i = 0; i < kFitSub; ++i) v[i] = term(t_first + i);
#pragma unroll
    for (int i = 0; i < kFitSub; ++i) acc += v[i];
  } else {
    for (int i = 0; i < kFitSub; ++i)
      if (t_first + i < (long)T) acc += term(t_first + i);
  }
  return acc;
}

// the kFitSubs sub-slab sums of one keypoint, `stride` doubles apart
EKS_HD double heavy_fit_slab_lane(const double* subs, int stride) {
  double v[kFitSubs], acc = 0.0;
#pragma unroll
  for (int i = 0; i < kFitSubs; ++i) v[i] = subs[(size_t)i * (size_t)stride];   // the loads in one round, then the adds
#pragma unroll
  for (int i = 0; i < kFitSubs; ++i) acc += v[i];
  return acc;
}

// The step on s[k] from S_k, and |delta log s| into dlog[k] (may be null).  S_k that is NaN, infinite or negative - a
// NaN-poisoned keypoint - and an s that is not finite and positive leave s[k] as it is, with 0 in dlog[k].  S_k = 0 is
// log s = -inf: clipped to lo.
EKS_HD void heavy_fit_apply_lane(double S, int k, double n, double lo, double hi, double* s, float* dlog) {
  const double s_old = s[k];
  double dl = 0.0;
  if (S >= 0.0 && S <= 1.7e308 && s_old > 0.0 && s_old <= 1.7e308) {
    const double ratio = S / n, l_old = log(s_old), l_new = l_old + log(ratio);
    double l_set = l_new, s_new = s_old * ratio;
    if (!(l_new >= lo)) { l_set = lo; s_new = exp(lo); }
    else if (l_new > hi) { l_set = hi; s_new = exp(hi); }
    s[k] = s_new;
    dl = fabs(l_set - l_old);
  }
  if (dlog) dlog[k] = (float)dl;
}

// m more slab sums of one keypoint, `stride` doubles apart, added in order onto S.  The kernel's last block calls it
// on the rounds of slab sums it has gathered in LDS, heavy_fit_step_lane on the partial sums themselves.
EKS_HD double heavy_fit_sum_lane(double S, const double* vals, int m, int stride) {
#pragma unroll 16
  for (int i = 0; i < m; ++i) S += vals[(size_t)i * (size_t)stride];
  return S;
}

// Keypoint k: S_k from the [n_slabs][K] partial sums, the slabs in order, then the step
EKS_HD void heavy_fit_step_lane(const double* part, int n_slabs, int K, int k, double n, double lo, double hi,
                                double* s, float* dlog) {
  heavy_fit_apply_lane(heavy_fit_sum_lane(0.0, part + k, n_slabs, K), k, n, lo, hi, s, dlog);
}

}  // namespace eks
