// Lane-level bodies of eks_smooth_robust (eks_smooth_student.hip: scalar chains; eks_dense.hip: dense_smooth_robust),
// shared unchanged with tests/host_sim/robust_sim.cpp (plain loops).  No reference counterpart: the reference's
// observation noise is Gaussian with the ensemble variance (eks/core.py:182-186).
//
// The smoother under Student-t observation noise, one weight per scalar observation:
//     y_t | x_t, lam_t ~ N(c x_t, r_t / lam_t),   lam_t ~ Gamma(nu / 2, rate nu / 2),   r_t = clip_var(var_t),
// by the mean-field iteration of Agamennoni, Nieto and Nebot (2012).  One pass smooths under
// r_eff = clip_var(r_t / lam_t) - eks_smooth_tv's bodies at w = 1: elem_append, filter_step, rts_step - and, unless
// it is the call's last pass, replaces every weight by
//     lam_t = (nu + 1) / (nu + delta_t),   delta_t = ((y_t - c ms_t)^2 + c^2 Vs_t) / r_t       in (0, (nu + 1) / nu].
// lam: float [T][N] on scalar chains ([T][K][O] on general models), frame-major like var.  A lane reads its own B
// frames of lam before it writes them, and no other lane touches them in that launch: the update is in place.
//
// Accuracy limit: y - c ms cancels in float32, so delta carries an absolute error of about (2^-24 |y|)^2 / r:
// negligible for var >= 1e-2 at |y| <= 400 px, useless for var near the 1e-12 clip.  There the weights
// stay in range - lam is floored at kLamFloor, so that r / lam never divides by a rounded-to-zero weight - but carry
// no information.
#pragma once
#include "eks_smooth_tv_lane.hpp"

namespace eks {

constexpr float kLamFloor = 1e-30f;   // delta = inf (a missing frame's Vs over a clipped var) -> lam = 1e-30, not 0

// The variance a pass smooths frame t under, and the weight update.  Quotients are products with eks_math.hpp's rcp
// (v_rcp_f32 and one Newton step on the device, 1 / x on the host; rcp(1) = 1 exactly, so lam = 1 leaves r's bits):
// the IEEE division sequence is ten instructions deep and, three to a frame, took the replay to the 256-VGPR limit.
EKS_HD float robust_var(float var, float lam) { return clip_var(clip_var(var) * rcp(lam)); }

// (the ceiling: nu1 * rcp(nu) may round one ulp above (nu + 1) / nu; lam_max is that quotient rounded once from float64)
EKS_HD float robust_weight(float nu, float nu1, float lam_max, float delta) {
  return fminf(fmaxf(nu1 * rcp(nu + delta), kLamFloor), lam_max);
}

// max into change[k] on the bits of a non-negative float (they order like the values).  Most lanes find the maximum
// already above their own and issue no atomic.
EKS_HD void robust_change_max(float* dst, float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned bits = __float_as_uint(v);
  unsigned* p = reinterpret_cast<unsigned*>(dst);
  if (bits > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, bits);
#else
  if (v > *dst) *dst = v;
#endif
}

// the chunk's weights into registers (ordinary loads, B more in flight next to load_chunk's 2 B)
template <int B, bool FULL = false>
EKS_HD void load_chunk_weights(const float* __restrict__ lam, int N, int n, int t0, int len, float (&lv)[B]) {
#pragma unroll
  for (int i = 0; i < B; ++i)
    if (FULL || i < len) lv[i] = (lam + (size_t)(t0 + i) * (size_t)N)[(unsigned)n];
}

// var -> r_eff in place
template <int B, bool FULL = false>
EKS_HD void reweight_chunk(float (&rr)[B], const float (&lv)[B], int len) {
#pragma unroll
  for (int i = 0; i < B; ++i)
    if (FULL || i < len) rr[i] = robust_var(rr[i], lv[i]);
}

// ------------------------------------------------------------------------------------------------------------------
// General (D, O) models with diagonal R_t, float64 in the lane: the generic summarize / scan / replay with an
// observation visitor that divides r by lam[t][k][o], and an emit step that revisits the frame's rows:
//     delta_o = ((y_o - C_o m_s)^2 + C_o P_s C_o^T) / r_{t,o}      with the full P_s.
// ------------------------------------------------------------------------------------------------------------------
template <int D>
struct RobustObs {
  const float *y, *var;     // [T][K][O]
  const float* lam;         // [T][K][O], or null: every weight is 1
  int K, O;
  DenseModelPtrs M;
  template <typename Fn>
  EKS_HD void visit(int t, int k, const double* /*xl*/, Fn&& fn) const {
    const size_t row = ((size_t)t * K + k) * O;
    for (int o = 0; o < O; ++o) {
      const float v = var[row + o];
      const double r = (double)clip_var(v);   // float64 like the rest of this path; the weight itself is a float32
      fn(load_obs_row<double, D>(M, k, O, o), (double)y[row + o],
         lam ? fmin(fmax(r / (double)lam[row + o], (double)kVarFloor), (double)kVarCeil) : r);
    }
  }
};

template <int D>
EKS_HD RobustObs<D> make_robust_obs(const float* y, const float* var, const float* lam, int K, int O,
                                    const DenseModelPtrs& M) {
  return RobustObs<D>{y, var, lam, K, O, M};
}

// (m, P): the filtered belief of frame t0 - 1 (the prior itself when t0 == 0); (eta_s, J_s): what all later frames
// say about the state at the chunk's last frame; filt / fs: this lane's scratch records as in dense_replay_chunk_obs.
// last: ms / Vs out, weights untouched (ones written when obs.lam is null); else the weight update into lam_out and
// the lane's largest |lam_new - lam_old| returned.
template <int D>
EKS_HD double dense_robust_replay_chunk(const RobustObs<D>& obs, float* lam_out, double nu, bool last,
                                        int k, int t0, int len, const Mat<double, D>& F, const Mat<double, D>& sQ,
                                        bool f_identity, Vec<double, D> m, Mat<double, D> P,
                                        const Vec<double, D>& eta_s, const Mat<double, D>& J_s,
                                        double* __restrict__ filt, float* __restrict__ ms, float* __restrict__ Vs,
                                        bool vs_diag, size_t fs) {
  const int K = obs.K, O = obs.O;
  const Vec<double, D> m_in = m;
  const Mat<double, D> P_in = P;
  dense_forward_chunk<D, false>(obs, k, t0, len, F, sQ, f_identity, m, P, filt, fs);
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
      const double delta = (d * d + dot(h, mat_vec(Po, h))) / (double)clip_var(v);
      const float lam_new = fminf(fmaxf((float)((nu + 1.0) / (nu + delta)), kLamFloor), (float)((nu + 1.0) / nu));
      const float lam_old = obs.lam ? obs.lam[row + o] : 1.0f;
      ch = fmax(ch, (double)fabsf(lam_new - lam_old));
      lam_out[row + o] = lam_new;
    }
  };
  dense_backward_chunk<D>(
      t0, len, 0, F, sQ, f_identity, m_in, P_in, m, P, eta_s, J_s, filt, fs,
      [&](const Vec<double, D>& m_s, const Mat<double, D>& P_s) { emit(len - 1, m_s, P_s); },
      [&](int i, const DenseTransition<D>& tr) { emit(i, tr.m_s, tr.P_s); });
  return ch;
}

}  // namespace eks
