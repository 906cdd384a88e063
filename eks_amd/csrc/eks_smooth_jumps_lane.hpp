// Lane-level bodies of eks_smooth_jumps (eks_smooth_student.hip: scalar chains and the combine kernel; eks_dense.hip:
// dense_smooth_jumps), shared unchanged with tests/host_sim/jumps_sim.cpp (plain loops).  No reference counterpart:
// the reference's process noise is Gaussian with one s per keypoint (eks/core.py:274-295).
//
// The smoother under Student-t process noise, one weight per keypoint and frame shared by its D state coordinates:
//     x_t = A x_{t-1} + eps_t,   eps_t | u_t ~ N(0, s Q / u_t),   u_t ~ Gamma(nu / 2, rate nu / 2),   t = 1 .. T-1,
// by the mean-field iteration: one pass smooths under the scales w_t = 1 / u_t - eks_smooth_tv with a per-keypoint
// qscale - and, unless it is the call's last pass, replaces every scale by
//     w_t = (nu + delta_t) / (nu + D),   delta_t = E[eps_t' (s Q)^-1 eps_t | y]   under the pass's own scales.
// delta_t comes from what the RTS step from frame t-1 to frame t already holds; Q is never inverted.  Scalar chain,
// with (mf, Pf) the filtered belief of frame t-1, Pp = a^2 Pf + s q w_t, h = s q w_t / Pp, (m', P') the smoothed
// belief of frame t and dm = m' - a mf:
//     delta_{t,d} = w_t ( h (dm^2 + P') + a^2 Pf ) / Pp,      delta_t = sum over the keypoint's D chains.
// With no data the term is w_t (w = 1 is the fixed point); a chain with s q = 0 contributes w_t, its prior value,
// whatever Pf is.  General models (Ht = Pp^-1 (s w_t Q), Z = Pp^-1 F Pf):
//     delta_t = w_t [ tr( Pp^-1 (P' + dm dm') Ht ) + tr( Z F' ) ].
//
// The D chains of a keypoint sit in different lanes, possibly in different blocks, and on general models the chunk
// after a boundary reads the scale the chunk before it would write: the replay stores contributions into a plane of
// their own ([T][N] float on scalar chains, [T][K] double on general models), and the scale plane changes only in the
// combine launch that follows it (jumps_combine_lane).  Row 0 of both planes is never read; w_0 is returned as 1.
//
// Accuracy limit: dm = m' - a mf cancels in float32 as y - c ms does for eks_smooth_robust's weights: delta carries an
// absolute error of about (2^-24 |m|)^2 / Pp.  u is floored at kLamFloor, so w stays finite.
#pragma once
#include "eks_smooth_robust_lane.hpp"

namespace eks {

// rts_step (eks_math.hpp) that also returns delta_{t+1,d} of the step it walks over: the same rts_gain and
// rts_advance, so the smoothed belief carried backwards is bit for bit the smoother's.  On entry (ms, Ps) is the
// smoothed belief on x_{t+1}, on exit on x_t; p.q_s is the step's own s q w, w its scale.
template <typename R, bool UNIT>
EKS_HD R rts_step_jumps(R& ms, R& Ps, R mf, R Pf, const ChainParams<R>& p, R w) {
  const RtsGain<R> k = rts_gain<R, UNIT>(mf, Pf, p);
  const R a2Pf = UNIT ? Pf : p.times_a2(Pf);
  const R ig = rcp(a2Pf + p.q_s);          // rts_gain's own 1 / Pp
  const R dm = ms - k.amf;
  const R term = (k.h * (dm * dm + Ps) + a2Pf) * ig;
  rts_advance(ms, Ps, mf, Pf, k);
  return p.q_s > R(0) ? w * term : w;      // s q w = 0: the prior value, never 0 / 0
}

// w[t0 + i + 1] of the chunk's frames (load_chunk_noise's addressing without the product with s q)
template <int B, bool FULL = false>
EKS_HD void load_chunk_scale(const NoiseScale& ns, int t0, int len, float (&wv)[B]) {
  const float* row = ns.w + (size_t)(t0 + 1) * (size_t)ns.stride + (unsigned)ns.col;
  const int left = ns.T - (t0 + 1);
#pragma unroll
  for (int i = 0; i < B; ++i) {
    if (FULL && i < B - 1) wv[i] = row[(unsigned)i * (unsigned)ns.stride];
    else if (FULL || i < len) wv[i] = i < left ? row[(unsigned)i * (unsigned)ns.stride] : 1.0f;
  }
}

// Combine, lane = (frame t >= 1, keypoint k): delta_t = the sum of the keypoint's nd contributions (D floats on
// scalar chains, one double on general models), u = (nu + D) / (nu + delta) kept in [kLamFloor, (nu + D) / nu],
// w = 1 / u rounded once to float32 into the scale plane; returns |u_new - u_old| for the caller's max into change[k].
// Float64 inside: the lanes are few and a float32 quotient would cost an ulp of u on top of the contribution's own
// error.
template <typename C>
EKS_HD float jumps_combine_lane(const C* __restrict__ contrib, int nd, float* scales, int K, int t, int k, double nu,
                                double nu_d) {
  const size_t o = (size_t)t * (size_t)K + (unsigned)k;
  double delta = 0.0;
  for (int d = 0; d < nd; ++d) delta += (double)contrib[o * (size_t)nd + d];
  const double u = fmin(fmax(nu_d / (nu + delta), (double)kLamFloor), nu_d / nu);
  const double u_old = 1.0 / (double)scales[o];
  scales[o] = (float)(1.0 / u);
  return (float)fabs(u - u_old);
}

// ------------------------------------------------------------------------------------------------------------------
// General (D, O) models, float64 in the lane: dense_tv_replay_chunk's forward pass, then the shared backward walker
// to i = -1 - the transition between the chunk's first frame and the frame before it belongs to THIS chunk, from
// the belief that entered it - with delta of frame t0 + i + 1 formed in the transition callback.  No ms / Vs.
// ------------------------------------------------------------------------------------------------------------------
template <int D, typename Obs>
EKS_HD void dense_jumps_replay_chunk(const Obs& obs, const DenseNoiseScale& ns, int K, int k, int t0, int len,
                                     const Mat<double, D>& F, const Mat<double, D>& sQ, bool f_identity,
                                     Vec<double, D> m, Mat<double, D> P, const Vec<double, D>& eta_s,
                                     const Mat<double, D>& J_s, double* __restrict__ filt, double* __restrict__ delta,
                                     size_t fs) {
  constexpr int REC = D + D * D;
  const Vec<double, D> m_in = m;
  const Mat<double, D> P_in = P;
  for (int i = 0; i < len; ++i) {
    const int t = t0 + i;
    if (t > 0) dense_predict(F, mat_scaled<D>(sQ, ns.at(t)), f_identity, m, P);
    belief_update_obs<D>(obs, k, t, nullptr, m, P);
    dense_store_rec<D>(filt + (size_t)i * REC * fs, fs, m, P);
  }
  dense_backward_walk<D>(
      t0, len, -1, F, [&](int i) { return mat_scaled<D>(sQ, ns.at(t0 + i + 1)); }, f_identity, m_in, P_in, m, P, eta_s,
      J_s, filt, fs, [](const Vec<double, D>&, const Mat<double, D>&) {},
      [&](int i, const DenseTransition<D>& tr) {
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
          for (int b = 0; b < D; ++b) acc += X.a[a][b] * Ht.a[b][a] + tr.Z.a[a][b] * (f_identity ? (a == b ? 1.0 : 0.0) : F.a[a][b]);
        delta[(size_t)(t0 + i + 1) * K + k] = w * acc;
      });
}

}  // namespace eks
