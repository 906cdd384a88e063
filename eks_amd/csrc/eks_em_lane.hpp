// Lane-level bodies of eks_em_stats (eks_em.hip: scalar chains; eks_dense.hip: dense_em), shared unchanged with
// tests/host_sim/em_sim.cpp (plain loops).  No reference counterpart: the reference fits s to a constant-R filter
// likelihood (eks/core.py:640-652) and has no E-step.
//
// The E-step statistic of the model eks_smooth runs, per keypoint: the smoothed second moment of the process noise
//     Sw = sum_{t=0}^{T-2} E[ w_t w_t^T | y ],      w_t = x_{t+1} - A x_t,
// all from quantities the RTS step already holds.  Scalar chain, with (mf, Pf) the filtered belief of frame t,
// Pp = a^2 Pf + s q, h = s q / Pp (= 1 - a G) and (ms, Ps) the smoothed belief of frame t+1:
//     E[w_t | y]   = h (ms - a mf)
//     Var(w_t | y) = h^2 Ps + a^2 Pf h          (w_t = h (x_{t+1} - a mf) - a e, Var e = Pf h, e independent of x_{t+1})
//     Sw          += (E w_t)^2 + Var w_t
// a sum of non-negative products.  Vs[t+1] - 2 a lag1[t] + a^2 Vs[t] cancels three nearly equal numbers under heavy
// smoothing (as Vs[t] + Vs[t+1] - 2 lag1[t] does for dV) and is never formed.  The filter and the RTS step are
// float32 as in eks_smooth; each step's term is widened to float64 before it is added.
#pragma once
#include "eks_increments_lane.hpp"

namespace eks {

// rts_step (eks_math.hpp) that also returns the step's term of Sw: the same rts_gain and rts_advance, so the smoothed
// belief carried backwards is bit for bit the smoother's.  On entry (ms, Ps) is the smoothed belief on x_{t+1}, on
// exit on x_t.
template <typename R, bool UNIT>
EKS_HD R rts_step_em(R& ms, R& Ps, R mf, R Pf, const ChainParams<R>& p) {
  const RtsGain<R> k = rts_gain<R, UNIT>(mf, Pf, p);
  const R ew = k.h * (ms - k.amf);
  const R a2Pf = UNIT ? Pf : p.times_a2(Pf);
  const R term = ew * ew + (k.h * k.h * Ps + a2Pf * k.h);
  rts_advance(ms, Ps, mf, Pf, k);
  return term;
}

// RTS pass backwards over the filtered chunk (v0, v1) = (mf, Pf) from the smoothed belief (m, P) on the frame after
// it; returns the chunk's float64 sum of the steps' terms.  Step i is the transition from frame t0 + i to the next
// frame, so the transition into the following chunk belongs to THIS chunk; `last_chunk`: the chunk ends at frame T-1,
// whose "next frame" is the phantom predicted belief of frame T - that step adds nothing.
template <int B, bool UNIT>
EKS_HD double smooth_rows_em(const float (&v0)[B], const float (&v1)[B], int len, bool last_chunk,
                             const ChainParams<float>& p, float m, float P) {
  double acc = 0.0;
#pragma unroll
  for (int i = B - 1; i >= 0; --i) {
    if (i < len) {
      const float term = rts_step_em<float, UNIT>(m, P, v0[i], v1[i], p);
      const bool phantom = last_chunk && i == len - 1;
      acc += phantom ? 0.0 : (double)term;
    }
  }
  return acc;
}

struct EmCall {
  const float *y, *var;
  double* part;   // [nc][N]: one partial sum per (chunk, chain)
  int T;
};

// increments_replay_lane with the store functor replaced by a float64 accumulator: filter the loaded chunk in
// registers, fuse with the information after it, walk back.  Nothing of length T is written.
template <int B, bool UNIT>
EKS_HD void em_replay_lane(const SampleWs& W, const DiagModel& M, const EmCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const size_t o = (size_t)j * W.N + n;
  float v0[B], v1[B];
  load_chunk<B>(c.y, c.var, W.N, n, t0, len, v0, v1);
  float m = W.pm[o], P = W.pP[o];
  filter_loaded<B, UNIT>(v0, v1, len, p, m, P);
  fuse_info(m, P, W.sEta[o], W.sJ[o]);
  c.part[o] = smooth_rows_em<B, UNIT>(v0, v1, len, j == W.nc - 1, p, m, P);
}

// ------------------------------------------------------------------------------------------------------------------
// General (D, O) models, float64 throughout.  dense_increments_chunk's passes (eks_dense_lane.hpp: dense_forward_chunk,
// dense_backward_chunk) - the exact filter over the chunk into the lane's scratch records, then backwards to i = -1,
// so the transition between the chunk's first frame and the frame before it belongs to THIS chunk, from the belief
// that entered it.  With Z = Pp^-1 F Pf (G = Z^T),
// H = sQ Pp^-1 formed as H^T = Pp^-1 (sQ), and (m', P') the smoothed belief of frame t+1:
//     E[w_t | y]   = H (m' - F mf)
//     Cov(w_t | y) = H P' H^T + F (Pf - Z^T F Pf) F^T
//     Sw          += E w_t E w_t^T + Cov(w_t | y)
// Only Pp is factored, never Q: singular Q or S0 are fine while Pp is positive definite.
// part: this (keypoint, chunk)'s D x D partial (row-major), or its D diagonal entries with `diag`.
// ------------------------------------------------------------------------------------------------------------------
template <int D, typename Obs>
EKS_HD void dense_em_chunk(const Obs& obs, int k, int t0, int len, const Mat<double, D>& F, const Mat<double, D>& sQ,
                           bool f_identity, Vec<double, D> m, Mat<double, D> P, const Vec<double, D>& eta_s,
                           const Mat<double, D>& J_s, double* __restrict__ filt, size_t fs, double* __restrict__ part,
                           bool diag) {
  const Vec<double, D> m_in = m;
  const Mat<double, D> P_in = P;
  dense_forward_chunk<D, false>(obs, k, t0, len, F, sQ, f_identity, m, P, filt, fs);
  Mat<double, D> Sw = mat_zero<double, D>();
  dense_backward_chunk<D>(
      t0, len, -1, F, sQ, f_identity, m_in, P_in, m, P, eta_s, J_s, filt, fs,
      [](const Vec<double, D>&, const Mat<double, D>&) {},
      [&](int, const DenseTransition<D>& tr) {
        const Mat<double, D> Ht = chol_solve_mat(tr.Lp, sQ);                        // Pp^-1 sQ = H^T
        const Vec<double, D> ew = mat_t_vec(Ht, tr.dm);                             // H (m' - F mf)
        const Mat<double, D> Wm = mat_sub(tr.Pf, mat_mul_tn(tr.Z, tr.FP));          // Pf - G Pp G^T
        const Mat<double, D> FWF = f_identity ? Wm : mat_mul_nt(mat_mul(F, Wm), F);
        const Mat<double, D> cw = mat_sandwich_tn_plus(Ht, tr.P_next, FWF);         // H P' H^T + F W F^T
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
          for (int b = 0; b < D; ++b) Sw.a[a][b] += ew.a[a] * ew.a[b] + cw.a[a][b];
      });
  if (diag) {
#pragma unroll
    for (int a = 0; a < D; ++a) part[a] = Sw.a[a][a];
  } else {
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) part[a * D + b] = Sw.a[a][b];
  }
}

}  // namespace eks
