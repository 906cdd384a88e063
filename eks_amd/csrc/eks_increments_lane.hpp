// Lane-level bodies of eks_smooth_increments (eks_increments.hip, eks_dense.hip: dense_increments), shared unchanged
// with tests/host_sim/increments_sim.cpp (plain loops).  No reference counterpart: the reference returns per-frame
// marginals only (eks/core.py:296-297).
//
// eks_smooth plus the posterior of the frame-to-frame increment, for t = 0 .. T-2:
//     lag1[t]  = Cov(x_t, x_{t+1} | y)      dmean[t] = E[x_{t+1} - x_t | y]      dV[t] = Cov(x_{t+1} - x_t | y)
// all from quantities the RTS step already holds.  Scalar chain, with Pf, mf the filtered belief of frame t,
// Pp = a^2 Pf + s q, h = s q / Pp, G = a Pf / Pp, g = 1 - G = (h - (1 - a)) / a (rts_step's g) and (ms, Ps) the
// smoothed belief of frame t+1:
//     lag1  = G Ps
//     dmean = g (ms - a mf) - (1 - a) mf            (UNIT: h (ms - mf))
//     dV    = g^2 Ps + Pf h                         (x_t = mf + G (x_{t+1} - a mf) + e, Var e = Pf h, e independent)
// dV is a sum of non-negative products; Vs[t] + Vs[t+1] - 2 lag1[t] cancels three nearly equal numbers under heavy
// smoothing and is never formed.  Row T-1 of the three outputs is zero.
#pragma once
#include "eks_dense_lane.hpp"
#include "eks_sample_lane.hpp"

namespace eks {

// rts_step (eks_math.hpp) with the three increment outputs: the same rts_gain and rts_advance, so ms and Ps agree bit
// for bit with smooth_rows on the same inputs.  On entry (ms, Ps) is the smoothed belief on x_{t+1}, on exit on x_t.
template <typename R, bool UNIT>
EKS_HD void rts_step_increments(R& ms, R& Ps, R mf, R Pf, const ChainParams<R>& p, R& lag1, R& dmean, R& dV) {
  const RtsGain<R> k = rts_gain<R, UNIT>(mf, Pf, p);
  const R dev = ms - k.amf;
  lag1 = k.G * Ps;
  dmean = UNIT ? k.g * dev : k.g * dev - p.oma * mf;
  dV = k.g * k.g * Ps + Pf * k.h;
  rts_advance(ms, Ps, mf, Pf, k);
}

// RTS pass backwards over the filtered chunk (v0, v1) = (mf, Pf) from the smoothed belief (m, P) on the frame after it;
// every frame goes out through st(i, ms, Ps, lag1, dmean, dV).  `last_chunk`: the chunk ends at frame T-1, whose
// "next frame" is the phantom predicted belief of frame T - that step's G P must not be stored: zeros go out.
template <int B, bool UNIT, typename ST>
EKS_HD void smooth_rows_increments(const float (&v0)[B], const float (&v1)[B], int len, bool last_chunk,
                                   const ChainParams<float>& p, float m, float P, const ST& st) {
#pragma unroll
  for (int i = B - 1; i >= 0; --i) {
    if (i < len) {
      float lag1, dmean, dV;
      rts_step_increments<float, UNIT>(m, P, v0[i], v1[i], p, lag1, dmean, dV);
      const bool phantom = last_chunk && i == len - 1;
      st(i, m, P, phantom ? 0.0f : lag1, phantom ? 0.0f : dmean, phantom ? 0.0f : dV);
    }
  }
}

struct IncrementsCall {
  const float *y, *var;
  float *ms, *Vs, *lag1, *dmean, *dV;   // [T][N] each; any may be null
  int T;
};

// ALL: the caller knows that all five pointers are set (no per-output branch is compiled in); otherwise every store
// sits behind a wave-uniform test of its pointer.  A wave's 64 lanes are 64 consecutive chains of one frame (or
// 64 / NT chunks of NT chains): whole 256-byte rows, non-temporal.
template <bool ALL>
struct IncrementsStore {
  float *ms, *Vs, *lag1, *dmean, *dV;   // offset to the chunk's first frame
  int N, n;
  EKS_HD void operator()(int i, float m, float P, float l, float dm, float dv) const {
    const size_t o = (size_t)i * (size_t)N + (unsigned)n;
    if (ALL || ms) EKS_STREAM_STORE(ms + o, m);
    if (ALL || Vs) EKS_STREAM_STORE(Vs + o, P);
    if (ALL || lag1) EKS_STREAM_STORE(lag1 + o, l);
    if (ALL || dmean) EKS_STREAM_STORE(dmean + o, dm);
    if (ALL || dV) EKS_STREAM_STORE(dV + o, dv);
  }
};

// Replay of chunk j of chain n: filter the loaded chunk in registers, fuse with the information after it, walk back.
// (pm, pP): predicted belief entering the chunk; (sEta, sJ): information after it (SampleWs planes).
template <int B, bool UNIT, bool ALL>
EKS_HD void increments_replay_lane(const SampleWs& W, const DiagModel& M, const IncrementsCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const size_t o = (size_t)j * W.N + n;
  float v0[B], v1[B];
  load_chunk<B>(c.y, c.var, W.N, n, t0, len, v0, v1);
  float m = W.pm[o], P = W.pP[o];
  filter_loaded<B, UNIT>(v0, v1, len, p, m, P);
  fuse_info(m, P, W.sEta[o], W.sJ[o]);
  const size_t r0 = (size_t)t0 * (size_t)W.N;
  auto at = [&](float* q) { return q ? q + r0 : q; };
  smooth_rows_increments<B, UNIT>(v0, v1, len, j == W.nc - 1, p, m, P,
                                  IncrementsStore<ALL>{at(c.ms), at(c.Vs), at(c.lag1), at(c.dmean), at(c.dV), W.N, n});
}

// ------------------------------------------------------------------------------------------------------------------
// General (D, O) models, float64 in the lane, one rounding to float32 at the store.  The chunk's forward pass and
// backward walker (eks_dense_lane.hpp: dense_forward_chunk, dense_backward_chunk) with three more outputs per
// transition; the walk runs to i = -1 like the SCORE form, so the transition between the chunk's first frame and the
// frame before it is emitted by THIS chunk, from the belief that entered it.  With Z = Pp^-1 F Pf (G = Z^T), (m', P') the smoothed belief of frame t+1:
//     lag1  = G P'                   (row: coordinate of x_t, column: of x_{t+1})
//     dmean = m' - m_t
//     dV    = (I - G) P' (I - G)^T + (Pf - G Pp G^T),      G Pp G^T = Z^T (F Pf)
// Only Pp is factored, never Q: singular Q or S0 are fine while Pp is positive definite.
// ------------------------------------------------------------------------------------------------------------------
struct DenseIncrementsOut {
  float *ms, *Vs, *lag1, *dmean, *dV;   // any may be null
  bool vs_diag;
  int T;
};

// (m, P): the filtered belief of frame t0 - 1 (the prior itself when t0 == 0); (eta_s, J_s): what all later frames say
// about the state at the chunk's last frame; filt / fs: this lane's scratch records as in dense_replay_chunk_obs.
template <int D, typename Obs>
EKS_HD void dense_increments_chunk(const Obs& obs, int K, int k, int t0, int len, const Mat<double, D>& F,
                                   const Mat<double, D>& sQ, bool f_identity, Vec<double, D> m, Mat<double, D> P,
                                   const Vec<double, D>& eta_s, const Mat<double, D>& J_s, double* __restrict__ filt,
                                   const DenseIncrementsOut& out, size_t fs) {
  const Vec<double, D> m_in = m;
  const Mat<double, D> P_in = P;
  dense_forward_chunk<D, false>(obs, k, t0, len, F, sQ, f_identity, m, P, filt, fs);
  const Mat<double, D> eye = mat_eye<double, D>();
  dense_backward_chunk<D>(
      t0, len, -1, F, sQ, f_identity, m_in, P_in, m, P, eta_s, J_s, filt, fs,
      [&](const Vec<double, D>& m_s, const Mat<double, D>& P_s) {
        const size_t ko = (size_t)(t0 + len - 1) * K + k;
        dense_store_vec<D>(out.ms, ko, m_s);
        dense_store_mat<D>(out.Vs, ko, P_s, out.vs_diag);
        if (t0 + len == out.T) {                                  // row T-1 of the increment outputs: zeros
          dense_store_vec<D>(out.dmean, ko, vec_zero<double, D>());
          dense_store_mat<D>(out.lag1, ko, mat_zero<double, D>(), out.vs_diag);
          dense_store_mat<D>(out.dV, ko, mat_zero<double, D>(), out.vs_diag);
        }
      },
      [&](int i, const DenseTransition<D>& tr) {
        const size_t ko = (size_t)(t0 + i) * K + k;
        if (i >= 0) {
          dense_store_vec<D>(out.ms, ko, tr.m_s);
          dense_store_mat<D>(out.Vs, ko, tr.P_s, out.vs_diag);
        }
        if (out.dmean) {
          Vec<double, D> inc;
#pragma unroll
          for (int a = 0; a < D; ++a) inc.a[a] = tr.m_next.a[a] - tr.m_s.a[a];
          dense_store_vec<D>(out.dmean, ko, inc);
        }
        if (out.lag1) dense_store_mat<D>(out.lag1, ko, mat_mul_tn(tr.Z, tr.P_next), out.vs_diag);   // Cov(x_i, x_{i+1} | y)
        if (out.dV) {
          const Mat<double, D> W = mat_sub(tr.Pf, mat_mul_tn(tr.Z, tr.FP));     // Pf - G Pp G^T
          dense_store_mat<D>(out.dV, ko, mat_sandwich_tn_plus(mat_sub(eye, tr.Z), tr.P_next, W), out.vs_diag);
        }
      });
}

}  // namespace eks
