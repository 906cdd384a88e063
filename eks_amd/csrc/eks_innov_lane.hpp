// Lane-level bodies of eks_innovations (eks_innov.hip: scalar chains; eks_dense.hip: dense_innovations), shared
// unchanged with tests/host_sim/innov_sim.cpp (plain loops).  No reference counterpart: the reference's filter
// likelihood has a constant R (eks/core.py:640-652) and its innovations are never returned.
//
// The prediction-error decomposition of the model eks_smooth runs, per frame t, from the PREDICTED belief
// (m, P) = (m_{t|t-1}, P_{t|t-1}) - the prior (m0, S0) at t = 0 - before any update with frame t:
//     v_t = y_t - C m          S_t = C P C' + R_t          nis_t = v' S^-1 v
//     log p(y_t | y_{<t}) = -0.5 (O log 2 pi + log det S_t + nis_t),      loglik = sum_t
// Scalar chain: S = c^2 P + r and d = y - c m are the two quantities filter_step (eks_math.hpp) already forms; the
// chain's term is log 2 pi + log S + d^2 / S in float32, widened to float64 before it is added.  General models with
// diagonal R: the O scalar updates of belief_update_obs give sigma_o and d_o of observation o GIVEN observations
// 0 .. o-1 of the frame, and  log det S_t = sum_o log sigma_o,  nis_t = sum_o d_o^2 / sigma_o  exactly (the chain rule
// of the Gaussian density); innov and innov_var are the marginal ones, from the predicted belief, for every row.
#pragma once
#include "eks_increments_lane.hpp"

namespace eks {

constexpr float kLog2PiF = 1.8378770664093453f;

// filter_step (eks_math.hpp) that also returns the innovation d and its variance S: the expressions of the belief
// are filter_step's own, in its order, so the belief carried forward is bit for bit the smoother's.
template <typename R, bool UNIT>
EKS_HD void filter_step_innov(R& m, R& P, R y, R r, const ChainParams<R>& p, R& d, R& S, R& g) {
  const R c = UNIT ? R(1) : p.c;
  const R Pc = UNIT ? P : P * c;
  S = UNIT ? (P + r) : (Pc * c + r);
  g = rcp(S);
  d = UNIT ? (y - m) : (y - c * m);
  const R mf = m + Pc * g * d;
  const R Pf = P * r * g;
  m = UNIT ? mf : p.times_a(mf);
  P = UNIT ? (Pf + p.q_s) : (p.times_a2(Pf) + p.q_s);
}

// log 2 pi + log S + d^2 / S of one frame in float32; -0.5 x the float64 sum of these is the chain's log-likelihood
EKS_HD float innov_term(float d, float S, float g) { return kLog2PiF + std::log(S) + d * d * g; }

// Forward pass over the loaded chunk (v0, v1) = (y, var) from the predicted belief (m, P) on its first frame; every
// frame goes out through st(i, d, S); (m, P) leaves as the predicted belief on the frame after the chunk.  Returns
// the float64 sum of the frames' terms (0 without want_ll: no logarithm is evaluated).  FULL: the caller knows
// len == B (every chunk but a sequence's last): no per-frame predicate is compiled in, and the chunk's loads are not
// sunk one by one into the frames' predicated blocks, each in front of its own wait.
template <int B, bool UNIT, bool FULL = false, typename ST>
EKS_HD double innov_rows(const float (&v0)[B], const float (&v1)[B], int len, const ChainParams<float>& p, float& m,
                         float& P, bool want_ll, const ST& st) {
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < B; ++i) {
    if (FULL || i < len) {
      const float r = clip_var(v1[i]);
      float d, S, g;
      filter_step_innov<float, UNIT>(m, P, v0[i], r, p, d, S, g);
      st(i, d, S);
      if (want_ll) acc += (double)innov_term(d, S, g);
    }
  }
  return acc;
}

struct InnovCall {
  const float *y, *var;
  float *innov, *innov_var;   // [T][N] each; either may be null
  double* part;               // [nc][N]: one partial log-likelihood per (chunk, chain), or null
  int T;
};

// a wave's 64 lanes are 64 consecutive chains of one frame (or 64 / NT chunks of NT chains): whole 256-byte rows,
// non-temporal; every store sits behind a wave-uniform test of its pointer
struct InnovStore {
  float *innov, *innov_var;   // offset to the chunk's first frame
  int N, n;
  EKS_HD void operator()(int i, float d, float S) const {
    const size_t o = (size_t)i * (size_t)N + (unsigned)n;
    if (innov) EKS_STREAM_STORE(innov + o, d);
    if (innov_var) EKS_STREAM_STORE(innov_var + o, S);
  }
};

// Replay of chunk j of chain n, forward only: no fuse_info, no backward pass, no (mf, Pf) arrays.
// (pm, pP): predicted belief entering the chunk (SampleWs planes).
template <int B, bool UNIT>
EKS_HD void innov_replay_lane(const SampleWs& W, const DiagModel& M, const InnovCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const size_t o = (size_t)j * W.N + n;
  float v0[B], v1[B];
  float m = W.pm[o], P = W.pP[o];
  const size_t r0 = (size_t)t0 * (size_t)W.N;
  auto at = [&](float* q) { return q ? q + r0 : q; };
  const InnovStore st{at(c.innov), at(c.innov_var), W.N, n};
  double acc;
  if (len == B) {
    load_chunk<B, true>(c.y, c.var, W.N, n, t0, len, v0, v1);
    acc = innov_rows<B, UNIT, true>(v0, v1, len, p, m, P, c.part != nullptr, st);
  } else {
    load_chunk<B>(c.y, c.var, W.N, n, t0, len, v0, v1);
    acc = innov_rows<B, UNIT>(v0, v1, len, p, m, P, c.part != nullptr, st);
  }
  if (c.part) c.part[o] = -0.5 * acc;
}

// ------------------------------------------------------------------------------------------------------------------
// General (D, O) models, float64 in the lane, one rounding to float32 at the store.  (m, P) enters as the FILTERED
// belief of frame t0 - 1 (the prior itself when t0 == 0), as in dense_em_chunk; per frame: predict, the marginal
// innovations of all O rows from the predicted belief, then the update itself (belief_update_obs_acc) with the sums
// of log sigma and d^2 / sigma kept.  No scratch records and nothing is factored: a singular Q
// or S0 is fine while the innovation variances are positive.  Returns the chunk's log-likelihood.
// ------------------------------------------------------------------------------------------------------------------
struct DenseInnovOut {
  float *innov, *innov_var;   // [T][K][O], either may be null
  float *nis, *frame_ll;      // [T][K], either may be null
};

template <int D, typename Obs>
EKS_HD double dense_innov_chunk(const Obs& obs, int K, int O, int k, int t0, int len, const Mat<double, D>& F,
                                const Mat<double, D>& sQ, bool f_identity, Vec<double, D> m, Mat<double, D> P,
                                const DenseInnovOut& out) {
  double acc = 0.0;
  for (int i = 0; i < len; ++i) {
    const int t = t0 + i;
    if (t > 0) dense_predict(F, sQ, f_identity, m, P);
    const size_t fk = (size_t)t * K + k;
    if (out.innov || out.innov_var) {
      size_t at = fk * O;
      obs.visit(t, k, nullptr, [&](const Vec<double, D>& h, double yv, double r) {
        if (out.innov) EKS_STREAM_STORE(out.innov + at, (float)(yv - dot(h, m)));
        if (out.innov_var) EKS_STREAM_STORE(out.innov_var + at, (float)(r + dot(h, mat_vec(P, h))));
        ++at;
      });
    }
    double sum_log = 0.0, sum_sq = 0.0;
    belief_update_obs_acc<D>(obs, k, t, nullptr, m, P, [&](double sigma, double d, double gd) {
      sum_log += log(sigma);
      sum_sq += d * gd;
    });
    const double ll = -0.5 * ((double)O * kLog2Pi + sum_log + sum_sq);
    if (out.nis) EKS_STREAM_STORE(out.nis + fk, (float)sum_sq);
    if (out.frame_ll) EKS_STREAM_STORE(out.frame_ll + fk, (float)ll);
    acc += ll;
  }
  return acc;
}

}  // namespace eks
