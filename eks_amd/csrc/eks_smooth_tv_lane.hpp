// Lane-level bodies of eks_smooth_tv (eks_smooth_tv.hip: scalar chains; eks_dense.hip: dense_smooth_tv), shared
// unchanged with tests/host_sim/smooth_tv_sim.cpp (plain loops).  No reference counterpart: the reference's process
// noise is s Q at every step (eks/core.py:274-295).
//
// eks_smooth with one process-noise scale per frame:
//     x_0 ~ N(m0, S0),      x_t = A x_{t-1} + N(0, s w_t Q)      for t = 1 .. T-1,
// w = qscale [T] (shared) or [T][K] (per keypoint: every chain of keypoint k = n / D reads column k).  w_0 is never
// read, and a lane that predicts past frame T-1 uses 1 (no output depends on it).
//
// Scalar chains.  A frame is "update with y_t, then predict" (eks_math.hpp), so the noise added AFTER frame t's
// update is that of the step INTO t+1: frame t0 + i of a chunk uses w[t0 + i + 1], a chunk's last frame the first w
// of the next chunk, and the RTS gain of frame t the same w[t + 1].  The lane loads q_i = (s q) w[t0 + i + 1] for
// its B frames once and keeps them in registers for both passes; each frame then runs the constant-q bodies
// themselves - elem_append, filter_step, rts_gain / rts_advance - on a ChainParams whose q_s is q_i: the same
// expressions in the same order, and with w = 1 (q_s * 1.0f is exact) the same bits.
//
// General models predict INTO frame t and then observe it (eks_dense_lane.hpp), so frame t reads w[t], frame 0 has
// no predict, and the backward transition from frame t to t+1 reads w[t + 1].
#pragma once
#include "eks_increments_lane.hpp"

namespace eks {

// w of one chain: row t, column `col` of a [T][stride] plane (stride 1, col 0: the shared form)
struct NoiseScale {
  const float* w;
  int stride, col, T;
};

EKS_HD NoiseScale chain_noise_scale(const float* qscale, int per_keypoint, int K, int D, int n, int T) {
  return per_keypoint ? NoiseScale{qscale, K, n / D, T} : NoiseScale{qscale, 1, 0, T};
}

EKS_HD ChainParams<float> with_q(const ChainParams<float>& p, float q) {
  ChainParams<float> o = p;
  o.q_s = q;
  return o;
}

// q_i = (s q) w[t0 + i + 1] of the chunk's frames.  Ordinary per-lane loads: lanes of the same chunk (and, shared
// form, of the same keypoint) hit the same address; 32-bit offsets from the row of frame t0 + 1 (B * K < 2^31).
// FULL: len == B, so only the last frame's w can lie past T-1.
template <int B, bool FULL = false>
EKS_HD void load_chunk_noise(const NoiseScale& ns, int t0, int len, float q_s, float (&qv)[B]) {
  const float* row = ns.w + (size_t)(t0 + 1) * (size_t)ns.stride + (unsigned)ns.col;
  const int left = ns.T - (t0 + 1);
#pragma unroll
  for (int i = 0; i < B; ++i) {
    if (FULL && i < B - 1) qv[i] = q_s * row[(unsigned)i * (unsigned)ns.stride];
    else if (FULL || i < len) qv[i] = q_s * (i < left ? row[(unsigned)i * (unsigned)ns.stride] : 1.0f);
  }
}

// summarize_loaded with the frame's own q
template <int B, bool UNIT, bool FULL = false>
EKS_HD Elem<float> summarize_loaded_tv(const float (&yy)[B], const float (&rr)[B], const float (&qv)[B], int len,
                                       const ChainParams<float>& p) {
  Elem<float> e = elem_identity<float>();
#pragma unroll
  for (int i = 0; i < B; ++i) {
    if (FULL || i < len) {
      const float r = clip_var(rr[i]);
      elem_append<float, UNIT>(e, yy[i], r, with_q(p, qv[i]));
    }
  }
  return e;
}

// filter_loaded with the frame's own q
template <int B, bool UNIT, bool FULL = false>
EKS_HD void filter_loaded_tv(float (&v0)[B], float (&v1)[B], const float (&qv)[B], int len,
                             const ChainParams<float>& p, float& m, float& P) {
#pragma unroll
  for (int i = 0; i < B; ++i) {
    if (FULL || i < len) {
      const float r = clip_var(v1[i]);
      float mf, Pf;
      filter_step<float, UNIT>(m, P, v0[i], r, with_q(p, qv[i]), mf, Pf);
      v0[i] = mf;
      v1[i] = Pf;
    }
  }
}

// smooth_rows with the frame's own q (rts_advance, the deviation-form select included, is rts_step's)
template <int B, bool UNIT, bool FULL = false, typename ST>
EKS_HD void smooth_rows_tv(const float (&v0)[B], const float (&v1)[B], const float (&qv)[B], int len,
                           const ChainParams<float>& p, float m, float P, const ST& st) {
#pragma unroll
  for (int i = B - 1; i >= 0; --i) {
    if (FULL || i < len) {
      rts_step<float, UNIT>(m, P, v0[i], v1[i], with_q(p, qv[i]));
      st(i, m, P);
    }
  }
}

struct SmoothTvCall {
  const float *y, *var, *qscale;
  float *ms, *Vs;
  int T, K, per_keypoint;
};

// T1: element of chunk j of chain n
template <int B, bool UNIT>
EKS_HD void smooth_tv_summarize_lane(const SampleWs& W, const DiagModel& M, const SmoothTvCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const NoiseScale ns = chain_noise_scale(c.qscale, c.per_keypoint, c.K, M.D, n, c.T);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  float yy[B], rr[B], qv[B];
  Elem<float> e;
  if (len == B) {
    load_chunk<B, true>(c.y, c.var, W.N, n, t0, len, yy, rr);
    load_chunk_noise<B, true>(ns, t0, len, p.q_s, qv);
    e = summarize_loaded_tv<B, UNIT, true>(yy, rr, qv, len, p);
  } else {
    load_chunk<B>(c.y, c.var, W.N, n, t0, len, yy, rr);
    load_chunk_noise<B>(ns, t0, len, p.q_s, qv);
    e = summarize_loaded_tv<B, UNIT>(yy, rr, qv, len, p);
  }
  const size_t o = (size_t)j * W.N + n;
  W.eA[o] = e.A; W.eb[o] = e.b; W.eC[o] = e.C; W.eEta[o] = e.eta; W.eJ[o] = e.J;
}

// T3: replay of chunk j of chain n from the predicted belief that entered it (pm, pP) and the information after it
// (sEta, sJ): filter in registers, fuse, RTS backwards; ms / Vs rows follow PointerStore's contract.  Full chunks load
// and filter without per-frame predicates (with them each frame's loads sink in front of a wait of their
// own); the backward pass over registers has no loads and is the predicated one for both - a second unpredicated
// copy of it cost 40 - 70 VGPRs for nothing.
template <int B, bool UNIT, int VS_ROW>
EKS_HD void smooth_tv_replay_lane(const SampleWs& W, const DiagModel& M, const SmoothTvCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const NoiseScale ns = chain_noise_scale(c.qscale, c.per_keypoint, c.K, M.D, n, c.T);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const size_t o = (size_t)j * W.N + n;
  float v0[B], v1[B], qv[B];
  float m = W.pm[o], P = W.pP[o];
  const PointerStore<VS_ROW> st{c.ms, c.Vs, W.N, n, n % M.D, t0};
  if (len == B) {
    load_chunk<B, true>(c.y, c.var, W.N, n, t0, len, v0, v1);
    load_chunk_noise<B, true>(ns, t0, len, p.q_s, qv);
    filter_loaded_tv<B, UNIT, true>(v0, v1, qv, len, p, m, P);
  } else {
    load_chunk<B>(c.y, c.var, W.N, n, t0, len, v0, v1);
    load_chunk_noise<B>(ns, t0, len, p.q_s, qv);
    filter_loaded_tv<B, UNIT>(v0, v1, qv, len, p, m, P);
  }
  fuse_info(m, P, W.sEta[o], W.sJ[o]);
  smooth_rows_tv<B, UNIT>(v0, v1, qv, len, p, m, P, st);
}

// ------------------------------------------------------------------------------------------------------------------
// General (D, O) models, float64 in the lane: dense_smooth_element_obs, dense_forward_chunk and the shared backward
// walker with w_t (s Q) in place of s Q.  w = 0 and a singular Q are fine: only Pp is ever factored.
// ------------------------------------------------------------------------------------------------------------------
struct DenseNoiseScale {
  const float* w;
  int stride, col;     // [T][stride], column col (stride 1, col 0: shared)
  EKS_HD double at(int t) const { return (double)(w + (size_t)t * (size_t)stride)[(unsigned)col]; }
};

template <int D>
EKS_HD Mat<double, D> mat_scaled(const Mat<double, D>& Q, double w) {
  Mat<double, D> o;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) o.a[a][b] = w * Q.a[a][b];
  return o;
}

template <int D, typename Obs>
EKS_HD DElem<double, D> dense_tv_element(const Obs& obs, const DenseNoiseScale& ns, int k, int t0, int len,
                                         const Mat<double, D>& F, const Mat<double, D>& sQ, bool f_identity) {
  DElem<double, D> e = delem_identity<double, D>();
  for (int t = t0 > 0 ? t0 : 1; t < t0 + len; ++t) {
    delem_predict(e, F, mat_scaled<D>(sQ, ns.at(t)), f_identity);
    obs.visit(t, k, nullptr, [&](const Vec<double, D>& h, double yv, double r) { delem_observe(e, h, yv, r, false); });
  }
  return e;
}

// (m, P): the filtered belief of frame t0 - 1 (the prior itself when t0 == 0); (eta_s, J_s): what all later frames
// say about the state at the chunk's last frame; filt / fs: this lane's scratch records as in dense_replay_chunk_obs.
template <int D, typename Obs>
EKS_HD void dense_tv_replay_chunk(const Obs& obs, const DenseNoiseScale& ns, int K, int k, int t0, int len,
                                  const Mat<double, D>& F, const Mat<double, D>& sQ, bool f_identity,
                                  Vec<double, D> m, Mat<double, D> P, const Vec<double, D>& eta_s,
                                  const Mat<double, D>& J_s, double* __restrict__ filt, float* __restrict__ ms,
                                  float* __restrict__ Vs, bool vs_diag, size_t fs) {
  constexpr int REC = D + D * D;
  const Vec<double, D> m_in = m;
  const Mat<double, D> P_in = P;
  for (int i = 0; i < len; ++i) {
    const int t = t0 + i;
    if (t > 0) dense_predict(F, mat_scaled<D>(sQ, ns.at(t)), f_identity, m, P);
    belief_update_obs<D>(obs, k, t, nullptr, m, P);
    dense_store_rec<D>(filt + (size_t)i * REC * fs, fs, m, P);
  }
  auto emit = [&](int i, const Vec<double, D>& mo, const Mat<double, D>& Po) {
    const size_t ko = (size_t)(t0 + i) * K + k;
    dense_store_vec<D>(ms, ko, mo);
    dense_store_mat<D>(Vs, ko, Po, vs_diag);
  };
  dense_backward_walk<D>(
      t0, len, 0, F, [&](int i) { return mat_scaled<D>(sQ, ns.at(t0 + i + 1)); }, f_identity, m_in, P_in, m, P, eta_s,
      J_s, filt, fs, [&](const Vec<double, D>& m_s, const Mat<double, D>& P_s) { emit(len - 1, m_s, P_s); },
      [&](int i, const DenseTransition<D>& tr) { emit(i, tr.m_s, tr.P_s); });
}

}  // namespace eks
