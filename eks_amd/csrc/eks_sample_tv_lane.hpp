// Lane-level bodies of eks_sample_tv on scalar chains (eks_sample_tv.hip), shared unchanged with
// tests/host_sim/sample_tv_sim.cpp (plain loops).  No reference counterpart.
//
// eks_sample (eks_sample_lane.hpp) under one process-noise scale per frame and one weight per observation:
//     x_t = a x_{t-1} + N(0, s w_t q),      y_t = c x_t + N(0, r_eff,t),      r_eff,t = robust_var(var_t, lam_t)
// - the Gaussian factor of the mean-field posteriors of eks_smooth_robust / _jumps / _heavy at their returned planes,
// and eks_smooth_tv's model at lam = 1.  Backward sampling as there, with the frame's own noise:
//     Pp_t = a^2 Pf_t + s q w_{t+1},   G_t = a Pf_t / Pp_t,   sd_t = sqrt(Pf_t s q w_{t+1} / Pp_t),
//     e_{T-1} = sqrt(Pf_{T-1}) z_{T-1},      e_t = G_t e_{t+1} + sd_t z_t.
// Index convention (eks_smooth_tv_lane.hpp): a frame is "update, then predict", so frame t0 + i of a chunk uses
// q_i = (s q) w[t0 + i + 1] in its filter step AND in its (G, sd); w[0] is never read and the session's last frame
// (G = 0, sd = sqrt(Pf)) reads none.  The lane loads q_i once (load_chunk_noise) and keeps it in registers across the
// filter and the backward pass; every frame runs the constant-q expressions of eks_sample_lane.hpp on
// with_q(p, q_i).  The variances are reweighted in registers (load_chunk_weights / reweight_chunk): no plane of r_eff
// exists anywhere.  chunk_beta, chunk_draw, the noise sources, the draw scans and the SampleWs planes are
// eks_sample's, unchanged.
#pragma once
#include "eks_smooth_robust_lane.hpp"

namespace eks {

struct SampleTvCall {
  const float *y, *var, *qscale, *weights, *noise;   // qscale null: every w is 1; weights read only where HAS_W
  float *ms, *draws;                                 // ms may be null
  int T, K, per_keypoint;
  uint32_t k0, k1, n_base, d_base;
};

// q_i of the chunk's frames; without a plane q_s * 1 = q_s
template <int B, bool FULL>
EKS_HD void sample_tv_chunk_noise(const SampleTvCall& c, int D, int n, int t0, int len, float q_s, float (&qv)[B]) {
  if (c.qscale) {
    load_chunk_noise<B, FULL>(chain_noise_scale(c.qscale, c.per_keypoint, c.K, D, n, c.T), t0, len, q_s, qv);
  } else {
#pragma unroll
    for (int i = 0; i < B; ++i) qv[i] = q_s;
  }
}

// (y, r_eff, q) of the chunk in registers
template <int B, bool FULL, bool HAS_W>
EKS_HD void sample_tv_load(const SampleTvCall& c, int N, int D, int n, int t0, int len, float q_s, float (&v0)[B],
                           float (&v1)[B], float (&qv)[B]) {
  load_chunk<B, FULL>(c.y, c.var, N, n, t0, len, v0, v1);
  if (HAS_W) {
    float lv[B];
    load_chunk_weights<B, FULL>(c.weights, N, n, t0, len, lv);
    reweight_chunk<B, FULL>(v1, lv, len);
  }
  sample_tv_chunk_noise<B, FULL>(c, D, n, t0, len, q_s, qv);
}

// filter_var_loaded with the frame's own q
template <int B, bool UNIT>
EKS_HD void filter_var_loaded_tv(float (&v1)[B], const float (&qv)[B], int len, const ChainParams<float>& p, float& P) {
#pragma unroll
  for (int i = 0; i < B; ++i) {
    if (i < len) {
      const float r = clip_var(v1[i]);
      const float Pc = UNIT ? P : P * p.c;
      const float g = rcp(UNIT ? (P + r) : (Pc * p.c + r));
      const float Pf = P * r * g;
      v1[i] = Pf;
      P = UNIT ? (Pf + qv[i]) : (p.times_a2(Pf) + qv[i]);
    }
  }
}

// chunk_gains with the frame's own q
template <int B, bool UNIT>
EKS_HD float chunk_gains_tv(float (&v1)[B], float (&v2)[B], const float (&qv)[B], int len, bool last_chunk,
                            const ChainParams<float>& p) {
  float gam = 1.0f;
#pragma unroll
  for (int i = 0; i < B; ++i) {
    if (i < len) {
      float G, sd;
      sample_coeffs<UNIT>(v1[i], with_q(p, qv[i]), last_chunk && i == len - 1, G, sd);
      v1[i] = G;
      v2[i] = sd;
      gam *= G;
    }
  }
  return gam;
}

// chunk_means_gains with the frame's own q; FULL: the filter runs without per-frame predicates
template <int B, bool UNIT, bool FULL>
EKS_HD void chunk_means_gains_tv(float (&v0)[B], float (&v1)[B], float (&v2)[B], const float (&qv)[B], int len,
                                 bool last_chunk, const ChainParams<float>& p, float m, float P, float etaS, float JS) {
  filter_loaded_tv<B, UNIT, FULL>(v0, v1, qv, len, p, m, P);
  fuse_info(m, P, etaS, JS);
#pragma unroll
  for (int i = B - 1; i >= 0; --i) {
    if (i < len) {
      const ChainParams<float> pi = with_q(p, qv[i]);
      float G, sd;
      sample_coeffs<UNIT>(v1[i], pi, last_chunk && i == len - 1, G, sd);
      rts_step<float, UNIT>(m, P, v0[i], v1[i], pi);
      v0[i] = m;
      v1[i] = G;
      v2[i] = sd;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The three passes over the frames, one lane = (chain n, chunk j), as in eks_sample_lane.hpp.
// ------------------------------------------------------------------------------------------------------------------
template <int B, bool UNIT, bool HAS_W>
EKS_HD void sample_tv_summarize_lane(const SampleWs& W, const DiagModel& M, const SampleTvCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  float yy[B], rr[B], qv[B];
  Elem<float> e;
  if (len == B) {
    sample_tv_load<B, true, HAS_W>(c, W.N, M.D, n, t0, len, p.q_s, yy, rr, qv);
    e = summarize_loaded_tv<B, UNIT, true>(yy, rr, qv, len, p);
  } else {
    sample_tv_load<B, false, HAS_W>(c, W.N, M.D, n, t0, len, p.q_s, yy, rr, qv);
    e = summarize_loaded_tv<B, UNIT>(yy, rr, qv, len, p);
  }
  const size_t o = (size_t)j * W.N + n;
  W.eA[o] = e.A; W.eb[o] = e.b; W.eC[o] = e.C; W.eEta[o] = e.eta; W.eJ[o] = e.J;
}

template <int B, bool UNIT, bool INJ, bool HAS_W>
EKS_HD void sample_beta_tv_lane(const SampleWs& W, const DiagModel& M, const SampleTvCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const size_t o = (size_t)j * W.N + n;
  float v1[B], v2[B], qv[B];
#pragma unroll
  for (int i = 0; i < B; ++i)
    if (i < len) v1[i] = (c.var + (size_t)(t0 + i) * (size_t)W.N)[(unsigned)n];
  if (HAS_W) {
    load_chunk_weights<B>(c.weights, W.N, n, t0, len, v2);
    reweight_chunk<B>(v1, v2, len);
  }
  if (len == B) sample_tv_chunk_noise<B, true>(c, M.D, n, t0, len, p.q_s, qv);
  else sample_tv_chunk_noise<B, false>(c, M.D, n, t0, len, p.q_s, qv);
  float P = W.pP[o];
  filter_var_loaded_tv<B, UNIT>(v1, qv, len, p, P);
  W.gam[o] = chunk_gains_tv<B, UNIT>(v1, v2, qv, len, j == W.nc - 1, p);
  auto draw_beta = [&](auto full) {
    for (int d = 0; d < W.n_draws; ++d) {
      float b;
      if (INJ)
        b = chunk_beta<B, full.value>(v1, v2, len, t0, NoiseRows{c.noise + (size_t)d * c.T * W.N, W.N, n});
      else
        b = chunk_beta<B, full.value>(v1, v2, len, t0,
                                      NoiseGen{c.k0, c.k1, c.n_base + (uint32_t)n, c.d_base + (uint32_t)d});
      W.beta[(size_t)d * W.nc * W.N + o] = b;
    }
  };
  if (len == B) draw_beta(std::true_type{});
  else draw_beta(std::false_type{});
}

template <int B, bool UNIT, bool INJ, bool HAS_W>
EKS_HD void sample_replay_tv_lane(const SampleWs& W, const DiagModel& M, const SampleTvCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const size_t o = (size_t)j * W.N + n;
  float v0[B], v1[B], v2[B];
  {
    float qv[B];
    if (len == B) {
      sample_tv_load<B, true, HAS_W>(c, W.N, M.D, n, t0, len, p.q_s, v0, v1, qv);
      chunk_means_gains_tv<B, UNIT, true>(v0, v1, v2, qv, len, j == W.nc - 1, p, W.pm[o], W.pP[o], W.sEta[o], W.sJ[o]);
    } else {
      sample_tv_load<B, false, HAS_W>(c, W.N, M.D, n, t0, len, p.q_s, v0, v1, qv);
      chunk_means_gains_tv<B, UNIT, false>(v0, v1, v2, qv, len, j == W.nc - 1, p, W.pm[o], W.pP[o], W.sEta[o], W.sJ[o]);
    }
  }
  if (c.ms) {
#pragma unroll
    for (int i = 0; i < B; ++i)
      if (i < len) EKS_STREAM_STORE(c.ms + (size_t)(t0 + i) * (size_t)W.N + (unsigned)n, v0[i]);
  }
  auto draw_all = [&](auto full) {
    for (int d = 0; d < W.n_draws; ++d) {
      const float e = W.beta[(size_t)d * W.nc * W.N + o];
      const DrawStore st{c.draws + ((size_t)d * c.T + t0) * (size_t)W.N, W.N, n};
      if (INJ)
        chunk_draw<B, full.value>(v0, v1, v2, len, t0, e, NoiseRows{c.noise + (size_t)d * c.T * W.N, W.N, n}, st);
      else
        chunk_draw<B, full.value>(v0, v1, v2, len, t0, e,
                                  NoiseGen{c.k0, c.k1, c.n_base + (uint32_t)n, c.d_base + (uint32_t)d}, st);
    }
  };
  if (len == B) draw_all(std::true_type{});
  else draw_all(std::false_type{});
}

}  // namespace eks
