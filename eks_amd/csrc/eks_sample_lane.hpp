// Lane-level bodies of the joint posterior sampler on scalar chains (eks_sample.hip), shared unchanged with
// tests/host_sim/sample_sim.cpp (plain loops) like eks_diag_lane.hpp.  No reference counterpart: the reference
// returns per-frame marginals only (eks/core.py:296-297).
//
// For a linear Gaussian model the posterior covariance does not depend on y, so a draw is x = ms + e with e a
// zero-mean draw of the joint posterior covariance.  Backward sampling on one chain, with the filtered variance
// Pf_t, Pp = a^2 Pf_t + s q and the RTS gain G_t = a Pf_t / Pp:
//     e_{T-1} = sqrt(Pf_{T-1}) z_{T-1},      e_t = G_t e_{t+1} + sqrt(Pf_t s q / Pp) z_t
// (the innovation variance Pf - G^2 Pp in its cancellation-free product form).  The recurrence is affine in e_{t+1},
// so a chunk of frames is summarised as e_first = Gamma e_next + beta (Gamma = prod G_t shared by all draws, beta per
// draw), the chunks are scanned backwards per (chain, draw), and the replay walks every chunk again from its e_next
// with the SAME normals: they come from a counter-based generator and are regenerated, never stored.
//
// Normals: Philox4x32-10 (Salmon et al. 2011), key = the 64-bit seed, counter = (frame / 4, global chain index,
// global draw index, 0); the block's four words give the normals of the four frames 4 (frame / 4) + {0, 1, 2, 3} by
// two Box-Muller transforms (words 0, 1 -> frames +0, +1; words 2, 3 -> frames +2, +3).  A normal is a function of
// (seed, frame, chain, draw) alone: no launch geometry, chunk length or tiling enters.
#pragma once
#include <type_traits>

#include "eks_diag_lane.hpp"

namespace eks {

struct Philox4 {
  uint32_t x[4];
};

EKS_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // (one 32 x 32 -> 64 multiply per half: v_mad_u64_u32 gives both words)
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// Box-Muller on two 32-bit words: u = (top 24 bits + 1/2) 2^-24 in (0, 1) and the angle v = top 24 bits 2^-24 of a
// revolution, both exact in float32; z0 = sqrt(-2 ln u) cos(2 pi v), z1 = ... sin(2 pi v).  |z| <= 5.9.  On the
// device the logarithm and the sine / cosine are the hardware's (v_log_f32, v_sin_f32 / v_cos_f32 take revolutions).
EKS_HD void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  const float u = ((float)(a >> 8) + 0.5f) * 5.9604644775390625e-08f;
  const float v = (float)(b >> 8) * 5.9604644775390625e-08f;
#if defined(__HIP_DEVICE_COMPILE__)
  // (-2 ln 2 log2 u lies in [1.2e-7, 35]: the raw v_sqrt_f32, 1 ulp, needs none of sqrtf's range fix-ups)
  const float r = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u));
  z0 = r * __builtin_amdgcn_cosf(v);
  z1 = r * __builtin_amdgcn_sinf(v);
#else
  const float r = std::sqrt(-2.0f * std::log(u));
  z0 = r * (float)std::cos(6.283185307179586 * (double)v);
  z1 = r * (float)std::sin(6.283185307179586 * (double)v);
#endif
}

// The normals of frames 4 tq .. 4 tq + 3 of (chain, draw), both GLOBAL indices.
struct NoiseGen {
  uint32_t k0, k1, chain, draw;
  EKS_HD void get4(int tq, int /*nvalid*/, float (&z)[4]) const {
    const Philox4 w = philox4x32_10((uint32_t)tq, chain, draw, 0u, k0, k1);
    box_muller(w.x[0], w.x[1], z[0], z[1]);
    box_muller(w.x[2], w.x[3], z[2], z[3]);
  }
};

// Injected normals: rows[t][n] of one draw's [T][N] plane; only the nvalid frames that exist are read.
struct NoiseRows {
  const float* z;   // the draw's plane
  int N, n;
  EKS_HD void get4(int tq, int nvalid, float (&out)[4]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = i < nvalid ? (z + (size_t)(4 * tq + i) * (size_t)N)[(unsigned)n] : 0.0f;
  }
};

// Variance half of filter_step (the same expressions): the filtered variances do not depend on y.
template <int B, bool UNIT>
EKS_HD void filter_var_loaded(float (&v1)[B], int len, const ChainParams<float>& p, float& P) {
#pragma unroll
  for (int i = 0; i < B; ++i) {
    if (i < len) {
      const float r = clip_var(v1[i]);
      const float Pc = UNIT ? P : P * p.c;
      const float g = rcp(UNIT ? (P + r) : (Pc * p.c + r));
      const float Pf = P * r * g;
      v1[i] = Pf;
      P = UNIT ? (Pf + p.q_s) : (p.times_a2(Pf) + p.q_s);
    }
  }
}

// (G_t, sd_t) of one frame from its filtered variance; `last`: t == T - 1 (nothing to condition on).
// (Pp, h, G as in rts_gain, eks_math.hpp; kept apart from it: taken from rts_gain the sampler's kernels come out of
// the compiler as different code.)
template <bool UNIT>
EKS_HD void sample_coeffs(float Pf, const ChainParams<float>& p, bool last, float& G, float& sd) {
  const float Pp = UNIT ? (Pf + p.q_s) : (p.times_a2(Pf) + p.q_s);
  const float ig = rcp(Pp);
  const float h = p.q_s * ig;
  G = last ? 0.0f : (UNIT ? Pf * ig : p.a * Pf * ig);
  sd = std::sqrt(last ? Pf : Pf * h);
}

// Filtered variances of a chunk (in v1) -> (G, sd) per frame (v1, v2); returns Gamma = prod G.
template <int B, bool UNIT>
EKS_HD float chunk_gains(float (&v1)[B], float (&v2)[B], int len, bool last_chunk, const ChainParams<float>& p) {
  float gam = 1.0f;
#pragma unroll
  for (int i = 0; i < B; ++i) {
    if (i < len) {
      float G, sd;
      sample_coeffs<UNIT>(v1[i], p, last_chunk && i == len - 1, G, sd);
      v1[i] = G;
      v2[i] = sd;
      gam *= G;
    }
  }
  return gam;
}

// beta of one (chunk, draw): the chunk's recurrence from e_next = 0.  t0 is a multiple of 4 (B is).  FULL: the
// caller knows len == B (every chunk but a session's last): no per-frame predicate is compiled in.
template <int B, bool FULL, typename NOISE>
EKS_HD float chunk_beta(const float (&G)[B], const float (&sd)[B], int len, int t0, const NOISE& noise) {
  static_assert(B % 4 == 0, "a Philox block serves four consecutive frames");
  float e = 0.0f;
#pragma unroll
  for (int q = B / 4 - 1; q >= 0; --q) {
    if (FULL || 4 * q < len) {
      float z[4];
      noise.get4((t0 >> 2) + q, FULL ? 4 : len - 4 * q, z);
#pragma unroll
      for (int ii = 3; ii >= 0; --ii) {
        const int i = 4 * q + ii;
        if (FULL || i < len) e = fmaf(G[i], e, sd[i] * z[ii]);
      }
    }
  }
  return e;
}

// One draw of a chunk: walks backwards from e (the deviation on the frame after the chunk) and hands
// st(i, ms_i + e_i) every frame.
template <int B, bool FULL, typename NOISE, typename ST>
EKS_HD void chunk_draw(const float (&msv)[B], const float (&G)[B], const float (&sd)[B], int len, int t0, float e,
                       const NOISE& noise, const ST& st) {
#pragma unroll
  for (int q = B / 4 - 1; q >= 0; --q) {
    if (FULL || 4 * q < len) {
      float z[4];
      noise.get4((t0 >> 2) + q, FULL ? 4 : len - 4 * q, z);
#pragma unroll
      for (int ii = 3; ii >= 0; --ii) {
        const int i = 4 * q + ii;
        if (FULL || i < len) {
          e = fmaf(G[i], e, sd[i] * z[ii]);
          st(i, msv[i] + e);
        }
      }
    }
  }
}

// Filter the loaded chunk, fuse with the future's information and run RTS backwards: v0 <- smoothed means,
// (v1, v2) <- (G, sd).  (m, P): predicted belief entering the chunk; (etaS, JS): information after it.
template <int B, bool UNIT>
EKS_HD void chunk_means_gains(float (&v0)[B], float (&v1)[B], float (&v2)[B], int len, bool last_chunk,
                              const ChainParams<float>& p, float m, float P, float etaS, float JS) {
  filter_loaded<B, UNIT>(v0, v1, len, p, m, P);
  fuse_info(m, P, etaS, JS);
#pragma unroll
  for (int i = B - 1; i >= 0; --i) {
    if (i < len) {
      float G, sd;
      sample_coeffs<UNIT>(v1[i], p, last_chunk && i == len - 1, G, sd);
      rts_step<float, UNIT>(m, P, v0[i], v1[i], p);
      v0[i] = m;
      v1[i] = G;
      v2[i] = sd;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The two scans over chunks, each in three steps with lanes along chains: the nc chunks of a chain are cut into ng
// groups of gs; (1) a lane reduces one group, (2) a lane walks the ng aggregates of a chain, (3) a lane walks its
// group again from the group's boundary values.  All planes are [chunk or group][N].
// ------------------------------------------------------------------------------------------------------------------
struct SampleWs {
  float *eA, *eb, *eC, *eEta, *eJ;   // chunk elements [nc][N]
  float *pm, *pP, *sEta, *sJ;        // predicted belief entering chunk j, information after it [nc][N]
  float* gam;                        // Gamma [nc][N]
  float* beta;                       // [n_draws][nc][N]: beta, then (in place) e_next of every chunk
  float *gA, *gb, *gC, *gEta, *gJ;   // group aggregates [ng][N]
  float *gm, *gP, *gsEta, *gsJ;      // belief entering / information after every group [ng][N]
  float* hG;                         // group Gamma [ng][N]
  float* hB;                         // [n_draws][ng][N]: group beta, then e_next of every group
  int N, nc, ng, gs, n_draws;
};

EKS_HD Elem<float> ws_elem(const SampleWs& W, size_t o) { return Elem<float>{W.eA[o], W.eb[o], W.eC[o], W.eEta[o], W.eJ[o]}; }

EKS_HD void kalman_group_reduce(const SampleWs& W, int n, int g) {
  const int j1 = (g + 1) * W.gs < W.nc ? (g + 1) * W.gs : W.nc;
  Elem<float> e = elem_identity<float>();
  for (int j = g * W.gs; j < j1; ++j) e = elem_combine(e, ws_elem(W, (size_t)j * W.N + n));
  const size_t o = (size_t)g * W.N + n;
  W.gA[o] = e.A; W.gb[o] = e.b; W.gC[o] = e.C; W.gEta[o] = e.eta; W.gJ[o] = e.J;
}

EKS_HD void kalman_group_scan(const SampleWs& W, int n, float m, float P) {
  for (int g = 0; g < W.ng; ++g) {
    const size_t o = (size_t)g * W.N + n;
    W.gm[o] = m;
    W.gP[o] = P;
    elem_apply(Elem<float>{W.gA[o], W.gb[o], W.gC[o], W.gEta[o], W.gJ[o]}, m, P);
  }
  float eta = 0.f, J = 0.f;
  for (int g = W.ng - 1; g >= 0; --g) {
    const size_t o = (size_t)g * W.N + n;
    W.gsEta[o] = eta;
    W.gsJ[o] = J;
    elem_back(Elem<float>{W.gA[o], W.gb[o], W.gC[o], W.gEta[o], W.gJ[o]}, eta, J);
  }
}

EKS_HD void kalman_group_apply(const SampleWs& W, int n, int g) {
  const int j0 = g * W.gs, j1 = (g + 1) * W.gs < W.nc ? (g + 1) * W.gs : W.nc;
  const size_t og = (size_t)g * W.N + n;
  float m = W.gm[og], P = W.gP[og];
  for (int j = j0; j < j1; ++j) {
    const size_t o = (size_t)j * W.N + n;
    W.pm[o] = m;
    W.pP[o] = P;
    elem_apply(ws_elem(W, o), m, P);
  }
  float eta = W.gsEta[og], J = W.gsJ[og];
  for (int j = j1 - 1; j >= j0; --j) {
    const size_t o = (size_t)j * W.N + n;
    W.sEta[o] = eta;
    W.sJ[o] = J;
    elem_back(ws_elem(W, o), eta, J);
  }
}

EKS_HD void draw_group_reduce(const SampleWs& W, int n, int g, int d) {
  const int j0 = g * W.gs, j1 = (g + 1) * W.gs < W.nc ? (g + 1) * W.gs : W.nc;
  const float* beta = W.beta + (size_t)d * W.nc * W.N;
  float GG = 1.0f, bb = 0.0f;
  for (int j = j1 - 1; j >= j0; --j) {
    const size_t o = (size_t)j * W.N + n;
    const float gm = W.gam[o];
    bb = fmaf(gm, bb, beta[o]);
    GG *= gm;
  }
  const size_t og = (size_t)g * W.N + n;
  W.hB[(size_t)d * W.ng * W.N + og] = bb;
  if (d == 0) W.hG[og] = GG;
}

EKS_HD void draw_group_scan(const SampleWs& W, int n, int d) {
  float* hB = W.hB + (size_t)d * W.ng * W.N;
  float e = 0.0f;
  for (int g = W.ng - 1; g >= 0; --g) {
    const size_t og = (size_t)g * W.N + n;
    const float bb = hB[og];
    hB[og] = e;
    e = fmaf(W.hG[og], e, bb);
  }
}

EKS_HD void draw_group_apply(const SampleWs& W, int n, int g, int d) {
  const int j0 = g * W.gs, j1 = (g + 1) * W.gs < W.nc ? (g + 1) * W.gs : W.nc;
  float* beta = W.beta + (size_t)d * W.nc * W.N;
  float e = W.hB[(size_t)d * W.ng * W.N + (size_t)g * W.N + n];
  for (int j = j1 - 1; j >= j0; --j) {
    const size_t o = (size_t)j * W.N + n;
    const float b = beta[o];
    beta[o] = e;
    e = fmaf(W.gam[o], e, b);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The three passes over the frames, one lane = (chain n, chunk j).  n_base / d_base: GLOBAL indices of chain 0 and
// draw 0 of this call (first_keypoint * D, first_draw); noise != nullptr: injected normals [n_draws][T][N].
// ------------------------------------------------------------------------------------------------------------------
struct SampleCall {
  const float *y, *var, *noise;
  float *ms, *draws;   // ms may be null
  int T;
  uint32_t k0, k1, n_base, d_base;
};

template <int B, bool UNIT>
EKS_HD void sample_summarize_lane(const SampleWs& W, const DiagModel& M, const SampleCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const Elem<float> e = summarize_chunk<B, UNIT>(c.y, c.var, W.N, n, t0, len, p);
  const size_t o = (size_t)j * W.N + n;
  W.eA[o] = e.A; W.eb[o] = e.b; W.eC[o] = e.C; W.eEta[o] = e.eta; W.eJ[o] = e.J;
}

template <int B, bool UNIT, bool INJ>
EKS_HD void sample_beta_lane(const SampleWs& W, const DiagModel& M, const SampleCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const size_t o = (size_t)j * W.N + n;
  float v1[B], v2[B];
#pragma unroll
  for (int i = 0; i < B; ++i)
    if (i < len) v1[i] = (c.var + (size_t)(t0 + i) * (size_t)W.N)[(unsigned)n];
  float P = W.pP[o];
  filter_var_loaded<B, UNIT>(v1, len, p, P);
  W.gam[o] = chunk_gains<B, UNIT>(v1, v2, len, j == W.nc - 1, p);
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

struct DrawStore {
  float* rows;   // the draw's [T][N] plane, offset to the chunk's first frame
  int N, n;
  EKS_HD void operator()(int i, float x) const { EKS_STREAM_STORE(rows + (size_t)i * (size_t)N + (unsigned)n, x); }
};

template <int B, bool UNIT, bool INJ>
EKS_HD void sample_replay_lane(const SampleWs& W, const DiagModel& M, const SampleCall& c, int n, int j) {
  const ChainParams<float> p = load_chain_params(M, n);
  const int t0 = j * B, len = c.T - t0 < B ? c.T - t0 : B;
  const size_t o = (size_t)j * W.N + n;
  float v0[B], v1[B], v2[B];
  load_chunk<B>(c.y, c.var, W.N, n, t0, len, v0, v1);
  chunk_means_gains<B, UNIT>(v0, v1, v2, len, j == W.nc - 1, p, W.pm[o], W.pP[o], W.sEta[o], W.sJ[o]);
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
