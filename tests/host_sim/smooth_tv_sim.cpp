// Host-side simulator of eks_smooth_tv's arithmetic on scalar chains.  TEST INFRASTRUCTURE ONLY: it calls the lane
// bodies the gfx950 kernels call (eks_amd/csrc/eks_smooth_tv_lane.hpp) from plain loops, in the kernels' order of
// passes.  It is not a fallback: nothing under eks_amd/ loads it.
#include <cstring>
#include <vector>

#include "chain_sim.hpp"
#include "eks_smooth_tv_lane.hpp"

using namespace eks;

struct RowsOut {
  float *m, *P;   // [B] each
  void operator()(int i, float mm, float PP) const { m[i] = mm; P[i] = PP; }
};

static bool same(const float* a, const float* b, int n) { return std::memcmp(a, b, sizeof(float) * n) == 0; }

// Runs the five passes into ms / Vs [T][N] (diagonal form).  compare != 0 (meaningful when every w that is read is 1):
// returns the number of (chain, chunk) lanes in which the element, the belief carried over the chunk or any output
// differs in any bit from summarize_loaded / filter_loaded / smooth_rows on the same inputs; else returns 0.
template <int B, bool UNIT>
static int run(int T, int N, int K, const DiagModel& M, const float* y, const float* var, const float* qscale,
               int per_keypoint, int gs, int compare, float* ms, float* Vs) {
  ChainSimWs S(T, N, B, gs, 0, false);
  const SampleWs& W = S.W;
  const SmoothTvCall c{y, var, qscale, ms, Vs, T, K, per_keypoint};
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < N; ++n) smooth_tv_summarize_lane<B, UNIT>(W, M, c, n, j);
  chain_sim_scan(W, M);
  int mismatches = 0;
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < N; ++n) {
      smooth_tv_replay_lane<B, UNIT, 0>(W, M, c, n, j);
      if (!compare) continue;
      const ChainParams<float> p = load_chain_params(M, n);
      const NoiseScale ns = chain_noise_scale(qscale, per_keypoint, K, M.D, n, T);
      const int t0 = j * B, len = T - t0 < B ? T - t0 : B;
      const size_t o = (size_t)j * N + n;
      float a0[B], a1[B], b0[B], b1[B], qv[B];
      load_chunk<B>(y, var, N, n, t0, len, a0, a1);
      load_chunk<B>(y, var, N, n, t0, len, b0, b1);
      load_chunk_noise<B>(ns, t0, len, p.q_s, qv);
      bool bad = false;
      // the element
      const Elem<float> e1 = summarize_loaded<B, UNIT>(a0, a1, len, p);
      const Elem<float> e2 = summarize_loaded_tv<B, UNIT>(b0, b1, qv, len, p);
      const float f1[5] = {e1.A, e1.b, e1.C, e1.eta, e1.J}, f2[5] = {e2.A, e2.b, e2.C, e2.eta, e2.J};
      const float f3[5] = {W.eA[o], W.eb[o], W.eC[o], W.eEta[o], W.eJ[o]};
      bad |= !same(f1, f2, 5) || !same(f1, f3, 5);
      // the carried belief and the filtered pairs
      float m1 = W.pm[o], P1 = W.pP[o], m2 = m1, P2 = P1;
      filter_loaded<B, UNIT>(a0, a1, len, p, m1, P1);
      filter_loaded_tv<B, UNIT>(b0, b1, qv, len, p, m2, P2);
      bad |= !same(&m1, &m2, 1) || !same(&P1, &P2, 1) || !same(a0, b0, len) || !same(a1, b1, len);
      // the outputs
      fuse_info(m1, P1, W.sEta[o], W.sJ[o]);
      float om[B], oP[B], tm[B], tP[B];
      smooth_rows<B, UNIT>(a0, a1, len, p, m1, P1, RowsOut{om, oP});
      smooth_rows_tv<B, UNIT>(b0, b1, qv, len, p, m1, P1, RowsOut{tm, tP});
      bad |= !same(om, tm, len) || !same(oP, tP, len);
      for (int i = 0; i < len; ++i)
        bad |= !same(om + i, ms + (size_t)(t0 + i) * N + n, 1) || !same(oP + i, Vs + (size_t)(t0 + i) * N + n, 1);
      mismatches += bad;
    }
  return mismatches;
}

// gs: chunks per scan group (<= 0: the library's choice, ceil(sqrt(number of chunks))).  qscale [T] or [T][K];
// ms, Vs [T][N].  Returns the number of mismatching lanes (compare != 0), 0, or -1 for an unknown chunk length.
extern "C" int sim_smooth_tv(int T, int N, int D, int B, int gs, int unit, const float* y, const float* var,
                             const float* qscale, int per_keypoint, const double* m0, const double* S0, const double* A,
                             const double* C, const double* Q, const double* s, int compare, float* ms, float* Vs) {
  const DiagModel M{m0, S0, A, C, Q, s, D};
  const int K = N / D;
#define RUN(BB)                                                                                           \
  case BB:                                                                                                \
    return unit ? run<BB, true>(T, N, K, M, y, var, qscale, per_keypoint, gs, compare, ms, Vs)            \
                : run<BB, false>(T, N, K, M, y, var, qscale, per_keypoint, gs, compare, ms, Vs);
  switch (B) {
    RUN(4)
    RUN(8)
    RUN(16)
    RUN(32)
    default: return -1;
  }
#undef RUN
}

// A stand-alone run for sanitizer builds of the lane header (g++ -fsanitize=address,undefined -DSMOOTH_TV_SIM_MAIN):
// odd sizes through every chunk length with exactly sized buffers, shared and per-keypoint w with zeros and a large
// value; everything written must be finite and every variance positive.
#ifdef SMOOTH_TV_SIM_MAIN
#include <cmath>
#include <cstdio>
int main() {
  int bad = 0;
  for (int B : {4, 8, 16, 32})
    for (int T : {1, 2, 3, 31, 32, 33, 129, 1000})
      for (int unit = 0; unit < 2; ++unit)
        for (int pk = 0; pk < 2; ++pk) {
          const int K = 3, D = 2, N = K * D;
          std::vector<float> y((size_t)T * N), var((size_t)T * N), w((size_t)T * (pk ? K : 1));
          for (size_t i = 0; i < y.size(); ++i) {
            y[i] = (float)((i * 37) % 101) * 0.1f;
            var[i] = 0.5f + (float)((i * 13) % 7);
          }
          for (size_t i = 0; i < w.size(); ++i) w[i] = i % 11 == 3 ? 0.0f : (i % 17 == 5 ? 1e4f : 0.25f * (float)(i % 9 + 1));
          w[0] = NAN;   // never read
          std::vector<double> m0(N, 0.0), S0(K * D * D, 0.0), A(K * D * D, 0.0), C(K * D * D, 0.0), Q(K * D * D, 0.0),
              s(K, 2.0);
          for (int k = 0; k < K; ++k)
            for (int d = 0; d < D; ++d) {
              const size_t dd = (size_t)k * D * D + d * (D + 1);
              S0[dd] = 3.0; Q[dd] = 1.0;
              A[dd] = unit ? 1.0 : 0.98;
              C[dd] = unit ? 1.0 : 1.3;
            }
          std::vector<float> ms((size_t)T * N, NAN), Vs((size_t)T * N, NAN);
          bad += sim_smooth_tv(T, N, D, B, 0, unit, y.data(), var.data(), w.data(), pk, m0.data(), S0.data(), A.data(),
                               C.data(), Q.data(), s.data(), 0, ms.data(), Vs.data()) != 0;
          for (size_t i = 0; i < ms.size(); ++i) bad += !std::isfinite(ms[i]) || !(std::isfinite(Vs[i]) && Vs[i] > 0.0f);
        }
  std::printf("smooth_tv_sim: %s\n", bad ? "FAILED" : "ok");
  return bad != 0;
}
#endif
