// Host-side simulator of eks_sample_tv's float32 arithmetic on scalar chains.  TEST INFRASTRUCTURE ONLY: it calls the
// lane bodies the gfx950 kernels call (eks_amd/csrc/eks_sample_tv_lane.hpp, unchanged) from plain loops, in the
// kernels' order of passes.  It is not a fallback: nothing under eks_amd/ loads it.
#include <algorithm>
#include <vector>

#include "chain_sim.hpp"
#include "eks_sample_tv_lane.hpp"

using namespace eks;

template <int B, bool UNIT, bool HAS_W>
static void run(int T, int N, const DiagModel& M, const SampleTvCall& c, int n_draws, int gs) {
  ChainSimWs S(T, N, B, gs, n_draws, false);
  const SampleWs& W = S.W;
  const bool inj = c.noise != nullptr;
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < N; ++n) sample_tv_summarize_lane<B, UNIT, HAS_W>(W, M, c, n, j);
  chain_sim_scan(W, M);
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < N; ++n) {
      if (inj) sample_beta_tv_lane<B, UNIT, true, HAS_W>(W, M, c, n, j);
      else sample_beta_tv_lane<B, UNIT, false, HAS_W>(W, M, c, n, j);
    }
  for (int d = 0; d < n_draws; ++d) {
    for (int g = 0; g < W.ng; ++g)
      for (int n = 0; n < N; ++n) draw_group_reduce(W, n, g, d);
    for (int n = 0; n < N; ++n) draw_group_scan(W, n, d);
    for (int g = 0; g < W.ng; ++g)
      for (int n = 0; n < N; ++n) draw_group_apply(W, n, g, d);
  }
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < N; ++n) {
      if (inj) sample_replay_tv_lane<B, UNIT, true, HAS_W>(W, M, c, n, j);
      else sample_replay_tv_lane<B, UNIT, false, HAS_W>(W, M, c, n, j);
    }
}

// B: frames per chunk, a multiple of 4 in 4 .. 32; gs: chunks per scan group (<= 0: the library's choice).  qscale [T]
// or [T][K] (per_keypoint) or null; weights [T][N] or null.
extern "C" int sim_sample_tv(int T, int N, int D, int B, int gs, int unit, const float* y, const float* var,
                             const float* qscale, int per_keypoint, const float* weights, const double* m0,
                             const double* S0, const double* A, const double* C, const double* Q, const double* s,
                             int n_draws, unsigned long long seed, int first_keypoint, int first_draw,
                             const float* noise, float* ms, float* draws) {
  const DiagModel M{m0, S0, A, C, Q, s, D};
  const SampleTvCall c{y, var, qscale, weights, noise, ms, draws, T, N / D, per_keypoint ? 1 : 0, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)first_keypoint * (uint32_t)D, (uint32_t)first_draw};
#define RUN(BB)                                                       \
  case BB:                                                            \
    if (unit && weights) run<BB, true, true>(T, N, M, c, n_draws, gs);        \
    else if (unit) run<BB, true, false>(T, N, M, c, n_draws, gs);             \
    else if (weights) run<BB, false, true>(T, N, M, c, n_draws, gs);          \
    else run<BB, false, false>(T, N, M, c, n_draws, gs);                      \
    break;
  switch (B) {
    RUN(4)
    RUN(8)
    RUN(12)
    RUN(16)
    RUN(20)
    RUN(24)
    RUN(28)
    RUN(32)
    default: return -1;
  }
#undef RUN
  return 0;
}

// A stand-alone run for sanitizer builds of the lane header (g++ -fsanitize=address,undefined -DSAMPLE_TV_SIM_MAIN): odd
// sizes through every chunk length, planes present and absent, exactly sized buffers (a read of w[T] or of a weight
// past the last frame is out of bounds), the generator against the same normals injected - which must give the same
// bits; everything written must be finite.
#ifdef SAMPLE_TV_SIM_MAIN
#include <cmath>
#include <cstdio>
#include <cstring>
int main() {
  int bad = 0;
  for (int B : {4, 8, 12, 16, 20, 24, 28, 32})
    for (int T : {1, 2, 31, 33, 129, 1000})
      for (int unit = 0; unit < 2; ++unit)
        for (int planes = 0; planes < 4; ++planes) {   // bit 0: qscale (per keypoint when T is odd), bit 1: weights
          const int K = 3, D = 2, N = K * D, n_draws = 1 + planes % 3;
          const int pk = T & 1;
          std::vector<float> y((size_t)T * N), var((size_t)T * N), lam((size_t)T * N), w((size_t)T * (pk ? K : 1));
          for (size_t i = 0; i < y.size(); ++i) {
            y[i] = (float)((i * 37) % 101) * 0.1f;
            var[i] = 0.5f + (float)((i * 13) % 7);
            lam[i] = i % 11 == 0 ? 1e-30f : (i % 7 == 0 ? 1.25f : 0.05f + (float)((i * 5) % 9) * 0.1f);
          }
          for (size_t i = 0; i < w.size(); ++i) w[i] = i % 9 == 0 ? 1e3f : (i % 5 == 0 ? 1e-3f : 1.0f + (float)(i % 3));
          w[0] = NAN;                                  // row 0 is never read
          std::vector<double> m0(N, 0.0), S0(K * D * D, 0.0), A(K * D * D, 0.0), C(K * D * D, 0.0), Q(K * D * D, 0.0),
              s(K, 2.0);
          for (int k = 0; k < K; ++k)
            for (int d = 0; d < D; ++d) {
              const size_t dd = (size_t)k * D * D + d * (D + 1);
              S0[dd] = 3.0; Q[dd] = 1.0;
              A[dd] = unit ? 1.0 : 0.98;
              C[dd] = unit ? 1.0 : -1.3;
            }
          const float* wp = (planes & 1) ? w.data() : nullptr;
          const float* lp = (planes & 2) ? lam.data() : nullptr;
          const size_t TN = (size_t)T * N;
          std::vector<float> noise(n_draws * TN), ms(TN, NAN), draws(n_draws * TN, NAN), ms2(TN, NAN), draws2(n_draws * TN, NAN);
          for (int d = 0; d < n_draws; ++d)
            for (int tq = 0; 4 * tq < T; ++tq)
              for (int n = 0; n < N; ++n) {
                float z[4];
                NoiseGen{1234u, 0u, (uint32_t)n, (uint32_t)d}.get4(tq, 4, z);
                for (int i = 0; i < 4 && 4 * tq + i < T; ++i) noise[((size_t)d * T + 4 * tq + i) * N + n] = z[i];
              }
          bad += sim_sample_tv(T, N, D, B, 0, unit, y.data(), var.data(), wp, pk, lp, m0.data(), S0.data(), A.data(),
                               C.data(), Q.data(), s.data(), n_draws, 1234u, 0, 0, nullptr, ms.data(), draws.data());
          bad += sim_sample_tv(T, N, D, B, 0, unit, y.data(), var.data(), wp, pk, lp, m0.data(), S0.data(), A.data(),
                               C.data(), Q.data(), s.data(), n_draws, 1234u, 0, 0, noise.data(), ms2.data(), draws2.data());
          for (size_t i = 0; i < TN; ++i) bad += !std::isfinite(ms[i]);
          for (size_t i = 0; i < draws.size(); ++i) bad += !std::isfinite(draws[i]);
          bad += std::memcmp(ms.data(), ms2.data(), TN * sizeof(float)) != 0;
          bad += std::memcmp(draws.data(), draws2.data(), draws.size() * sizeof(float)) != 0;
        }
  std::printf("sample_tv_sim: %s\n", bad ? "FAILED" : "ok");
  return bad != 0;
}
#endif
