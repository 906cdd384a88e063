// Host-side simulator of the posterior sampler's float32 arithmetic on scalar chains.  TEST INFRASTRUCTURE ONLY: it
// calls the lane bodies the gfx950 kernels call (eks_amd/csrc/eks_sample_lane.hpp) from plain loops, in the kernels'
// order of passes.  It is not a fallback: nothing under eks_amd/ loads it.
#include <algorithm>
#include <vector>

#include "chain_sim.hpp"

using namespace eks;

template <int B, bool UNIT>
static void run(int T, int N, const DiagModel& M, const SampleCall& c, int n_draws, int gs) {
  ChainSimWs S(T, N, B, gs, n_draws, false);
  const SampleWs& W = S.W;
  const bool inj = c.noise != nullptr;
  chain_sim_forward<B, UNIT>(W, M, c);
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < N; ++n) {
      if (inj) sample_beta_lane<B, UNIT, true>(W, M, c, n, j);
      else sample_beta_lane<B, UNIT, false>(W, M, c, n, j);
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
      if (inj) sample_replay_lane<B, UNIT, true>(W, M, c, n, j);
      else sample_replay_lane<B, UNIT, false>(W, M, c, n, j);
    }
}

// gs: chunks per scan group (<= 0: the library's choice, ceil(sqrt(number of chunks)))
extern "C" int sim_sample(int T, int N, int D, int B, int gs, int unit, const float* y, const float* var,
                          const double* m0, const double* S0, const double* A, const double* C, const double* Q,
                          const double* s, int n_draws, unsigned long long seed, int first_keypoint, int first_draw,
                          const float* noise, float* ms, float* draws) {
  const DiagModel M{m0, S0, A, C, Q, s, D};
  const SampleCall c{y, var, noise, ms, draws, T, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (uint32_t)first_keypoint * (uint32_t)D, (uint32_t)first_draw};
#define RUN(BB)                                        \
  case BB:                                             \
    if (unit) run<BB, true>(T, N, M, c, n_draws, gs);  \
    else run<BB, false>(T, N, M, c, n_draws, gs);      \
    break;
  switch (B) {
    RUN(4)
    RUN(8)
    RUN(16)
    RUN(32)
    default: return -1;
  }
#undef RUN
  return 0;
}

extern "C" void sim_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  const Philox4 w = philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
  for (int i = 0; i < 4; ++i) out[i] = w.x[i];
}

// the generator's normals, noise [n_draws][T][N]
extern "C" void sim_sample_noise(int T, int N, int n_draws, unsigned long long seed, int first_chain, int first_draw,
                                 float* noise) {
  for (int d = 0; d < n_draws; ++d)
    for (int tq = 0; 4 * tq < T; ++tq)
      for (int n = 0; n < N; ++n) {
        float z[4];
        NoiseGen{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(first_chain + n), (uint32_t)(first_draw + d)}.get4(tq, 4, z);
        for (int i = 0; i < 4 && 4 * tq + i < T; ++i) noise[((size_t)d * T + 4 * tq + i) * N + n] = z[i];
      }
}

// A stand-alone run for sanitizer builds of the lane header (g++ -fsanitize=address,undefined -DSAMPLE_SIM_MAIN): odd
// sizes through every chunk length, one and three draws, the generator's normals and the same normals injected - which
// must give the same bits; everything written must be finite.
#ifdef SAMPLE_SIM_MAIN
#include <cmath>
#include <cstdio>
#include <cstring>
int main() {
  int bad = 0;
  for (int B : {4, 8, 16, 32})
    for (int T : {1, 2, 31, 33, 129, 1000})
      for (int unit = 0; unit < 2; ++unit)
        for (int n_draws : {1, 3}) {
          const int K = 3, D = 2, N = K * D;
          std::vector<float> y((size_t)T * N), var((size_t)T * N);
          for (size_t i = 0; i < y.size(); ++i) {
            y[i] = (float)((i * 37) % 101) * 0.1f;
            var[i] = 0.5f + (float)((i * 13) % 7);
          }
          std::vector<double> m0(N, 0.0), S0(K * D * D, 0.0), A(K * D * D, 0.0), C(K * D * D, 0.0), Q(K * D * D, 0.0),
              s(K, 2.0);
          for (int k = 0; k < K; ++k)
            for (int d = 0; d < D; ++d) {
              const size_t dd = (size_t)k * D * D + d * (D + 1);
              S0[dd] = 3.0; Q[dd] = 1.0;
              A[dd] = unit ? 1.0 : 0.98;
              C[dd] = unit ? 1.0 : 1.3;
            }
          const size_t TN = (size_t)T * N;
          std::vector<float> noise(n_draws * TN), ms(TN, NAN), draws(n_draws * TN, NAN), ms2(TN, NAN), draws2(n_draws * TN, NAN);
          sim_sample_noise(T, N, n_draws, 1234u, 0, 0, noise.data());
          bad += sim_sample(T, N, D, B, 0, unit, y.data(), var.data(), m0.data(), S0.data(), A.data(), C.data(), Q.data(),
                            s.data(), n_draws, 1234u, 0, 0, nullptr, ms.data(), draws.data());
          bad += sim_sample(T, N, D, B, 0, unit, y.data(), var.data(), m0.data(), S0.data(), A.data(), C.data(), Q.data(),
                            s.data(), n_draws, 1234u, 0, 0, noise.data(), ms2.data(), draws2.data());
          for (size_t i = 0; i < TN; ++i) bad += !std::isfinite(ms[i]);
          for (size_t i = 0; i < draws.size(); ++i) bad += !std::isfinite(draws[i]);
          bad += std::memcmp(ms.data(), ms2.data(), TN * sizeof(float)) != 0;
          bad += std::memcmp(draws.data(), draws2.data(), draws.size() * sizeof(float)) != 0;
        }
  std::printf("sample_sim: %s\n", bad ? "FAILED" : "ok");
  return bad != 0;
}
#endif
