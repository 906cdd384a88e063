// Host-side simulator of the posterior sampler's float32 arithmetic on scalar chains.  TEST INFRASTRUCTURE ONLY: it
// calls the lane bodies the gfx950 kernels call (eks_amd/csrc/eks_sample_lane.hpp) from plain loops, in the kernels'
// order of passes.  It is not a fallback: nothing under eks_amd/ loads it.
#include <algorithm>
#include <vector>

#include "eks_sample_lane.hpp"

using namespace eks;

template <int B, bool UNIT>
static void run(int T, int N, const DiagModel& M, const SampleCall& c, int n_draws, int gs) {
  SampleWs W;
  W.N = N;
  W.nc = (T + B - 1) / B;
  W.gs = gs;
  W.ng = (W.nc + gs - 1) / gs;
  W.n_draws = n_draws;
  const size_t pc = (size_t)W.nc * N, pg = (size_t)W.ng * N;
  std::vector<float> buf(10 * pc + n_draws * pc + 10 * pg + n_draws * pg);
  float* at = buf.data();
  auto take = [&](size_t n) { float* p = at; at += n; return p; };
  W.eA = take(pc); W.eb = take(pc); W.eC = take(pc); W.eEta = take(pc); W.eJ = take(pc);
  W.pm = take(pc); W.pP = take(pc); W.sEta = take(pc); W.sJ = take(pc);
  W.gam = take(pc);
  W.beta = take(n_draws * pc);
  W.gA = take(pg); W.gb = take(pg); W.gC = take(pg); W.gEta = take(pg); W.gJ = take(pg);
  W.gm = take(pg); W.gP = take(pg); W.gsEta = take(pg); W.gsJ = take(pg);
  W.hG = take(pg);
  W.hB = take(n_draws * pg);
  const bool inj = c.noise != nullptr;
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < N; ++n) sample_summarize_lane<B, UNIT>(W, M, c, n, j);
  for (int g = 0; g < W.ng; ++g)
    for (int n = 0; n < N; ++n) kalman_group_reduce(W, n, g);
  for (int n = 0; n < N; ++n) {
    float m, P;
    load_chain_prior(M, n, m, P);
    kalman_group_scan(W, n, m, P);
  }
  for (int g = 0; g < W.ng; ++g)
    for (int n = 0; n < N; ++n) kalman_group_apply(W, n, g);
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
  if (gs <= 0) {
    const int nc = (T + B - 1) / B;
    gs = 1;
    while (gs * gs < nc) ++gs;
  }
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
