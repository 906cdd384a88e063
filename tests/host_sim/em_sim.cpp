// Host-side simulator of eks_em_stats' arithmetic on scalar chains.  TEST INFRASTRUCTURE ONLY: it calls the lane
// bodies the gfx950 kernels call (eks_amd/csrc/eks_em_lane.hpp) from plain loops, in the kernels' order of passes, and
// sums the chunk partials in em_reduce's order.  It is not a fallback: nothing under eks_amd/ loads it.
#include <vector>

#include "chain_sim.hpp"
#include "eks_em_lane.hpp"

using namespace eks;

template <int B, bool UNIT>
static void run(int T, int N, const DiagModel& M, const float* y, const float* var, int gs, double* Sw) {
  ChainSimWs S(T, N, B, gs, 0, true);
  const SampleWs& W = S.W;
  const SampleCall cs{y, var, nullptr, nullptr, nullptr, T, 0u, 0u, 0u, 0u};
  const EmCall c{y, var, S.part, T};
  chain_sim_forward<B, UNIT>(W, M, cs);
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < N; ++n) em_replay_lane<B, UNIT>(W, M, c, n, j);
  chain_sim_reduce(W, S.part, Sw);
}

// gs: chunks per scan group (<= 0: the library's choice, ceil(sqrt(number of chunks)))
extern "C" int sim_em(int T, int N, int D, int B, int gs, int unit, const float* y, const float* var, const double* m0,
                      const double* S0, const double* A, const double* C, const double* Q, const double* s, double* Sw) {
  const DiagModel M{m0, S0, A, C, Q, s, D};
#define RUN(BB)                                            \
  case BB:                                                 \
    if (unit) run<BB, true>(T, N, M, y, var, gs, Sw);      \
    else run<BB, false>(T, N, M, y, var, gs, Sw);          \
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

// one step: rts_step and rts_step_em on the same inputs (out: ms, Ps of each, then the step's term)
extern "C" void sim_rts_em_steps(int unit, float a, double oma, double oma2, float q_s, float ms, float Ps, float mf,
                                 float Pf, float* out) {
  ChainParams<float> p;
  p.a = a;
  p.c = 1.0f;
  p.q_s = q_s;
  p.oma = (float)oma;
  p.oma2 = (float)oma2;
  float m0 = ms, P0 = Ps, m1 = ms, P1 = Ps, term;
  if (unit) {
    rts_step<float, true>(m0, P0, mf, Pf, p);
    term = rts_step_em<float, true>(m1, P1, mf, Pf, p);
  } else {
    rts_step<float, false>(m0, P0, mf, Pf, p);
    term = rts_step_em<float, false>(m1, P1, mf, Pf, p);
  }
  out[0] = m0; out[1] = P0; out[2] = m1; out[3] = P1; out[4] = term;
}

// A stand-alone run for sanitizer builds of the lane header (g++ -fsanitize=address,undefined -DEM_SIM_MAIN): odd sizes
// through every chunk length; T = 1 must give exact zeros and every sum must be finite and non-negative.
#ifdef EM_SIM_MAIN
#include <cmath>
#include <cstdio>
int main() {
  int bad = 0;
  for (int B : {4, 8, 16, 32})
    for (int T : {1, 2, 31, 33, 129, 1000})
      for (int unit = 0; unit < 2; ++unit) {
        const int K = 3, D = 2, N = K * D;
        std::vector<float> y((size_t)T * N), var((size_t)T * N);
        for (size_t i = 0; i < y.size(); ++i) {
          y[i] = (float)((i * 37) % 101) * 0.1f;
          var[i] = 0.5f + (float)((i * 13) % 7);
        }
        std::vector<double> m0(N, 0.0), S0(K * D * D, 0.0), A(K * D * D, 0.0), C(K * D * D, 0.0), Q(K * D * D, 0.0), s(K, 2.0);
        for (int k = 0; k < K; ++k)
          for (int d = 0; d < D; ++d) {
            const size_t dd = (size_t)k * D * D + d * (D + 1);
            S0[dd] = 3.0; Q[dd] = 1.0;
            A[dd] = unit ? 1.0 : 0.98;
            C[dd] = unit ? 1.0 : 1.3;
          }
        std::vector<double> Sw(N, -1.0);
        bad += sim_em(T, N, D, B, 0, unit, y.data(), var.data(), m0.data(), S0.data(), A.data(), C.data(), Q.data(), s.data(),
                      Sw.data());
        for (int n = 0; n < N; ++n) bad += T == 1 ? Sw[n] != 0.0 : !(std::isfinite(Sw[n]) && Sw[n] > 0.0);
      }
  std::printf("em_sim: %s\n", bad ? "FAILED" : "ok");
  return bad != 0;
}
#endif
