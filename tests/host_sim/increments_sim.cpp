// Host-side simulator of eks_smooth_increments' float32 arithmetic on scalar chains.  TEST INFRASTRUCTURE ONLY: it
// calls the lane bodies the gfx950 kernels call (eks_amd/csrc/eks_increments_lane.hpp) from plain loops, in the
// kernels' order of passes.  It is not a fallback: nothing under eks_amd/ loads it.
#include <vector>

#include "chain_sim.hpp"
#include "eks_increments_lane.hpp"

using namespace eks;

// plain != 0: the last pass is eks_smooth's own replay (replay_chunk -> smooth_rows) on the same scan results; it
// writes ms and Vs only - what the increments replay has to reproduce bit for bit.
template <int B, bool UNIT>
static void run(int T, int N, const DiagModel& M, const IncrementsCall& c, int gs, int plain) {
  ChainSimWs S(T, N, B, gs, 0, false);
  const SampleWs& W = S.W;
  const SampleCall cs{c.y, c.var, nullptr, nullptr, nullptr, T, 0u, 0u, 0u, 0u};
  chain_sim_forward<B, UNIT>(W, M, cs);
  const bool all = c.ms && c.Vs && c.lag1 && c.dmean && c.dV;
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < N; ++n) {
      if (plain) {
        const size_t o = (size_t)j * N + n;
        const int t0 = j * B, len = T - t0 < B ? T - t0 : B;
        replay_chunk<B, UNIT, 0>(c.y, c.var, c.ms, c.Vs, N, n, n % M.D, t0, len, load_chain_params(M, n), W.pm[o],
                                 W.pP[o], W.sEta[o], W.sJ[o]);
      } else if (all) {
        increments_replay_lane<B, UNIT, true>(W, M, c, n, j);
      } else {
        increments_replay_lane<B, UNIT, false>(W, M, c, n, j);
      }
    }
}

// gs: chunks per scan group (<= 0: the library's choice, ceil(sqrt(number of chunks)))
extern "C" int sim_increments(int T, int N, int D, int B, int gs, int unit, int plain, const float* y, const float* var,
                              const double* m0, const double* S0, const double* A, const double* C, const double* Q,
                              const double* s, float* ms, float* Vs, float* lag1, float* dmean, float* dV) {
  const DiagModel M{m0, S0, A, C, Q, s, D};
  const IncrementsCall c{y, var, ms, Vs, lag1, dmean, dV, T};
#define RUN(BB)                                         \
  case BB:                                              \
    if (unit) run<BB, true>(T, N, M, c, gs, plain);     \
    else run<BB, false>(T, N, M, c, gs, plain);         \
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

// one step: rts_step and rts_step_increments on the same inputs (out: ms, Ps of each, then lag1, dmean, dV)
extern "C" void sim_rts_steps(int unit, float a, double oma, double oma2, float q_s, float ms, float Ps, float mf, float Pf,
                              float* out) {
  ChainParams<float> p;
  p.a = a;
  p.c = 1.0f;
  p.q_s = q_s;
  p.oma = (float)oma;
  p.oma2 = (float)oma2;
  float m0 = ms, P0 = Ps, m1 = ms, P1 = Ps, l, dm, dv;
  if (unit) {
    rts_step<float, true>(m0, P0, mf, Pf, p);
    rts_step_increments<float, true>(m1, P1, mf, Pf, p, l, dm, dv);
  } else {
    rts_step<float, false>(m0, P0, mf, Pf, p);
    rts_step_increments<float, false>(m1, P1, mf, Pf, p, l, dm, dv);
  }
  out[0] = m0; out[1] = P0; out[2] = m1; out[3] = P1; out[4] = l; out[5] = dm; out[6] = dv;
}

// A stand-alone run for sanitizer builds of the lane header (g++ -fsanitize=address,undefined -DINCREMENTS_SIM_MAIN):
// odd sizes through every chunk length, all outputs and a NULL mix.
#ifdef INCREMENTS_SIM_MAIN
#include <cstdio>
int main() {
  int bad = 0;
  for (int B : {4, 8, 16, 32})
    for (int T : {1, 2, 31, 33, 129, 1000})
      for (int unit = 0; unit < 2; ++unit) {
        const int K = 3, D = 2, N = K * D;
        std::vector<float> y((size_t)T * N), var((size_t)T * N), o[5];
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
        for (auto& v : o) v.assign((size_t)T * N, -1.0f);
        bad += sim_increments(T, N, D, B, 0, unit, 0, y.data(), var.data(), m0.data(), S0.data(), A.data(), C.data(), Q.data(),
                              s.data(), o[0].data(), o[1].data(), o[2].data(), o[3].data(), o[4].data());
        bad += sim_increments(T, N, D, B, 0, unit, 0, y.data(), var.data(), m0.data(), S0.data(), A.data(), C.data(), Q.data(),
                              s.data(), nullptr, o[1].data(), nullptr, o[3].data(), nullptr);
        for (int n = 0; n < N; ++n) bad += o[2][(size_t)(T - 1) * N + n] != 0.0f || o[4][(size_t)(T - 1) * N + n] != 0.0f;
      }
  std::printf("increments_sim: %s\n", bad ? "FAILED" : "ok");
  return bad != 0;
}
#endif
