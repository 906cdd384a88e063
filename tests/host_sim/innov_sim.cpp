// Host-side simulator of eks_innovations' arithmetic on scalar chains.  TEST INFRASTRUCTURE ONLY: it calls the lane
// bodies the gfx950 kernels call (eks_amd/csrc/eks_innov_lane.hpp) from plain loops, in the kernels' order of passes,
// and sums the chunk partials in em_reduce's order.  It is not a fallback: nothing under eks_amd/ loads it.
#include <cstring>
#include <vector>

#include "chain_sim.hpp"
#include "eks_innov_lane.hpp"

using namespace eks;

struct NoStore {
  void operator()(int, float, float) const {}
};

// returns the number of (chain, chunk) lanes whose carried belief differs in any bit from filter_loaded's
template <int B, bool UNIT>
static int run(int T, int N, const DiagModel& M, const float* y, const float* var, int gs, float* innov,
               float* innov_var, double* loglik) {
  ChainSimWs S(T, N, B, gs, 0, true);
  const SampleWs& W = S.W;
  const SampleCall cs{y, var, nullptr, nullptr, nullptr, T, 0u, 0u, 0u, 0u};
  const InnovCall c{y, var, innov, innov_var, loglik ? S.part : nullptr, T};
  chain_sim_forward<B, UNIT>(W, M, cs);
  int mismatches = 0;
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < N; ++n) {
      innov_replay_lane<B, UNIT>(W, M, c, n, j);
      // the belief carried over the chunk: innov_rows against filter_loaded, from the same entry belief
      const ChainParams<float> p = load_chain_params(M, n);
      const int t0 = j * B, len = T - t0 < B ? T - t0 : B;
      const size_t o = (size_t)j * N + n;
      float a0[B], a1[B], b0[B], b1[B];
      load_chunk<B>(y, var, N, n, t0, len, a0, a1);
      load_chunk<B>(y, var, N, n, t0, len, b0, b1);
      float m1 = W.pm[o], P1 = W.pP[o], m2 = m1, P2 = P1;
      filter_loaded<B, UNIT>(a0, a1, len, p, m1, P1);
      innov_rows<B, UNIT>(b0, b1, len, p, m2, P2, false, NoStore{});
      mismatches += std::memcmp(&m1, &m2, 4) != 0 || std::memcmp(&P1, &P2, 4) != 0;
    }
  if (loglik) chain_sim_reduce(W, S.part, loglik);
  return mismatches;
}

// gs: chunks per scan group (<= 0: the library's choice, ceil(sqrt(number of chunks))).  innov, innov_var [T][N] and
// loglik [N] may each be null.  Returns the number of lanes whose carried belief is not filter_loaded's, or -1.
extern "C" int sim_innov(int T, int N, int D, int B, int gs, int unit, const float* y, const float* var,
                         const double* m0, const double* S0, const double* A, const double* C, const double* Q,
                         const double* s, float* innov, float* innov_var, double* loglik) {
  const DiagModel M{m0, S0, A, C, Q, s, D};
#define RUN(BB)                                                                          \
  case BB:                                                                               \
    return unit ? run<BB, true>(T, N, M, y, var, gs, innov, innov_var, loglik)           \
                : run<BB, false>(T, N, M, y, var, gs, innov, innov_var, loglik);
  switch (B) {
    RUN(4)
    RUN(8)
    RUN(16)
    RUN(32)
    default: return -1;
  }
#undef RUN
}

// A stand-alone run for sanitizer builds of the lane header (g++ -fsanitize=address,undefined -DINNOV_SIM_MAIN): odd
// sizes through every chunk length, with every combination of absent outputs; everything written must be finite.
#ifdef INNOV_SIM_MAIN
#include <cmath>
#include <cstdio>
int main() {
  int bad = 0;
  for (int B : {4, 8, 16, 32})
    for (int T : {1, 2, 31, 33, 129, 1000})
      for (int unit = 0; unit < 2; ++unit)
        for (int mask = 1; mask < 8; ++mask) {
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
          std::vector<float> v((size_t)T * N, NAN), S((size_t)T * N, NAN);
          std::vector<double> ll(N, NAN);
          bad += sim_innov(T, N, D, B, 0, unit, y.data(), var.data(), m0.data(), S0.data(), A.data(), C.data(), Q.data(),
                           s.data(), mask & 1 ? v.data() : nullptr, mask & 2 ? S.data() : nullptr,
                           mask & 4 ? ll.data() : nullptr);
          for (size_t i = 0; i < v.size(); ++i) {
            if (mask & 1) bad += !std::isfinite(v[i]);
            if (mask & 2) bad += !(std::isfinite(S[i]) && S[i] > 0.0f);
          }
          if (mask & 4)
            for (int n = 0; n < N; ++n) bad += !std::isfinite(ll[n]);
        }
  std::printf("innov_sim: %s\n", bad ? "FAILED" : "ok");
  return bad != 0;
}
#endif
