// What the scalar-chain simulators (em_sim, increments_sim, innov_sim, sample_sim, smooth_tv_sim) share.  TEST
// INFRASTRUCTURE ONLY.  Geometry and planes come from the library's own chain_geometry / chain_layout
// (eks_amd/csrc/eks_chain_plan.hpp) on a heap buffer of exactly the size the layout reports, so a sanitizer build sees
// any plane the layout hands out beyond what it counts; the forward passes are eks_chain.hip's launches as plain loops.
#pragma once
#include <algorithm>
#include <vector>

#include "eks_chain_plan.hpp"

namespace eks {

// gs <= 0: the library's choice.  Planes are packed to their element size (8 bytes with the float64 plane, which has to
// stay aligned), not to the library's 256.
struct ChainSimWs {
  std::vector<char> buf;
  SampleWs W;
  double* part = nullptr;   // [nc][N], -1 everywhere

  ChainSimWs(int T, int N, int B, int gs, int n_draws, bool with_part) {
    const ChainGeometry g = chain_geometry(T, B, gs);
    const size_t align = with_part ? sizeof(double) : sizeof(float);
    buf.resize(chain_layout(N, g, n_draws, with_part, align, nullptr));
    chain_layout(N, g, n_draws, with_part, align, buf.data(), &W, &part);
    if (part) std::fill(part, part + (size_t)g.nc * N, -1.0);
  }
};

// S1: reduce, scan, apply
inline void chain_sim_scan(const SampleWs& W, const DiagModel& M) {
  for (int g = 0; g < W.ng; ++g)
    for (int n = 0; n < W.N; ++n) kalman_group_reduce(W, n, g);
  for (int n = 0; n < W.N; ++n) {
    float m, P;
    load_chain_prior(M, n, m, P);
    kalman_group_scan(W, n, m, P);
  }
  for (int g = 0; g < W.ng; ++g)
    for (int n = 0; n < W.N; ++n) kalman_group_apply(W, n, g);
}

// summarize + S1
template <int B, bool UNIT>
inline void chain_sim_forward(const SampleWs& W, const DiagModel& M, const SampleCall& c) {
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < W.N; ++n) sample_summarize_lane<B, UNIT>(W, M, c, n, j);
  chain_sim_scan(W, M);
}

// em_reduce's order: 16 contiguous runs of ceil(nc / 16) chunks, then the run sums in run order
inline void chain_sim_reduce(const SampleWs& W, const double* part, double* out) {
  const int per = (W.nc + 15) / 16;
  for (int n = 0; n < W.N; ++n) {
    double total = 0.0;
    for (int r = 0; r < 16; ++r) {
      double acc = 0.0;
      for (int j = r * per; j < W.nc && j < (r + 1) * per; ++j) acc += part[(size_t)j * W.N + n];
      total += acc;
    }
    out[n] = total;
  }
}

}  // namespace eks
