// Host-side simulator of eks_smooth_increments and eks_em_stats on general (D, O) models.  TEST INFRASTRUCTURE ONLY: it
// calls the lane bodies the gfx950 kernels call (eks_amd/csrc/eks_increments_lane.hpp: dense_increments_chunk,
// eks_em_lane.hpp: dense_em_chunk - both the forward pass and the backward walker of eks_dense_lane.hpp) from plain
// loops over chunked sequences, the way dense_sim.cpp's sim_dense_smooth drives the replay: chunk elements, the scan as
// sequential applies / pull-backs, then every chunk from its own boundary.  It is not a fallback: nothing under
// eks_amd/ loads it.
#include <algorithm>
#include <vector>

#include "eks_em_lane.hpp"

using namespace eks;

// fn(k, j, t0, len, F, sQ, fid, m, P, eta, J) for every chunk j of every keypoint k, with the chunk's boundary: (m, P)
// the filtered belief of frame t0 - 1 (the prior itself for chunk 0), (eta, J) what all later frames say about the
// chunk's last frame.
template <int D, typename Fn>
static void for_each_chunk(int T, int K, int O, int B, const float* y, const float* var, const DenseModelPtrs& M,
                           const double* s, Fn&& fn) {
  const int nc = (T + B - 1) / B;
  for (int k = 0; k < K; ++k) {
    Mat<double, D> F, sQ;
    bool fid;
    load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
    std::vector<DElem<double, D>> el(nc);
    for (int j = 0; j < nc; ++j)
      el[j] = dense_smooth_element<D>(y, var, K, O, k, j * B, std::min(B, T - j * B), M, F, sQ, fid);
    std::vector<Vec<double, D>> pm(nc), se(nc);
    std::vector<Mat<double, D>> pP(nc), sJ(nc);
    Vec<double, D> m;
    Mat<double, D> P;
    load_prior<D>(M, k, m, P);
    belief_update_frame<D>(y, var, K, O, k, 0, M, m, P);
    for (int j = 0; j < nc; ++j) {
      pm[j] = m;
      pP[j] = P;
      delem_apply(el[j], m, P);
    }
    Vec<double, D> eta = vec_zero<double, D>();
    Mat<double, D> J = mat_zero<double, D>();
    for (int j = nc - 1; j >= 0; --j) {
      se[j] = eta;
      sJ[j] = J;
      delem_back(el[j], eta, J);
    }
    load_prior<D>(M, k, pm[0], pP[0]);
    for (int j = 0; j < nc; ++j) fn(k, j, j * B, std::min(B, T - j * B), F, sQ, fid, pm[j], pP[j], se[j], sJ[j]);
  }
}

template <int D>
static void increments_sim(int T, int K, int O, int B, const float* y, const float* var, const DenseModelPtrs& M,
                           const double* s, const DenseIncrementsOut& out) {
  std::vector<double> filt((size_t)B * (D + D * D));
  const LinearObs<D> obs = make_linear_obs<D>(y, var, K, O, M);
  for_each_chunk<D>(T, K, O, B, y, var, M, s, [&](int k, int, int t0, int len, auto&... boundary) {
    dense_increments_chunk<D>(obs, K, k, t0, len, boundary..., filt.data(), out, 1);
  });
}

// Sw [K][w], w = D * D or (diag) D: the chunk partials [chunk][keypoint][w] summed in em_reduce's order (eks_em.hip):
// 16 contiguous runs of ceil(nc / 16) chunks in chunk order, then the runs in run order.
template <int D>
static void em_sim(int T, int K, int O, int B, const float* y, const float* var, const DenseModelPtrs& M,
                   const double* s, bool diag, double* Sw) {
  const int nc = (T + B - 1) / B, w = diag ? D : D * D, ne = K * w;
  std::vector<double> filt((size_t)B * (D + D * D)), part((size_t)nc * ne, -1.0);
  const LinearObs<D> obs = make_linear_obs<D>(y, var, K, O, M);
  for_each_chunk<D>(T, K, O, B, y, var, M, s, [&](int k, int j, int t0, int len, auto&... boundary) {
    dense_em_chunk<D>(obs, k, t0, len, boundary..., filt.data(), 1, part.data() + ((size_t)j * K + k) * w, diag);
  });
  const int per = (nc + 15) / 16;
  for (int e = 0; e < ne; ++e) {
    double total = 0.0;
    for (int seg = 0; seg < 16; ++seg) {
      double acc = 0.0;
      for (int j = seg * per; j < std::min(nc, (seg + 1) * per); ++j) acc += part[(size_t)j * ne + e];
      total += acc;
    }
    Sw[e] = total;
  }
}

// ms, dmean [T][K][D]; Vs, lag1, dV [T][K][D][D] or (vs_diag) [T][K][D]; any output may be null
extern "C" int sim_dense_increments(int T, int K, int D, int O, int B, int vs_diag, const float* y, const float* var,
                                    const double* m0, const double* S0, const double* A, const double* C,
                                    const double* Q, const double* s, float* ms, float* Vs, float* lag1,
                                    float* dmean, float* dV) {
  const DenseModelPtrs M{m0, S0, A, C, Q};
  const DenseIncrementsOut out{ms, Vs, lag1, dmean, dV, vs_diag != 0, T};
  switch (D) {
    case 1: increments_sim<1>(T, K, O, B, y, var, M, s, out); return 0;
    case 2: increments_sim<2>(T, K, O, B, y, var, M, s, out); return 0;
    case 3: increments_sim<3>(T, K, O, B, y, var, M, s, out); return 0;
    default: return -3;
  }
}

extern "C" int sim_dense_em(int T, int K, int D, int O, int B, int diag, const float* y, const float* var,
                            const double* m0, const double* S0, const double* A, const double* C, const double* Q,
                            const double* s, double* Sw) {
  const DenseModelPtrs M{m0, S0, A, C, Q};
  switch (D) {
    case 1: em_sim<1>(T, K, O, B, y, var, M, s, diag != 0, Sw); return 0;
    case 2: em_sim<2>(T, K, O, B, y, var, M, s, diag != 0, Sw); return 0;
    case 3: em_sim<3>(T, K, O, B, y, var, M, s, diag != 0, Sw); return 0;
    default: return -3;
  }
}
