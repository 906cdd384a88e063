// Host-side simulator of ONE sweep of eks_ekf_affine_sweep (eks_amd/csrc/eks_dense.hip).  TEST
// INFRASTRUCTURE ONLY: the lane bodies come from the same header the gfx950 kernels include
// (eks_amd/csrc/eks_dense_lane.hpp, AffineObs), driven from plain loops - chunk elements, the scan as
// sequential applies / pull-backs, then the extended replay of every chunk that rewrites xlin - so that
// the tabulated fixed point can be compared with the sequential extended filter on a CPU-only box.  The
// Python side rebuilds the tables between sweeps.  Nothing under eks_amd/ loads it.
#include <algorithm>
#include <vector>

#include "eks_dense_lane.hpp"

using namespace eks;

template <int D>
static double affine_sweep(int T, int K, int Kd, int O, int B, const float* y, const float* var,
                           const double* rconst, const DenseModelPtrs& M, const double* s, const double* jac,
                           const double* off, double* xlin, float* ms, float* Vs, double* nll) {
  constexpr int REC = D + D * D;
  const int nc = (T + B - 1) / B;
  const AffineObs<D> obs{y, ObsNoise{var, rconst}, K, Kd, O, jac, off};
  std::vector<double> filt((size_t)B * REC);
  double worst = 0.0;
  for (int k = 0; k < K; ++k) {
    Mat<double, D> F, sQ;
    bool fid;
    load_dynamics<double, D>(M, k, s[k], F, sQ, fid);
    std::vector<DElem<double, D>> el(nc);
    for (int j = 0; j < nc; ++j) el[j] = dense_smooth_element_obs<D>(obs, k, j * B, std::min(B, T - j * B), F, sQ, fid);
    std::vector<Vec<double, D>> pm(nc), se(nc);
    std::vector<Mat<double, D>> pP(nc), sJ(nc);
    Vec<double, D> m;
    Mat<double, D> P;
    load_prior<D>(M, k, m, P);
    double xl[D];
    for (int a = 0; a < D; ++a) xl[a] = m.a[a];
    belief_update_obs<D>(obs, k, 0, xl, m, P);
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
    double ll_k = 0.0;
    for (int j = 0; j < nc; ++j) {
      if (j == 0) load_prior<D>(M, k, pm[0], pP[0]);
      double ll = 0.0, ch = 0.0;
      dense_replay_chunk_obs<D, true, AffineObs<D>>(obs, K, k, j * B, std::min(B, T - j * B), F, sQ, fid, pm[j],
                                                    pP[j], se[j], sJ[j], filt.data(), ms, Vs, false,
                                                    xlin + ((size_t)k * T + (size_t)j * B) * D, &ll, &ch);
      ll_k += ll;
      worst = std::max(worst, ch);
    }
    if (nll) nll[k] = -ll_k;
  }
  return worst;
}

// One sweep over K chains (chain k reads keypoint k % Kd); tables jac [T][K][O][D], off [T][K][O];
// xlin [K][T][D] in/out; ms [T][K][D], Vs [T][K][D][D] or NULL (filter only).  Returns the largest
// relative change of a linearisation point, or -1 for an unsupported D.
extern "C" double sim_affine_sweep(int T, int K, int Kd, int D, int O, int B, const float* y, const float* var,
                                   const double* rconst, const double* m0, const double* S0, const double* A,
                                   const double* Q, const double* s, const double* jac, const double* off,
                                   double* xlin, float* ms, float* Vs, double* nll) {
  const DenseModelPtrs M{m0, S0, A, nullptr, Q};
  switch (D) {
    case 1: return affine_sweep<1>(T, K, Kd, O, B, y, var, rconst, M, s, jac, off, xlin, ms, Vs, nll);
    case 2: return affine_sweep<2>(T, K, Kd, O, B, y, var, rconst, M, s, jac, off, xlin, ms, Vs, nll);
    case 3: return affine_sweep<3>(T, K, Kd, O, B, y, var, rconst, M, s, jac, off, xlin, ms, Vs, nll);
    case 6: return affine_sweep<6>(T, K, Kd, O, B, y, var, rconst, M, s, jac, off, xlin, ms, Vs, nll);
    default: return -1.0;
  }
}
