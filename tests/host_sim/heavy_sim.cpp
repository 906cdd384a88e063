// Host-side simulator of eks_smooth_heavy's arithmetic on scalar chains.  TEST INFRASTRUCTURE ONLY: a stand-alone
// program that calls the lane bodies the gfx950 kernels call (eks_amd/csrc/eks_smooth_student_lane.hpp) from plain loops,
// in the kernels' order of launches, on a workspace carved by chain_layout from a heap buffer of exactly the reported
// size, a weight plane of exactly [T][N], a scale plane of exactly [T][K] and a contribution plane of exactly [T][N]
// floats.  It is not a fallback and is never loaded into Python: tests/test_heavy_cpu.py builds it (plain, and with
// -fsanitize=address,undefined) and runs it.
//   heavy_sim                  the self-check: chunk lengths 4 .. 32, T = 1 .. 1000, UNIT and a = 0.98, c = 1.3; with
//                              n_iters = 1 weights and scales are 1, change 0 and the outputs bit for bit those of the
//                              smooth_tv bodies at w = 1; a middle pass rewrites rows 1 .. T-1 of a poisoned
//                              contribution plane; after 2 and 8 passes everything is finite and in range, and 3 + 6
//                              passes continued through both planes give the bits of 8.
//   heavy_sim IN OUT           one problem from file IN (layout below); ms, Vs, lam [T][N], w [T][K], change [2][K] to OUT.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "chain_sim.hpp"
#include "eks_smooth_student_lane.hpp"

using namespace eks;

struct Problem {
  int T, N, D, B, unit, n_iters, planes_in;
  double nu_obs, nu_proc;
  std::vector<float> y, var, lam, w;
  std::vector<double> m0, S0, A, C, Q, s;
};

struct Result {
  std::vector<float> ms, Vs, lam, w, change;
  int unwritten = 0;   // contributions of rows 1 .. T-1 a middle pass left poisoned
};

template <int B, bool UNIT, bool HAS_LAM>
static void pass(const SampleWs& W, const DiagModel& M, const StudentCall& c, int N, bool last) {
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < N; ++n) student_summarize_lane<B, UNIT, HAS_LAM, kObsInPlace, true>(W, M, c, n, j);
  chain_sim_scan(W, M);
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < N; ++n) {
      if (last) student_last_lane<B, UNIT, 0, HAS_LAM, kObsInPlace, true>(W, M, c, n, j);
      else student_replay_lane<B, UNIT, HAS_LAM, kObsInPlace, true>(W, M, c, n, j);
    }
}

template <int B, bool UNIT>
static Result run(const Problem& p) {
  const int K = p.N / p.D;
  const DiagModel M{p.m0.data(), p.S0.data(), p.A.data(), p.C.data(), p.Q.data(), p.s.data(), p.D};
  ChainSimWs S(p.T, p.N, B, 0, 0, false);
  const size_t TN = (size_t)p.T * p.N, TK = (size_t)p.T * K;
  Result r;
  r.ms.assign(TN, NAN); r.Vs.assign(TN, NAN);
  r.lam = (p.planes_in & 1) ? p.lam : std::vector<float>(TN, NAN);   // exactly [T][N]; not read before it is written
  r.w = (p.planes_in & 2) ? p.w : std::vector<float>(TK, 1.0f);     // exactly [T][K]
  for (int k = 0; k < K; ++k) r.w[k] = 1.0f;
  r.change.assign(2 * (size_t)K, 0.0f);
  std::vector<float> contrib(TN);                                   // exactly [T][N]
  for (int it = 0; it < p.n_iters; ++it) {
    const bool last = it == p.n_iters - 1, has_lam = it > 0 || (p.planes_in & 1);
    float* ch = it == p.n_iters - 2 ? r.change.data() : nullptr;
    const StudentCall c{p.y.data(), p.var.data(), r.lam.data(), r.w.data(), contrib.data(), ch, r.ms.data(), r.Vs.data(),
                        p.T, K, (float)p.nu_obs, (float)(p.nu_obs + 1.0), (float)((p.nu_obs + 1.0) / p.nu_obs), p.N, 1};
    if (!last) std::fill(contrib.begin(), contrib.end(), NAN);
    if (has_lam) pass<B, UNIT, true>(S.W, M, c, p.N, last);
    else pass<B, UNIT, false>(S.W, M, c, p.N, last);
    if (last) break;
    for (size_t i = p.N; i < TN; ++i) r.unwritten += contrib[i] != contrib[i];
    for (int t = 1; t < p.T; ++t)
      for (int k = 0; k < K; ++k) {
        const float cu = jumps_combine_lane<float>(contrib.data(), p.D, r.w.data(), K, t, k, p.nu_proc, p.nu_proc + p.D);
        if (ch) robust_change_max(ch + K + k, cu);
      }
  }
  return r;
}

// the smooth_tv bodies under a plane of ones: what n_iters = 1 has to reproduce bit for bit
template <int B, bool UNIT>
static Result run_tv(const Problem& p) {
  const int K = p.N / p.D;
  const DiagModel M{p.m0.data(), p.S0.data(), p.A.data(), p.C.data(), p.Q.data(), p.s.data(), p.D};
  ChainSimWs S(p.T, p.N, B, 0, 0, false);
  Result r;
  r.ms.assign((size_t)p.T * p.N, NAN); r.Vs.assign((size_t)p.T * p.N, NAN);
  std::vector<float> ones((size_t)p.T * K, 1.0f);
  const SmoothTvCall tv{p.y.data(), p.var.data(), ones.data(), r.ms.data(), r.Vs.data(), p.T, K, 1};
  for (int j = 0; j < S.W.nc; ++j)
    for (int n = 0; n < p.N; ++n) smooth_tv_summarize_lane<B, UNIT>(S.W, M, tv, n, j);
  chain_sim_scan(S.W, M);
  for (int j = 0; j < S.W.nc; ++j)
    for (int n = 0; n < p.N; ++n) smooth_tv_replay_lane<B, UNIT, 0>(S.W, M, tv, n, j);
  return r;
}

static bool dispatch(const Problem& p, Result& out, bool tv = false) {
#define RUN(BB) \
  case BB: out = tv ? (p.unit ? run_tv<BB, true>(p) : run_tv<BB, false>(p)) : (p.unit ? run<BB, true>(p) : run<BB, false>(p)); return true;
  switch (p.B) {
    RUN(4)
    RUN(8)
    RUN(16)
    RUN(32)
    default: return false;
  }
#undef RUN
}

static bool same(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

static Problem synthetic(int T, int B, int unit) {
  Problem p;
  const int K = 3, D = 2, N = K * D;
  p.T = T; p.N = N; p.D = D; p.B = B; p.unit = unit; p.n_iters = 1; p.planes_in = 0; p.nu_obs = 4.0; p.nu_proc = 4.0;
  p.y.resize((size_t)T * N); p.var.resize((size_t)T * N);
  for (size_t i = 0; i < p.y.size(); ++i) {
    const size_t t = i / N, k = (i % N) / D;
    p.y[i] = 100.0f + (float)((i * 37) % 101) * 0.02f + ((t + 11 * k) % 53 >= 7 ? 40.0f : 0.0f)   // steps of 40 px
             + ((t + 5 * k) % 29 == 3 ? -35.0f : 0.0f);                                             // displaced frames
    p.var[i] = 0.5f + (float)((i * 13) % 7) * 0.25f;
  }
  p.m0.assign(N, 100.0); p.S0.assign(K * D * D, 0.0); p.A.assign(K * D * D, 0.0); p.C.assign(K * D * D, 0.0);
  p.Q.assign(K * D * D, 0.0); p.s.assign(K, 0.05);
  for (int k = 0; k < K; ++k)
    for (int d = 0; d < D; ++d) {
      const size_t dd = (size_t)k * D * D + d * (D + 1);
      p.S0[dd] = 3.0; p.Q[dd] = (k == 2 && d == 1) ? 0.0 : 1.0;    // one chain with s q = 0
      p.A[dd] = unit ? 1.0 : 0.98;
      p.C[dd] = unit ? 1.0 : 1.3;
    }
  return p;
}

static int self_check() {
  int bad = 0;
  for (int B : {4, 8, 16, 32})
    for (int T : {1, 2, 3, 31, 32, 33, 129, 1000})
      for (int unit = 0; unit < 2; ++unit) {
        Problem p = synthetic(T, B, unit);
        Result one, tvr;
        dispatch(p, one);
        dispatch(p, tvr, true);
        int b = 0;
        for (float l : one.lam) b += l != 1.0f;
        for (float w : one.w) b += w != 1.0f;
        for (float c : one.change) b += c != 0.0f;
        b += !same(one.ms, tvr.ms) || !same(one.Vs, tvr.Vs);
        Result r2, r8, r3, r36;
        p.n_iters = 2; dispatch(p, r2);
        p.n_iters = 8; dispatch(p, r8);
        p.n_iters = 3; dispatch(p, r3);
        p.n_iters = 6; p.planes_in = 3; p.lam = r3.lam; p.w = r3.w; dispatch(p, r36);
        b += !same(r36.ms, r8.ms) || !same(r36.Vs, r8.Vs) || !same(r36.lam, r8.lam) || !same(r36.w, r8.w) ||
             !same(r36.change, r8.change);
        const float w_min = (float)(4.0 / 6.0) * 0.999999f;
        for (const Result* r : {&r2, &r8}) {
          b += r->unwritten;
          for (size_t i = 0; i < r->ms.size(); ++i)
            b += !std::isfinite(r->ms[i]) || !(std::isfinite(r->Vs[i]) && r->Vs[i] > 0.0f);
          for (float l : r->lam) b += !(l >= 1e-30f && l <= 1.25f);
          for (float w : r->w) b += !(w >= w_min && w <= 1.0001e30f);
          for (float c : r->change) b += !(c >= 0.0f && c <= 1.5f);
        }
        if (b) std::printf("heavy_sim: B=%d T=%d unit=%d: %d problems\n", B, T, unit, b);
        bad += b;
      }
  std::printf("heavy_sim: %s\n", bad ? "FAILED" : "ok");
  return bad != 0;
}

// IN: int32 {T, N, D, B, unit, n_iters, planes_in}, float64 nu_obs, nu_proc, float32 y, var [T][N], lam [T][N] (only with
// planes_in bit 0), w [T][K] (only with bit 1), float64 m0 [N], S0, A, C, Q [K][D][D], s [K].
// OUT: float32 ms, Vs, lam [T][N], w [T][K], change [2][K].
template <typename V>
static bool rd(std::FILE* f, std::vector<V>& v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(V), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_check();
  if (argc != 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  Problem p;
  int32_t h[7];
  double nu[2];
  bool ok = std::fread(h, sizeof(int32_t), 7, f) == 7 && std::fread(nu, sizeof(double), 2, f) == 2;
  if (ok) {
    p.T = h[0]; p.N = h[1]; p.D = h[2]; p.B = h[3]; p.unit = h[4]; p.n_iters = h[5]; p.planes_in = h[6];
    p.nu_obs = nu[0]; p.nu_proc = nu[1];
    ok = p.T > 0 && p.N > 0 && p.D > 0 && p.N % p.D == 0 && p.n_iters > 0;
  }
  if (ok) {
    const size_t TN = (size_t)p.T * p.N, K = p.N / p.D, DD = K * p.D * p.D;
    ok = rd(f, p.y, TN) && rd(f, p.var, TN) && (!(p.planes_in & 1) || rd(f, p.lam, TN)) &&
         (!(p.planes_in & 2) || rd(f, p.w, (size_t)p.T * K)) && rd(f, p.m0, (size_t)p.N) && rd(f, p.S0, DD) &&
         rd(f, p.A, DD) && rd(f, p.C, DD) && rd(f, p.Q, DD) && rd(f, p.s, K);
  }
  std::fclose(f);
  Result r;
  if (!ok || !dispatch(p, r)) return 2;
  std::FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 2;
  for (const std::vector<float>* v : {&r.ms, &r.Vs, &r.lam, &r.w, &r.change})
    std::fwrite(v->data(), sizeof(float), v->size(), g);
  return std::fclose(g) != 0;
}
