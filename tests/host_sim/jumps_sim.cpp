// Host-side simulator of eks_smooth_jumps' arithmetic on scalar chains.  TEST INFRASTRUCTURE ONLY: a stand-alone
// program that calls the lane bodies the gfx950 kernels call (eks_amd/csrc/eks_smooth_student_lane.hpp) from plain loops,
// in the kernels' order of launches, on a workspace carved by chain_layout from a heap buffer of exactly the reported
// size, a scale plane of exactly [T][K] and a contribution plane of exactly [T][N] floats.  It is not a fallback and is
// never loaded into Python: tests/test_jumps_cpu.py builds it (plain, and with -fsanitize=address,undefined) and runs it.
//   jumps_sim                  the self-check: chunk lengths 4 .. 32, T = 1 .. 1000, UNIT and a = 0.98, c = 1.3; with
//                              n_iters = 1 the scales are 1 and the outputs bit for bit those of the smooth_tv bodies at
//                              w = 1; a middle pass rewrites rows 1 .. T-1 of a poisoned contribution plane; after 2 and
//                              8 passes everything is finite, variances positive, nu / (nu + D) <= w <= 1e30, and 3 + 6
//                              passes continued through the scales give the bits of 8.
//   jumps_sim IN OUT           one problem from file IN (layout below), its ms, Vs [T][N], w [T][K], change [K] to OUT.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "chain_sim.hpp"
#include "eks_smooth_student_lane.hpp"

using namespace eks;

struct Problem {
  int T, N, D, B, unit, n_iters, scales_in;
  double nu;
  std::vector<float> y, var, w;
  std::vector<double> m0, S0, A, C, Q, s;
};

struct Result {
  std::vector<float> ms, Vs, w, change;
  int unwritten = 0;   // contributions of rows 1 .. T-1 a middle pass left poisoned
};

template <int B, bool UNIT>
static Result run(const Problem& p) {
  const int K = p.N / p.D;
  const DiagModel M{p.m0.data(), p.S0.data(), p.A.data(), p.C.data(), p.Q.data(), p.s.data(), p.D};
  ChainSimWs S(p.T, p.N, B, 0, 0, false);
  const size_t TN = (size_t)p.T * p.N, TK = (size_t)p.T * K;
  Result r;
  r.ms.assign(TN, NAN); r.Vs.assign(TN, NAN);
  r.w = p.scales_in ? p.w : std::vector<float>(TK, 1.0f);   // exactly [T][K]
  for (int k = 0; k < K; ++k) r.w[k] = 1.0f;
  r.change.assign(K, 0.0f);
  std::vector<float> contrib(TN);                           // exactly [T][N]
  const SmoothTvCall tv{p.y.data(), p.var.data(), r.w.data(), r.ms.data(), r.Vs.data(), p.T, K, 1};
  const StudentCall c{p.y.data(), p.var.data(), nullptr, r.w.data(), contrib.data(), nullptr, nullptr, nullptr, p.T, K,
                      0.0f, 0.0f, 0.0f, p.N, 1};
  for (int it = 0; it + 1 < p.n_iters; ++it) {
    for (int j = 0; j < S.W.nc; ++j)
      for (int n = 0; n < p.N; ++n) smooth_tv_summarize_lane<B, UNIT>(S.W, M, tv, n, j);
    chain_sim_scan(S.W, M);
    std::fill(contrib.begin(), contrib.end(), NAN);
    for (int j = 0; j < S.W.nc; ++j)
      for (int n = 0; n < p.N; ++n) student_replay_lane<B, UNIT, false, kObsFixed, true>(S.W, M, c, n, j);
    for (size_t i = p.N; i < TN; ++i) r.unwritten += contrib[i] != contrib[i];
    for (int t = 1; t < p.T; ++t)
      for (int k = 0; k < K; ++k) {
        const float ch = jumps_combine_lane<float>(contrib.data(), p.D, r.w.data(), K, t, k, p.nu, p.nu + p.D);
        if (it == p.n_iters - 2) robust_change_max(r.change.data() + k, ch);
      }
  }
  for (int j = 0; j < S.W.nc; ++j)
    for (int n = 0; n < p.N; ++n) smooth_tv_summarize_lane<B, UNIT>(S.W, M, tv, n, j);
  chain_sim_scan(S.W, M);
  for (int j = 0; j < S.W.nc; ++j)
    for (int n = 0; n < p.N; ++n) smooth_tv_replay_lane<B, UNIT, 0>(S.W, M, tv, n, j);
  return r;
}

static bool dispatch(const Problem& p, Result& out) {
#define RUN(BB) \
  case BB: out = p.unit ? run<BB, true>(p) : run<BB, false>(p); return true;
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
  p.T = T; p.N = N; p.D = D; p.B = B; p.unit = unit; p.n_iters = 1; p.scales_in = 0; p.nu = 4.0;
  p.y.resize((size_t)T * N); p.var.resize((size_t)T * N);
  for (size_t i = 0; i < p.y.size(); ++i) {
    const size_t t = i / N, k = (i % N) / D;
    p.y[i] = 100.0f + (float)((i * 37) % 101) * 0.02f + ((t + 11 * k) % 53 >= 7 ? 40.0f : 0.0f);   // steps of 40 px
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
        int b = 0;
        for (float w : one.w) b += w != 1.0f;
        for (float c : one.change) b += c != 0.0f;
        p.scales_in = 1; p.w.assign((size_t)T * 3, 1.0f); dispatch(p, tvr); p.scales_in = 0;   // one pass under given ones
        b += !same(one.ms, tvr.ms) || !same(one.Vs, tvr.Vs);
        Result r2, r8, r3, r36;
        p.n_iters = 2; dispatch(p, r2);
        p.n_iters = 8; dispatch(p, r8);
        p.n_iters = 3; dispatch(p, r3);
        p.n_iters = 6; p.scales_in = 1; p.w = r3.w; dispatch(p, r36);
        b += !same(r36.ms, r8.ms) || !same(r36.Vs, r8.Vs) || !same(r36.w, r8.w) || !same(r36.change, r8.change);
        const float w_min = (float)(4.0 / 6.0) * 0.999999f;
        for (const Result* r : {&r2, &r8}) {
          b += r->unwritten;
          for (size_t i = 0; i < r->ms.size(); ++i)
            b += !std::isfinite(r->ms[i]) || !(std::isfinite(r->Vs[i]) && r->Vs[i] > 0.0f);
          for (float w : r->w) b += !(w >= w_min && w <= 1.0001e30f);
          for (float c : r->change) b += !(c >= 0.0f && c <= 1.5f);
        }
        if (b) std::printf("jumps_sim: B=%d T=%d unit=%d: %d problems\n", B, T, unit, b);
        bad += b;
      }
  std::printf("jumps_sim: %s\n", bad ? "FAILED" : "ok");
  return bad != 0;
}

// IN: int32 {T, N, D, B, unit, n_iters, scales_in}, float64 nu, float32 y, var [T][N], w [T][K] (only with scales_in),
// float64 m0 [N], S0, A, C, Q [K][D][D], s [K].  OUT: float32 ms, Vs [T][N], w [T][K], change [K].
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
  bool ok = std::fread(h, sizeof(int32_t), 7, f) == 7 && std::fread(&p.nu, sizeof(double), 1, f) == 1;
  if (ok) {
    p.T = h[0]; p.N = h[1]; p.D = h[2]; p.B = h[3]; p.unit = h[4]; p.n_iters = h[5]; p.scales_in = h[6];
    ok = p.T > 0 && p.N > 0 && p.D > 0 && p.N % p.D == 0 && p.n_iters > 0;
  }
  if (ok) {
    const size_t TN = (size_t)p.T * p.N, K = p.N / p.D, DD = K * p.D * p.D;
    ok = rd(f, p.y, TN) && rd(f, p.var, TN) && (!p.scales_in || rd(f, p.w, (size_t)p.T * K)) && rd(f, p.m0, (size_t)p.N) &&
         rd(f, p.S0, DD) && rd(f, p.A, DD) && rd(f, p.C, DD) && rd(f, p.Q, DD) && rd(f, p.s, K);
  }
  std::fclose(f);
  Result r;
  if (!ok || !dispatch(p, r)) return 2;
  std::FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 2;
  for (const std::vector<float>* v : {&r.ms, &r.Vs, &r.w, &r.change}) std::fwrite(v->data(), sizeof(float), v->size(), g);
  return std::fclose(g) != 0;
}
