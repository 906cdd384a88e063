// Host-side simulator of eks_smooth_robust's arithmetic on scalar chains.  TEST INFRASTRUCTURE ONLY: a stand-alone
// program that calls the lane bodies the gfx950 kernels call (eks_amd/csrc/eks_smooth_student_lane.hpp) from plain loops,
// in the kernels' order of passes, on a workspace carved by chain_layout from a heap buffer of exactly the reported
// size.  It is not a fallback and is never loaded into Python: tests/test_robust_cpu.py builds it (plain, and with
// -fsanitize=address,undefined) and runs it.
//   robust_sim                 the self-check: chunk lengths 4 .. 32, T = 1 .. 1000, UNIT and a = 0.98, c = 1.3; with
//                              n_iters = 1 every lane's element, the scan's planes (the carried beliefs) and the outputs
//                              are bit for bit those of the smooth_tv bodies at w = 1; after 2 and 8 passes everything
//                              is finite, variances positive, 0 < lam <= (nu + 1) / nu, and 3 + 6 passes continued
//                              through the weights give the bits of 8.
//   robust_sim IN OUT          one problem from file IN (layout below), its ms, Vs, lam [T][N] and change [K] to OUT.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "chain_sim.hpp"
#include "eks_smooth_student_lane.hpp"

using namespace eks;

struct Problem {
  int T, N, D, B, unit, n_iters, weights_in;
  double nu;
  std::vector<float> y, var, lam;
  std::vector<double> m0, S0, A, C, Q, s;
};

struct Result {
  std::vector<float> ms, Vs, lam, change;
  std::vector<char> planes;   // the workspace after the FIRST pass's summarize and scan
};

template <int B, bool UNIT, bool HAS_LAM>
static void pass(const SampleWs& W, const DiagModel& M, const StudentCall& c, bool last, Result* keep) {
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < W.N; ++n) student_summarize_lane<B, UNIT, HAS_LAM, kObsInPlace, false>(W, M, c, n, j);
  chain_sim_scan(W, M);
  if (keep) keep->planes.assign(reinterpret_cast<const char*>(W.eA), reinterpret_cast<const char*>(W.eA) + keep->planes.size());
  for (int j = 0; j < W.nc; ++j)
    for (int n = 0; n < W.N; ++n) {
      if (last) student_last_lane<B, UNIT, 0, HAS_LAM, kObsInPlace, false>(W, M, c, n, j);
      else student_replay_lane<B, UNIT, HAS_LAM, kObsInPlace, false>(W, M, c, n, j);
    }
}

template <int B, bool UNIT>
static Result run(const Problem& p) {
  const int K = p.N / p.D;
  const DiagModel M{p.m0.data(), p.S0.data(), p.A.data(), p.C.data(), p.Q.data(), p.s.data(), p.D};
  ChainSimWs S(p.T, p.N, B, 0, 0, false);
  const size_t TN = (size_t)p.T * p.N;
  Result r;
  r.ms.assign(TN, NAN); r.Vs.assign(TN, NAN);
  r.lam = p.weights_in ? p.lam : std::vector<float>(TN, NAN);   // exactly [T][N]
  r.change.assign(K, 0.0f);
  r.planes.resize(S.buf.size());
  const std::vector<float> ones(p.T, 1.0f);   // exactly [T]
  for (int it = 0; it < p.n_iters; ++it) {
    const bool last = it == p.n_iters - 1;
    const StudentCall c{p.y.data(), p.var.data(), r.lam.data(), ones.data(), nullptr,
                        it == p.n_iters - 2 ? r.change.data() : nullptr, r.ms.data(), r.Vs.data(), p.T, K, (float)p.nu,
                        (float)(p.nu + 1.0), (float)((p.nu + 1.0) / p.nu), p.N, 1};
    if (it > 0 || p.weights_in) pass<B, UNIT, true>(S.W, M, c, last, it == 0 ? &r : nullptr);
    else pass<B, UNIT, false>(S.W, M, c, last, &r);
  }
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

// eks_smooth_tv's bodies at w = 1 on the same problem: the planes after summarize + scan, ms and Vs
template <int B, bool UNIT>
static Result run_tv(const Problem& p) {
  const int K = p.N / p.D;
  const DiagModel M{p.m0.data(), p.S0.data(), p.A.data(), p.C.data(), p.Q.data(), p.s.data(), p.D};
  ChainSimWs S(p.T, p.N, B, 0, 0, false);
  const size_t TN = (size_t)p.T * p.N;
  Result r;
  r.ms.assign(TN, NAN); r.Vs.assign(TN, NAN);
  std::vector<float> w(p.T, 1.0f);
  const SmoothTvCall c{p.y.data(), p.var.data(), w.data(), r.ms.data(), r.Vs.data(), p.T, K, 0};
  for (int j = 0; j < S.W.nc; ++j)
    for (int n = 0; n < p.N; ++n) smooth_tv_summarize_lane<B, UNIT>(S.W, M, c, n, j);
  chain_sim_scan(S.W, M);
  r.planes = S.buf;
  for (int j = 0; j < S.W.nc; ++j)
    for (int n = 0; n < p.N; ++n) smooth_tv_replay_lane<B, UNIT, 0>(S.W, M, c, n, j);
  return r;
}

static Result dispatch_tv(const Problem& p) {
#define RUN(BB) \
  case BB: return p.unit ? run_tv<BB, true>(p) : run_tv<BB, false>(p);
  switch (p.B) {
    RUN(4)
    RUN(8)
    RUN(16)
    default: return p.unit ? run_tv<32, true>(p) : run_tv<32, false>(p);
  }
#undef RUN
}

static bool same(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

static Problem synthetic(int T, int B, int unit) {
  Problem p;
  const int K = 3, D = 2, N = K * D;
  p.T = T; p.N = N; p.D = D; p.B = B; p.unit = unit; p.n_iters = 1; p.weights_in = 0; p.nu = 4.0;
  p.y.resize((size_t)T * N); p.var.resize((size_t)T * N);
  for (size_t i = 0; i < p.y.size(); ++i) {
    p.y[i] = 100.0f + (float)((i * 37) % 101) * 0.1f + (i % 53 == 7 ? 40.0f : 0.0f);   // ~2 % displaced
    p.var[i] = 0.5f + (float)((i * 13) % 7);
  }
  p.m0.assign(N, 100.0); p.S0.assign(K * D * D, 0.0); p.A.assign(K * D * D, 0.0); p.C.assign(K * D * D, 0.0);
  p.Q.assign(K * D * D, 0.0); p.s.assign(K, 2.0);
  for (int k = 0; k < K; ++k)
    for (int d = 0; d < D; ++d) {
      const size_t dd = (size_t)k * D * D + d * (D + 1);
      p.S0[dd] = 3.0; p.Q[dd] = 1.0;
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
        Result one, tv = dispatch_tv(p);
        dispatch(p, one);
        int b = 0;
        b += one.planes != tv.planes || !same(one.ms, tv.ms) || !same(one.Vs, tv.Vs);
        for (float l : one.lam) b += l != 1.0f;
        for (float c : one.change) b += c != 0.0f;
        Result r2, r8, r3, r36;
        p.n_iters = 2; dispatch(p, r2);
        p.n_iters = 8; dispatch(p, r8);
        p.n_iters = 3; dispatch(p, r3);
        p.n_iters = 6; p.weights_in = 1; p.lam = r3.lam; dispatch(p, r36);
        b += !same(r36.ms, r8.ms) || !same(r36.Vs, r8.Vs) || !same(r36.lam, r8.lam) || !same(r36.change, r8.change);
        for (const Result* r : {&r2, &r8}) {
          for (size_t i = 0; i < r->ms.size(); ++i)
            b += !std::isfinite(r->ms[i]) || !(std::isfinite(r->Vs[i]) && r->Vs[i] > 0.0f) ||
                 !(r->lam[i] > 0.0f && r->lam[i] <= 1.25f);
          for (float c : r->change) b += !(c >= 0.0f && c <= 1.25f);
        }
        if (b) std::printf("robust_sim: B=%d T=%d unit=%d: %d problems\n", B, T, unit, b);
        bad += b;
      }
  std::printf("robust_sim: %s\n", bad ? "FAILED" : "ok");
  return bad != 0;
}

// IN: int32 {T, N, D, B, unit, n_iters, weights_in}, float64 nu, float32 y, var, lam [T][N] (lam only with weights_in),
// float64 m0 [N], S0, A, C, Q [K][D][D], s [K].  OUT: float32 ms, Vs, lam [T][N], change [K].
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
    p.T = h[0]; p.N = h[1]; p.D = h[2]; p.B = h[3]; p.unit = h[4]; p.n_iters = h[5]; p.weights_in = h[6];
    ok = p.T > 0 && p.N > 0 && p.D > 0 && p.N % p.D == 0 && p.n_iters > 0;
  }
  if (ok) {
    const size_t TN = (size_t)p.T * p.N, K = p.N / p.D, DD = K * p.D * p.D;
    ok = rd(f, p.y, TN) && rd(f, p.var, TN) && (!p.weights_in || rd(f, p.lam, TN)) && rd(f, p.m0, (size_t)p.N) &&
         rd(f, p.S0, DD) && rd(f, p.A, DD) && rd(f, p.C, DD) && rd(f, p.Q, DD) && rd(f, p.s, K);
  }
  std::fclose(f);
  Result r;
  if (!ok || !dispatch(p, r)) return 2;
  std::FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 2;
  for (const std::vector<float>* v : {&r.ms, &r.Vs, &r.lam, &r.change}) std::fwrite(v->data(), sizeof(float), v->size(), g);
  return std::fclose(g) != 0;
}
