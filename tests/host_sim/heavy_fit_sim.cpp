// Host-side simulator of eks_smooth_heavy_fit's statistic and step.  TEST INFRASTRUCTURE ONLY: a stand-alone program
// that calls the lane bodies the gfx950 kernels call (eks_amd/csrc/eks_smooth_heavy_fit_lane.hpp) from plain loops, in
// the kernel's organisation - a lane per (sub-slab, keypoint), the sub-slab sums of a slab added in order into
// part[slab][k], then the last block's rounds of slab sums and the step - on heap buffers of exactly the sizes the
// kernels are given: contributions [T][K][nd], scales [T][K], partial sums [slabs][K].  It is not a fallback and is
// never loaded into Python: tests/test_heavy_fit_cpu.py builds it (plain, and with -fsanitize=address,undefined) and
// runs it.  The self-check, over T - 1 in {1, R-1, R, R+1, 3R+1}, K in {1, 3, 65}, nd in {1, 3} floats and one double:
//   - S_k (through the step, s_new = s S_k / n under wide bounds) against a long-double sum of the same terms;
//   - row 0 of both planes is never read (it holds NaN);
//   - keypoints [k0, k1) alone, repacked, give the bits of the full run;
//   - a NaN-poisoned keypoint keeps its s with 0 change, every other keypoint the bits of the healthy run;
//   - S_k = 0 lands on the lower bound, a huge S_k on the upper, and a start at a bound stays inside.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "eks_smooth_heavy_fit_lane.hpp"

using namespace eks;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

template <typename C>
struct Planes {
  int T, K, nd;
  std::vector<C> contrib;      // exactly [T][K][nd]
  std::vector<float> scales;   // exactly [T][K]
};

template <typename C>
static Planes<C> make(int T, int K, int nd) {
  Planes<C> p{T, K, nd, std::vector<C>((size_t)T * K * nd), std::vector<float>((size_t)T * K)};
  for (size_t i = 0; i < p.contrib.size(); ++i) p.contrib[i] = (C)(uniform() < 0.02 ? 400.0 * uniform() : 2.0 * uniform());
  for (size_t i = 0; i < p.scales.size(); ++i) p.scales[i] = (float)std::exp(3.0 * (uniform() - 0.5));
  for (int k = 0; k < K; ++k) {   // row 0 of either plane is never read
    p.scales[k] = NAN;
    for (int d = 0; d < nd; ++d) p.contrib[(size_t)k * nd + d] = (C)NAN;
  }
  return p;
}

template <typename C>
static Planes<C> subset(const Planes<C>& p, int k0, int k1) {
  const int K2 = k1 - k0;
  Planes<C> q{p.T, K2, p.nd, std::vector<C>((size_t)p.T * K2 * p.nd), std::vector<float>((size_t)p.T * K2)};
  for (int t = 0; t < p.T; ++t)
    for (int k = 0; k < K2; ++k) {
      q.scales[(size_t)t * K2 + k] = p.scales[(size_t)t * p.K + k0 + k];
      for (int d = 0; d < p.nd; ++d)
        q.contrib[((size_t)t * K2 + k) * p.nd + d] = p.contrib[((size_t)t * p.K + k0 + k) * p.nd + d];
    }
  return q;
}

struct Out {
  std::vector<double> s, S;
  std::vector<float> dlog;
};

// heavy_fit_kernel's lanes (whatever its keypoint tile, a keypoint's order is this one), then its last block's
static int round_mismatches = 0;

template <typename C>
static Out run(const Planes<C>& p, int D, const std::vector<double>& s0, double lo, double hi, int round = 64,
               int KT = 16) {
  const int n_slabs = heavy_fit_slabs(p.T);
  std::vector<double> part((size_t)n_slabs * p.K);   // exactly [slabs][K]
  for (int slab = 0; slab < n_slabs; ++slab)
    for (int k = 0; k < p.K; ++k) {
      double subs[kFitSubs];
      for (int sub = 0; sub < kFitSubs; ++sub)
        subs[sub] = heavy_fit_sub_lane<C>(p.contrib.data(), p.nd, p.scales.data(), p.K, p.T, k,
                                          1 + (long)slab * kFitSlab + (long)sub * kFitSub);
      part[(size_t)slab * p.K + k] = heavy_fit_slab_lane(subs, 1);
    }
  // the tile's last block: rounds of `round` slab sums gathered in a buffer (the kernel's LDS, KT keypoints wide), added
  // by heavy_fit_sum_lane, then the step - and heavy_fit_step_lane straight from part[] must give the same bits
  Out o{s0, std::vector<double>(p.K, 0.0), std::vector<float>(p.K, -1.0f)};
  std::vector<double> s_direct(s0);
  std::vector<float> dlog_direct(p.K, -1.0f);
  const double n = (double)D * (p.T - 1);
  for (int k = 0; k < p.K; ++k) {
    std::vector<double> buf((size_t)round * KT, NAN);
    const int kl = k % KT;
    double S = 0.0;
    for (int j0 = 0; j0 < n_slabs; j0 += round) {
      const int m = n_slabs - j0 < round ? n_slabs - j0 : round;
      for (int i = 0; i < m; ++i) buf[(size_t)i * KT + kl] = part[(size_t)(j0 + i) * p.K + k];
      S = heavy_fit_sum_lane(S, buf.data() + kl, m, KT);
    }
    o.S[k] = S;
    heavy_fit_apply_lane(S, k, n, lo, hi, o.s.data(), o.dlog.data());
    heavy_fit_step_lane(part.data(), n_slabs, p.K, k, n, lo, hi, s_direct.data(), dlog_direct.data());
    if (std::memcmp(&o.s[k], &s_direct[k], sizeof(double)) != 0 || o.dlog[k] != dlog_direct[k]) ++round_mismatches;
  }
  return o;
}

static int fails = 0;
#define CHECK(cond, ...)                                 \
  do {                                                   \
    if (!(cond)) {                                       \
      ++fails;                                           \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);   \
      std::printf(__VA_ARGS__);                          \
      std::printf("\n");                                 \
    }                                                    \
  } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

template <typename C>
static void check_shape(int T, int K, int nd, const char* type) {
  const int D = nd > 1 ? nd : 2;
  const Planes<C> p = make<C>(T, K, nd);
  std::vector<double> s0(K);
  for (int k = 0; k < K; ++k) s0[k] = std::exp(4.0 * (uniform() - 0.5));
  const Out full = run(p, D, s0, -700.0, 700.0);
  const double n = (double)D * (T - 1);
  for (int k = 0; k < K; ++k) {
    long double want = 0.0L;
    for (int t = 1; t < T; ++t) {
      const size_t o = (size_t)t * K + k;
      long double delta = 0.0L;
      for (int d = 0; d < nd; ++d) delta += (long double)p.contrib[o * nd + d];
      want += delta / (long double)p.scales[o];
    }
    const double rel = (double)fabsl(((long double)full.S[k] - want) / want);
    CHECK(rel <= 1e-13, "%s T=%d K=%d nd=%d k=%d: S %.17g against %.17Lg (rel %.3g)", type, T, K, nd, k, full.S[k], want, rel);
    const double s_want = (double)((long double)s0[k] * want / n);
    CHECK(std::fabs(full.s[k] / s_want - 1.0) <= 1e-13, "%s T=%d K=%d nd=%d k=%d: s %.17g against %.17g", type, T, K, nd,
          k, full.s[k], s_want);
    CHECK(std::fabs((double)full.dlog[k] - std::fabs(std::log(s_want / s0[k]))) <= 1e-6 * (1.0 + full.dlog[k]),
          "%s T=%d K=%d k=%d: dlog %.9g", type, T, K, k, (double)full.dlog[k]);
  }
  // the compile-time nd forms the kernels instantiate: the same bits as the run-time one, full and cut sub-slabs alike
  for (long t0 = 1; t0 < T; t0 += kFitSub) {
    const int k = (int)(t0 % K);
    const double a = heavy_fit_sub_lane<C>(p.contrib.data(), nd, p.scales.data(), K, T, k, t0);
    const double b = nd == 1 ? heavy_fit_sub_lane<C, 1>(p.contrib.data(), nd, p.scales.data(), K, T, k, t0)
                             : heavy_fit_sub_lane<C, 3>(p.contrib.data(), nd, p.scales.data(), K, T, k, t0);
    CHECK(same_bits(a, b), "%s T=%d K=%d nd=%d: the compile-time form differs at row %ld", type, T, K, nd, t0);
  }
  const Out again = run(p, D, s0, -700.0, 700.0, 2, 4);   // rounds of two slabs: T - 1 = 3 R + 1 takes two rounds
  for (int k = 0; k < K; ++k) CHECK(same_bits(again.s[k], full.s[k]), "second run differs, k=%d", k);
  if (K >= 3) {   // a subset of the keypoints, repacked
    const int k0 = 1, k1 = K > 40 ? 40 : K;
    const Out sub = run(subset(p, k0, k1), D, std::vector<double>(s0.begin() + k0, s0.begin() + k1), -700.0, 700.0);
    for (int k = k0; k < k1; ++k)
      CHECK(same_bits(sub.s[k - k0], full.s[k]) && sub.dlog[k - k0] == full.dlog[k],
            "%s T=%d K=%d nd=%d: keypoint %d of the subset differs", type, T, K, nd, k);
    // keypoint 1 poisoned at one frame
    Planes<C> bad = p;
    bad.contrib[((size_t)(T - 1) * K + 1) * nd] = (C)NAN;
    const Out pois = run(bad, D, s0, -700.0, 700.0);
    for (int k = 0; k < K; ++k) {
      if (k == 1) CHECK(same_bits(pois.s[k], s0[k]) && pois.dlog[k] == 0.0f, "poisoned keypoint moved");
      else CHECK(same_bits(pois.s[k], full.s[k]) && pois.dlog[k] == full.dlog[k], "keypoint %d beside a poisoned one", k);
    }
    bad = p;
    bad.scales[(size_t)(T - 1) * K + 1] = 0.0f;   // u = +inf
    const Out inf = run(bad, D, s0, -700.0, 700.0);
    CHECK(same_bits(inf.s[1], s0[1]) && inf.dlog[1] == 0.0f, "keypoint with an infinite S moved");
  }
  // the bounds
  const Out clipped = run(p, D, s0, -0.5, 0.25);
  for (int k = 0; k < K; ++k) {
    const double l = std::log(clipped.s[k]);
    CHECK(l >= -0.5 - 1e-15 && l <= 0.25 + 1e-15, "log s %.17g outside the bounds", l);
    const double unclipped = std::log(full.s[k]);
    if (unclipped > 0.25) CHECK(same_bits(clipped.s[k], std::exp(0.25)), "not on the upper bound");
    if (unclipped < -0.5) CHECK(same_bits(clipped.s[k], std::exp(-0.5)), "not on the lower bound");
  }
  Planes<C> zero = p;
  for (size_t i = 0; i < zero.contrib.size(); ++i) zero.contrib[i] = (C)0;
  const Out low = run(zero, D, s0, -8.0, 8.0);
  for (int k = 0; k < K; ++k) CHECK(same_bits(low.s[k], std::exp(-8.0)), "S = 0 is not the lower bound");
  std::vector<double> bad_s(s0);
  bad_s[0] = 0.0;
  const Out kept = run(p, D, bad_s, -8.0, 8.0);
  CHECK(kept.s[0] == 0.0 && kept.dlog[0] == 0.0f, "s = 0 was stepped");
}

int main() {
  const int R = kFitSlab;
  const int rows[] = {1, R - 1, R, R + 1, 3 * R + 1};
  const int Ks[] = {1, 3, 65};
  for (int r : rows)
    for (int K : Ks) {
      check_shape<float>(r + 1, K, 1, "float");
      check_shape<float>(r + 1, K, 3, "float");
      check_shape<double>(r + 1, K, 1, "double");
    }
  CHECK(heavy_fit_slabs(1) == 0 && heavy_fit_slabs(2) == 1 && heavy_fit_slabs(R + 1) == 1 && heavy_fit_slabs(R + 2) == 2,
        "slab count");
  CHECK(round_mismatches == 0, "%d keypoints: the rounds of slab sums and heavy_fit_step_lane disagree", round_mismatches);
  if (fails) {
    std::printf("heavy_fit_sim: %d checks failed\n", fails);
    return 1;
  }
  std::printf("heavy_fit_sim: ok\n");
  return 0;
}
