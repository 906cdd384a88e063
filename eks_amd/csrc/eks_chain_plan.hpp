// Geometry, lane mapping, workspace layout and forward pass shared by the scalar-chain entry points that summarise
// every (chain, chunk of frames) into a filter element, run the grouped Kalman scan over SampleWs planes and replay over
// the same (chain, chunk) lanes: eks_sample (eks_sample.hip), eks_smooth_increments (eks_increments.hip), eks_em_stats
// (eks_em.hip), eks_innovations (eks_innov.hip) and eks_smooth_tv (eks_smooth_tv.hip).  The host part is plain C++:
// tests/host_sim/ carves its buffers with the same chain_layout.  Kernels and launches: eks_chain.hip.
#pragma once
#include <utility>

#include "eks_sample_lane.hpp"

namespace eks {

constexpr int kChainChunk = 32;   // frames per lane: the replays hold 2 or 3 values per frame of the chunk in VGPRs

// nc chunks of B frames cut into ng scan groups of gs chunks (gs_override <= 0: ceil(sqrt(nc)))
struct ChainGeometry {
  int nc, gs, ng;
};
inline ChainGeometry chain_geometry(int T, int B, int gs_override = 0) {
  ChainGeometry g;
  g.nc = (T + B - 1) / B;
  g.gs = gs_override > 0 ? gs_override : 1;
  while (gs_override <= 0 && g.gs * g.gs < g.nc) ++g.gs;
  g.ng = (g.nc + g.gs - 1) / g.gs;
  return g;
}

// lanes along chains; N < 64 packs 64 / NT chunks of NT = pow2ceil(N) chains into a wave
struct ChainMap {
  int nt_log2;   // log2 of chains per wave row (min(64, pow2ceil(N)))
  int ntile;     // ceil(N / NT)
};
inline ChainMap chain_map(int N) {
  ChainMap L;
  L.nt_log2 = 0;
  while ((1 << L.nt_log2) < N && L.nt_log2 < 6) ++L.nt_log2;
  L.ntile = (N + (1 << L.nt_log2) - 1) >> L.nt_log2;
  return L;
}
// 256-thread workgroups that give every (chain, chunk) a lane
inline unsigned chain_blocks(const ChainMap& L, int nc) {
  const int cpw = 64 >> L.nt_log2;                               // chunks per wave
  const long waves = (long)L.ntile * ((nc + cpw - 1) / cpw);
  return (unsigned)((waves + 3) / 4);
}

inline size_t chain_plane(size_t rows, int N, size_t elem, size_t align) {
  return (rows * (size_t)N * elem + align - 1) / align * align;
}

// THE layout of the family's workspace: W's planes of [rows][N] floats, each on a multiple of `align` bytes, n_draws > 0
// adding the draw scans' gam / beta / hG / hB, and with `part` a [nc][N] float64 plane of chunk partials behind them.
// Returns the bytes taken.  base == nullptr: the size alone (a size query is this call); else W and *part point into
// base.  align = 256 in the library; the host simulators pack tighter so that a sanitizer sees every plane's end.
inline size_t chain_layout(int N, const ChainGeometry& g, int n_draws, bool with_part, size_t align, char* base,
                           SampleWs* W = nullptr, double** part = nullptr) {
  size_t at = 0;
  auto take = [&](size_t rows, size_t elem = sizeof(float)) {
    char* p = base ? base + at : nullptr;
    at += chain_plane(rows, N, elem, align);
    return reinterpret_cast<float*>(p);
  };
  const size_t nc = (size_t)g.nc, ng = (size_t)g.ng, nd = (size_t)n_draws;
  SampleWs w{};
  w.N = N; w.nc = g.nc; w.ng = g.ng; w.gs = g.gs; w.n_draws = n_draws;
  w.eA = take(nc); w.eb = take(nc); w.eC = take(nc); w.eEta = take(nc); w.eJ = take(nc);
  w.pm = take(nc); w.pP = take(nc); w.sEta = take(nc); w.sJ = take(nc);
  if (n_draws > 0) { w.gam = take(nc); w.beta = take(nd * nc); }
  w.gA = take(ng); w.gb = take(ng); w.gC = take(ng); w.gEta = take(ng); w.gJ = take(ng);
  w.gm = take(ng); w.gP = take(ng); w.gsEta = take(ng); w.gsJ = take(ng);
  if (n_draws > 0) { w.hG = take(ng); w.hB = take(nd * ng); }
  double* pt = with_part ? reinterpret_cast<double*>(take(nc, sizeof(double))) : nullptr;
  if (W) *W = w;
  if (part) *part = pt;
  return at;
}

// one call's planes on its workspace, the lane mapping and the grid of the (chain, chunk) launches
struct ChainPlan {
  SampleWs W;
  ChainMap L;
  unsigned blocks;   // of 256 threads
  double* part;      // [nc][N] float64 chunk partials, or null
};
inline size_t chain_workspace_bytes(int T, int N, int n_draws, bool with_part) {
  return chain_layout(N, chain_geometry(T, kChainChunk), n_draws, with_part, 256, nullptr);
}
inline ChainPlan chain_plan(int T, int N, int n_draws, bool with_part, void* ws) {
  ChainPlan P;
  chain_layout(N, chain_geometry(T, kChainChunk), n_draws, with_part, 256, static_cast<char*>(ws), &P.W, &P.part);
  P.L = chain_map(N);
  P.blocks = chain_blocks(P.L, P.W.nc);
  return P;
}

// f(std::integral_constant<int, R>{}) for R == vs_row, PointerStore's VS_ROW as a compile-time constant: 0
// (EKS_FLAG_VS_DIAG) or the state dimension 1 .. 8; any other value calls nothing
template <typename F, int... R>
inline void with_vs_row(int vs_row, F&& f, std::integer_sequence<int, R...>) {
  (void)((vs_row == R && (f(std::integral_constant<int, R>{}), true)) || ...);
}
template <typename F>
inline void with_vs_row(int vs_row, F&& f) {
  with_vs_row(vs_row, f, std::make_integer_sequence<int, 9>{});
}

}  // namespace eks

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace eks {

__device__ __forceinline__ bool chain_coords(const ChainMap& L, int N, int nc, int& n, int& j) {
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int tile = wave % L.ntile, cg = wave / L.ntile;
  const int nt = 1 << L.nt_log2;
  n = tile * nt + (lane & (nt - 1));
  j = cg * (64 >> L.nt_log2) + (lane >> L.nt_log2);
  return n < N && j < nc;
}

// eks_chain.hip.  chain_forward: summarize (sample_summarize_lane: reads c.y, c.var) + the scan; chain_scan: the three
// scan launches over the chunk elements in P.W, for a caller with a summarize of its own.  The scopes are the names
// the profile reports (string literals).
int chain_forward(const ChainPlan& P, const DiagModel& M, const SampleCall& c, bool unit, const char* summarize_scope,
                  const char* scan_scope, hipStream_t st);
int chain_scan(const ChainPlan& P, const DiagModel& M, const char* scan_scope, hipStream_t st);

}  // namespace eks
#endif
