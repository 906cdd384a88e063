// Lane mapping and launch plan shared by the scalar-chain kernels of eks_em_stats (eks_em.hip), eks_innovations
// (eks_innov.hip) and eks_smooth_tv (eks_smooth_tv.hip): the first two run em_summarize and the grouped Kalman scan
// (diag_em_forward), the third a summarize of its own and the same scan (diag_em_plan, diag_em_scan); each then
// replays over the same (chain, chunk) lanes.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/eks_hip.h"
#include "eks_sample_lane.hpp"

namespace eks {

constexpr int kEmChunk = 32;   // frames per lane: 2 * B VGPRs hold (mf, Pf) of the chunk in E2

// lanes along chains; N < 64 packs 64 / NT chunks of NT = pow2ceil(N) chains into a wave (as eks_increments.hip)
struct EmMap {
  int nt_log2;
  int ntile;     // ceil(N / NT)
};

__device__ __forceinline__ bool em_coords(const EmMap& L, int N, int nc, int& n, int& j) {
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int tile = wave % L.ntile, cg = wave / L.ntile;
  const int nt = 1 << L.nt_log2;
  n = tile * nt + (lane & (nt - 1));
  j = cg * (64 >> L.nt_log2) + (lane >> L.nt_log2);
  return n < N && j < nc;
}

struct EmPlan {
  SampleWs W;     // planes on the caller's workspace
  EmMap L;
  dim3 grid;      // of 256-thread workgroups, one lane per (chain, chunk)
  double* part;   // [nc][N] float64 chunk partials behind the planes
};

void diag_em_plan(int T, int N, void* ws, EmPlan& E);                       // planes, lane mapping, grid
int diag_em_scan(const EmPlan& E, const DiagModel& M, hipStream_t st);      // the three scan launches over E.W
int diag_em_forward(const eks_dims_t& d, const float* y, const float* var, const DiagModel& M, void* ws, EmPlan& E,
                    hipStream_t st);

}  // namespace eks
