// Geometry of the windowed replay and the schedule of its walk form (eks_diag.hip: replay_walk_block): which wave
// holds which chunk in which step, and where a chunk's element and stand-in row live in LDS.  Plain constexpr
// arithmetic so that the kernel and tests/host_sim/win_walk_sim.cpp read the same code.
//
// A block of the walk form is (64-chain tile, run of R consecutive window groups) and takes one group per step.  In
// the step of group g the kWinW = 12 consecutive chunks from walk_base(g) = g kWinG - kWinH on are the group's window
// (front halo, own chunks, back halo).  Chunk j belongs to wave j mod kWinW for the whole run, so each of the window's
// chunks has a wave of its own; `off` = j - walk_base(g) is what the wave does in the step:
//
//   off  0 ..  1  front halo   = own chunks 6, 7 of group g - 1: replayed in the previous step, their elements are
//                                still in LDS.  Idle - except in the run's first step, which loads and summarises them.
//   off  2 ..  3  carried      = own chunks 0, 1: loaded and summarised in the previous step as its back halo, rows
//                                still in registers.  Replays.  (First step of a run: loads and summarises as well.)
//   off  4 ..  9  own chunks 2 .. 7: loads, summarises, replays.
//   off 10 .. 11  back halo    = own chunks 0, 1 of group g + 1: loads, summarises, keeps its rows for the next step.
//
// One barrier per step, between the summarise and the replay phase.
#pragma once

namespace eks {

#ifndef EKS_WIN_G
#define EKS_WIN_G 8
#endif
constexpr int kWinG = EKS_WIN_G;           // own chunks of a block
constexpr int kWinH = 2;                   // halo chunks on either side (64 frames)
constexpr int kWinW = kWinG + 2 * kWinH;   // waves of a block
static_assert(kWinG >= 2 * kWinH, "the carried chunks of a step and the chunks whose elements the next step's front "
                                  "halo needs are different own chunks");

// LDS rings.  A wave that has passed the barrier of step g reads the window's kWinW elements while a faster wave may
// already be writing the elements of step g + 1 - the kWinG chunks behind the window - in front of the next barrier;
// nobody writes the elements of step g + 2 before every wave has passed the barrier of step g + 1, i.e. has finished
// the reads of step g.  Chunks that must not share a slot are therefore kWinW + kWinG = 20 consecutive ones; the ring
// has 2 kWinW = 24 slots (chunk j in slot j mod 24, that is the wave's index or that plus kWinW).
constexpr int kWalkRing = 2 * kWinW;
// The stand-in row (first observation of the front halo's first chunk) of group g is saved in step g - 1 (run start:
// in step g), read behind the barrier of step g, and the row of group g + 2 is written in front of the barrier of
// step g + 1: three groups' rows are distinct at any time.
constexpr int kWalkStand = 3;

constexpr int walk_base(int g) { return g * kWinG - kWinH; }                 // first chunk of the window (may be < 0)
constexpr int walk_wave(int j) { return (j + kWinW) % kWinW; }               // j >= -kWinH
constexpr int walk_off(int g, int w) { return (w + kWinW - walk_wave(walk_base(g))) % kWinW; }
constexpr int walk_chunk(int g, int w) { return walk_base(g) + walk_off(g, w); }
constexpr bool walk_loads(int off, bool first_step) { return first_step || off >= 2 * kWinH; }
constexpr bool walk_replays(int off) { return off >= kWinH && off < kWinH + kWinG; }
constexpr bool walk_keeps(int off) { return off >= kWinH + kWinG; }          // rows stay in registers for the next step
constexpr int walk_elem_slot(int j) { return (j + kWalkRing) % kWalkRing; }
constexpr bool walk_saves_stand(int j) { return (j + kWinH) % kWinG == 0; }  // first chunk of some group's front halo
constexpr int walk_stand_slot(int j) { return ((j + kWinH) / kWinG) % kWalkStand; }

// Run length from the launch alone (the outputs do not depend on it): the R that minimises
// rounds of blocks x (R steps + kWalkRunEnd), where a run's ends cost about one step - the first step loads and
// summarises twelve chunks instead of eight and the last loads a back halo nobody replays.  Ties go to the shorter run.
// 8 tiles x 391 groups on 256 CUs: R = 13, 248 blocks, one round.
constexpr int kWalkRunEnd = 1;
constexpr int walk_run_length(int ntile, int nwg, int ncu) {
  long best = -1;
  int br = 1;
  for (int r = 1; r <= nwg; ++r) {
    const long blocks = (long)ntile * ((nwg + r - 1) / r);
    const long cost = ((blocks + ncu - 1) / ncu) * (r + kWalkRunEnd);
    if (best < 0 || cost < best) {
      best = cost;
      br = r;
    }
  }
  return br;
}

}  // namespace eks
