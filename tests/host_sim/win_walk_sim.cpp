// Stand-alone check of the walk form's schedule (eks_amd/csrc/eks_win_walk.hpp, read by replay_walk_block in
// eks_diag.hip): the waves, steps and LDS ring slots of a block are played through for every number of chunks and every
// run length, with the kernel's own order of events - in a step every wave first does what it does in front of the
// barrier (load, summarise, write its element and stand-in row), then what it does behind it (read the window's
// elements and the stand-in row, replay) - and with the one freedom the single barrier leaves: the writes in front of
// the barrier of step g + 1 may land while a slower wave still reads behind the barrier of step g.
//
//   win_walk_sim [max_nc [max_run]]      (defaults 200, 30)       exit status 0 and "ok ..." when every property holds
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eks_win_walk.hpp"

using namespace eks;

namespace {

constexpr int kNone = -1000;

struct Slot {
  int chunk = kNone, step = kNone;
};

int fails = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (++fails <= 20) {                        \
        std::printf("FAIL %s: ", #cond);          \
        std::printf(__VA_ARGS__);                 \
        std::printf("\n");                        \
      }                                           \
    }                                             \
  } while (0)

void play(int nc, int R) {
  const int nwg = (nc + kWinG - 1) / kWinG;
  std::vector<int> replayed(nc, 0);
  for (int g0 = 0; g0 < nwg; g0 += R) {
    const int g1 = g0 + R < nwg ? g0 + R : nwg;
    std::vector<Slot> elem(kWalkRing), stand(kWalkStand);
    std::vector<int> held(kWinW, kNone);          // the chunk whose rows a wave has in registers
    std::vector<int> loads(nc, 0);
    std::vector<char> read_elem(kWalkRing, 0), read_stand(kWalkStand, 0);   // what the previous step's replays read
    int n_loaded = 0, n_replayed = 0;
    for (int g = g0; g < g1; ++g) {
      const int base = walk_base(g);
      std::vector<char> seen(kWinW, 0);
      // in front of the barrier
      for (int w = 0; w < kWinW; ++w) {
        const int off = walk_off(g, w), j = walk_chunk(g, w);
        CHECK(off >= 0 && off < kWinW && j == base + off, "nc %d R %d g %d w %d off %d", nc, R, g, w, off);
        CHECK(walk_wave(j) == w, "chunk %d is wave %d's, not wave %d's", j, walk_wave(j), w);
        CHECK(!seen[off], "two waves on chunk %d", j);
        seen[off] = 1;
        if (!walk_loads(off, g == g0)) continue;
        const bool valid = j >= 0 && j < nc;
        CHECK(held[w] == kNone, "nc %d R %d g %d: wave %d loads chunk %d over the rows of chunk %d", nc, R, g, w, j,
              held[w]);
        if (valid) {
          held[w] = j;
          ++loads[j];
          ++n_loaded;
        }
        const int s = walk_elem_slot(j);
        CHECK(s >= 0 && s < kWalkRing, "slot %d", s);
        CHECK(!read_elem[s], "nc %d R %d g %d: element of chunk %d lands in slot %d, which step %d still reads", nc, R, g,
              j, s, g - 1);
        CHECK(elem[s].step != g, "nc %d R %d g %d: two elements in slot %d", nc, R, g, s);
        elem[s] = Slot{j, g};
        if (walk_saves_stand(j)) {
          const int q = walk_stand_slot(j);
          CHECK(q >= 0 && q < kWalkStand, "stand-in slot %d", q);
          CHECK(!read_stand[q], "nc %d R %d g %d: row of chunk %d lands in stand-in slot %d, which step %d still reads",
                nc, R, g, j, q, g - 1);
          CHECK(stand[q].step != g, "nc %d R %d g %d: two rows in stand-in slot %d", nc, R, g, q);
          stand[q] = Slot{j, g};
        }
      }
      // behind the barrier
      read_elem.assign(kWalkRing, 0);
      read_stand.assign(kWalkStand, 0);
      const bool cut_front = base <= 0;
      for (int w = 0; w < kWinW; ++w) {
        const int off = walk_off(g, w), j = walk_chunk(g, w);
        const bool valid = j >= 0 && j < nc;
        if (walk_replays(off) && valid) {
          CHECK(j >= g * kWinG && j < (g + 1) * kWinG, "chunk %d is not group %d's", j, g);
          CHECK(held[w] == j, "nc %d R %d g %d: wave %d replays chunk %d but holds %d", nc, R, g, w, j, held[w]);
          ++replayed[j];
          ++n_replayed;
          for (int q = 0; q < kWinW; ++q) {       // (a wave reads a subset of the window's elements)
            const int s = walk_elem_slot(base + q);
            CHECK(elem[s].chunk == base + q && (elem[s].step == g || (elem[s].step == g - 1 && g > g0)),
                  "nc %d R %d g %d: slot %d holds chunk %d of step %d, wanted chunk %d", nc, R, g, s, elem[s].chunk,
                  elem[s].step, base + q);
            read_elem[s] = 1;
          }
          if (!cut_front) {
            const int q = walk_stand_slot(base);
            CHECK(walk_saves_stand(base), "chunk %d saves no row", base);
            CHECK(stand[q].chunk == base && (stand[q].step == g || (stand[q].step == g - 1 && g > g0)),
                  "nc %d R %d g %d: stand-in slot %d holds chunk %d of step %d, wanted chunk %d", nc, R, g, q,
                  stand[q].chunk, stand[q].step, base);
            read_stand[q] = 1;
          }
        }
        if (!walk_keeps(off)) held[w] = kNone;    // replayed, or a front halo that was only summarised
        else CHECK(!walk_replays(off), "off %d keeps and replays", off);
      }
    }
    int own = 0;
    for (int j = g0 * kWinG; j < g1 * kWinG && j < nc; ++j) ++own;
    for (int j = 0; j < nc; ++j) CHECK(loads[j] <= 1, "nc %d R %d run %d: chunk %d loaded %d times", nc, R, g0, j, loads[j]);
    CHECK(n_replayed == own, "nc %d R %d run %d: %d of %d own chunks replayed", nc, R, g0, n_replayed, own);
    CHECK(n_loaded >= own && n_loaded <= own + 2 * kWinH, "nc %d R %d run %d: %d loads for %d own chunks", nc, R, g0,
          n_loaded, own);
  }
  for (int j = 0; j < nc; ++j) CHECK(replayed[j] == 1, "nc %d R %d: chunk %d replayed %d times", nc, R, j, replayed[j]);
}

}  // namespace

int main(int argc, char** argv) {
  const int max_nc = argc > 1 ? std::atoi(argv[1]) : 200, max_run = argc > 2 ? std::atoi(argv[2]) : 30;
  static_assert(walk_run_length(8, 391, 256) == 13, "the headline: 248 blocks, one round");
  static_assert(kWalkRing >= kWinW + kWinG && kWalkRing % kWinW == 0, "ring size");
  long cases = 0;
  for (int nc = 1; nc <= max_nc; ++nc)
    for (int R = 1; R <= max_run; ++R, ++cases) play(nc, R);
  for (int ntile = 1; ntile <= 130; ntile += 3)
    for (int nwg = 1; nwg <= 520; nwg += 7) {
      const int r = walk_run_length(ntile, nwg, 256);
      CHECK(r >= 1 && r <= nwg, "run length %d for %d tiles x %d groups", r, ntile, nwg);
    }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ok %ld cases\n", cases);
  return 0;
}
