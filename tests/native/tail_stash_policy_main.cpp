// tail_stash_policy_main.cpp -- a sweep of the tail stash's policy functions (csrc/srt_tail_stash.hpp) on the CPU, for
// tests/test_tail_stash_policy.py.  Prints "ok <checks>" and returns 0, or says what failed and returns 1.
#include "../../stanford_raytracer_amd/csrc/srt_tail_stash.hpp"

#include <cstdio>
#include <cstdlib>

using namespace srt;

static long long checks = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    ++checks;                                \
    if (!(cond)) {                           \
      std::printf("FAILED %s: ", #cond);     \
      std::printf(__VA_ARGS__);              \
      std::printf("\n");                     \
      return 1;                              \
    }                                        \
  } while (0)

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n) { // xorshift64*: a value in 0 .. n - 1
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (unsigned)(((rng_state * 0x2545f4914f6cdd1dull) >> 33) % n);
}

int main() {
  // ---- the launch's policy
  for (int maxsteps = 1; maxsteps <= 4096; ++maxsteps) {
    const StashPolicy on = stash_policy(maxsteps, 1000, 128, -1);
    const bool expect = maxsteps >= STASH_MIN_MAXSTEPS;
    for (int k = 0; k < STASH_LEVELS; ++k) {
      CHECK(on.quota[k] == (expect ? STASH_QUOTA : 0), "maxsteps %d level %d quota %d", maxsteps, k, on.quota[k]);
      if (!expect) continue;
      CHECK(on.mark[k] >= 2 && on.mark[k] < maxsteps, "maxsteps %d mark %d", maxsteps, on.mark[k]);
      if (k > 0) CHECK(on.mark[k] > on.mark[k - 1], "maxsteps %d marks %d %d not ascending", maxsteps, on.mark[k - 1], on.mark[k]);
    }
    CHECK(stash_total_quota(on) == (expect ? STASH_LEVELS * STASH_QUOTA : 0), "maxsteps %d", maxsteps);
    // no more rays than lanes, or switched off: no banking; a cap caps, and never raises
    CHECK(stash_total_quota(stash_policy(maxsteps, 128, 128, -1)) == 0, "rays == lanes, maxsteps %d", maxsteps);
    CHECK(stash_total_quota(stash_policy(maxsteps, 0, 0, -1)) == 0, "no rays, maxsteps %d", maxsteps);
    CHECK(stash_total_quota(stash_policy(maxsteps, 1000, 128, 0)) == 0, "cap 0, maxsteps %d", maxsteps);
    CHECK(stash_total_quota(stash_policy(maxsteps, 1000, 128, 1)) == (expect ? STASH_LEVELS : 0), "cap 1, maxsteps %d", maxsteps);
    CHECK(stash_total_quota(stash_policy(maxsteps, 1000, 128, 1000)) == (expect ? STASH_LEVELS * STASH_QUOTA : 0), "cap 1000, maxsteps %d", maxsteps);
    // a step count stands on at most one mark, and on exactly the marks
    if (expect && maxsteps <= 600)
      for (int nstep = 0; nstep <= maxsteps + 1; ++nstep) {
        const int lvl = stash_bank_level(on, nstep);
        int want = -1;
        for (int k = 0; k < STASH_LEVELS; ++k)
          if (on.mark[k] == nstep) want = k;
        CHECK(lvl == want, "maxsteps %d nstep %d level %d, expected %d", maxsteps, nstep, lvl, want);
      }
  }
  // ---- the pick
  const int sizes[] = {32, 33, 47, 64, 100, 256, 257, 2000};
  for (int maxsteps : sizes) {
    const StashPolicy sp = stash_policy(maxsteps, 1000, 128, -1);
    for (int trial = 0; trial < 4000; ++trial) {
      int fill[STASH_LEVELS], total = 0;
      for (int k = 0; k < STASH_LEVELS; ++k) {
        fill[k] = rnd(3) == 0 ? 0 : (int)rnd((unsigned)sp.quota[k] + 1);
        total += fill[k];
      }
      long long trips = rnd(2) ? (long long)rnd((unsigned)(2 * maxsteps)) : (long long)rnd(8);
      // drain it: one record per pick, trips moving on now and then, as in the kernel
      for (int left = total; left > 0; --left) {
        const int k = stash_pick(sp, fill, maxsteps, trips);
        CHECK(k >= 0 && k < STASH_LEVELS, "maxsteps %d: pick %d with %d records left", maxsteps, k, left);
        CHECK(fill[k] > 0, "maxsteps %d: picked the empty level %d", maxsteps, k);
        const long long budget = (long long)maxsteps - trips;
        int best_fit = -1, smallest = -1; // by remainder: level 0 has the largest
        for (int q = 0; q < STASH_LEVELS; ++q) {
          if (fill[q] == 0) continue;
          if (maxsteps - sp.mark[q] <= budget && best_fit < 0) best_fit = q;
          smallest = q;
        }
        CHECK(k == (best_fit >= 0 ? best_fit : smallest), "maxsteps %d trips %lld fill %d %d %d %d: picked %d, largest fitting %d, smallest %d",
              maxsteps, trips, fill[0], fill[1], fill[2], fill[3], k, best_fit, smallest);
        --fill[k];
        trips += rnd(3);
      }
      CHECK(fill[0] == 0 && fill[1] == 0 && fill[2] == 0 && fill[3] == 0, "maxsteps %d: records left behind", maxsteps);
      CHECK(stash_pick(sp, fill, maxsteps, trips) == -1, "maxsteps %d: a pick from the empty stash", maxsteps);
    }
  }
  std::printf("ok %lld\n", checks);
  return 0;
}
