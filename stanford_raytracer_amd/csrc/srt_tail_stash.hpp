// srt_tail_stash.hpp -- the policy of the trace kernels' tail stash (srt_kernels.hpp, HISTORY.md section 29): which rays a wave
// banks while the queue still has fresh ones, and which banked ray a freed lane takes once the queue is empty.
//
// A wave banks a ray when its step count reaches a mark (1/2, 3/4, 7/8, 15/16 of maxsteps), up to a quota per mark.  A ray
// banked at mark k has at most maxsteps - mark[k] accepted steps left: the levels are ordered by falling remainder.  After the
// wave has seen the queue empty it expects to run for about maxsteps more trips (its last fresh ray); a freed lane takes a
// record of the level with the largest remainder that still ends before that, else of the level with the smallest.
//
// Plain functions of integers, host and device: tests/native/tail_stash_policy_main.cpp sweeps them on the CPU, and
// tools/sim_tail_stash.py states the same rules in Python.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRT_STASH_HD __host__ __device__ inline
#else
#define SRT_STASH_HD inline
#endif

namespace srt {

constexpr int STASH_LEVELS = 4;
constexpr int STASH_QUOTA = 32;        // records per wave and mark (tools/sim_tail_stash.py: profiles/tail_stash/sim_table.txt)
constexpr int STASH_MIN_MAXSTEPS = 32; // below it the marks are too close to each other to be worth a record
constexpr int STASH_REC = 18;          // doubles per record: the paused ray's state (TRACE_STATE = 17) and its ray id
constexpr int STASH_STATS = 7;         // srt.h, srt_launch_stash_stats

struct StashPolicy {
  int mark[STASH_LEVELS];  // nstep at which a ray is banked, ascending
  int quota[STASH_LEVELS]; // records a wave banks at most at that mark; all 0 = no banking
};

// The policy of one launch.  lanes = lanes the launch's grid offers (grid x wave_cap); quota_cap < 0 = the default quota.
// No banking where it cannot help: no more rays than lanes (every wave sees the queue empty at its first claim), or a
// maxsteps too small for distinct marks.
SRT_STASH_HD StashPolicy stash_policy(int maxsteps, long long nrays, long long lanes, int quota_cap) {
  StashPolicy sp;
  const bool on = maxsteps >= STASH_MIN_MAXSTEPS && nrays > lanes && quota_cap != 0;
  int q = STASH_QUOTA;
  if (quota_cap > 0 && quota_cap < q) q = quota_cap;
  for (int k = 0; k < STASH_LEVELS; ++k) {
    sp.mark[k] = maxsteps - (maxsteps >> (k + 1));
    sp.quota[k] = on ? q : 0;
  }
  return sp;
}

SRT_STASH_HD int stash_total_quota(const StashPolicy &sp) {
  int n = 0;
  for (int k = 0; k < STASH_LEVELS; ++k) n += sp.quota[k];
  return n;
}

// the level whose mark a ray with step count nstep stands on, or -1
SRT_STASH_HD int stash_bank_level(const StashPolicy &sp, int nstep) {
  int lvl = -1;
  for (int k = 0; k < STASH_LEVELS; ++k)
    if (nstep == sp.mark[k]) lvl = k;
  return lvl;
}

// The level a freed lane takes its record from, `tail_trips` trips after the wave saw the queue empty; fill[k] = records the
// level holds.  -1 when the stash is empty; never a level with fill 0.
SRT_STASH_HD int stash_pick(const StashPolicy &sp, const int fill[STASH_LEVELS], int maxsteps, long long tail_trips) {
  const long long budget = (long long)maxsteps - tail_trips;
  int fits = -1, smallest = -1;
  for (int k = STASH_LEVELS - 1; k >= 0; --k) { // (falling k = rising remainder)
    if (fill[k] <= 0) continue;
    if (smallest < 0) smallest = k;
    if ((long long)(maxsteps - sp.mark[k]) <= budget) fits = k;
  }
  return fits >= 0 ? fits : smallest;
}

} // namespace srt
