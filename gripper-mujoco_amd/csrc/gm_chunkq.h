// gm_chunkq.h -- the persistent work queue of gm_step_kernel's chunked mode (DESIGN.md §5,
// "Chunked dispatch", "The seam between the queue and the drivers"): the job it carries, its
// memory layout (shared with gm_capi.hip's diagnostics) and the device pieces chunked_env_steps
// is composed from.  It schedules JOBS -- job.steps env-steps of one env -- and reads no more of one.
#pragma once
#include <stdint.h>
#include "gm_state.h"
#include "gm_policy_net.h"
#include "gm_ac_net.h"
#include "gm_replay.h"
#include "gm_sac_net.h"

#define GM_CQ_NB 16      // priority buckets per XCD
// The job every env of a launch runs: `steps` env-steps in a row, each the per-step API's sequence:
// driver actions -> action_step + obs / done / reward -> gm_autoreset_episodes' record and reset
enum GmDriver {              // gm_rollout_params::action_mode for the scripted ones
  GM_DRV_NONE = -1,          // gm_step: one plain env-step, the actions already set, no reset
  GM_DRV_SCRIPT = 0,         // scripted grasp mix (gm_scripted_actions)
  GM_DRV_RANDOM = 1,         // uniform random (gm_random_actions)
  GM_DRV_DQN = 2,            // the DQN policy picks a discrete action (gm_policy_rollout)
  GM_DRV_PROGRAM = 3,        // grasp program (gm_program_actions)
  GM_DRV_MIX = 4,            // the program in 1 episode of 4, the scripted mix otherwise
  GM_DRV_AC = 5,             // the PPO actor-critic samples continuous actions (gm_ac_rollout)
  GM_DRV_SAC = 6             // the SAC squashed actor samples continuous actions (gm_sac_rollout)
};
struct GmRolloutJob {
  int steps, driver;         // driver: GmDriver
  uint64_t seed;             // the driver's (scripted draws, the policy's exploration)
  float jitter;
  int max_ep;                // truncation (num_action_steps >= max_ep), <= 0 off
  gm_episode_end* rec;       // [steps][n_envs] episode-end records (may be NULL)
  const double* eq;          // the reset's inputs: the settled equilibrium (calibrate_reset),
  const gm_object* objs;     // the object set, the scene spawn and the spawn draws
  int n_objects, scene_tries;
  const gm_spawn_params* scene;
  GmSpawnRand sr;            // (env_offset: the drivers' global env ids even without random spawns)
  const float* pparams;      // GM_DRV_DQN: packed network (gm_policy_pack layout),
  GpNet pnet;
  const float* peps;         // [steps] exploration threshold per env-step of the launch,
  uint64_t pdecision;        // the first env-step's decision index
  union {                    // device copy of the launch's arguments: one slot, so that both reach
    const GaArgs* ac;        // GM_DRV_AC's ...
    const GsArgs* sac;       // ... and GM_DRV_SAC's driver through the one call of ac_rollout_driver
  };
  const GrArgs* replay;      // GM_DRV_DQN: device copy of the replay memory to record into (NULL: none);
                             // GM_DRV_SAC: the same with a NULL action, for the second half of its push
  // an evaluation launch (gm_evaluate and the like; DESIGN.md §5, "Evaluation launch"; the EVAL
  // instantiations of the kernel): an env whose episode ends writes its report into ev and
  // retires instead of being reset.  Not read by the other kernels.
  const uint8_t* active;     // [n_envs] envs that take part (NULL: all); the others finish at their fresh pick
  gm_eval_out ev;
};
struct GmChunkCarry {        // what a chunk hands the next besides the hot state
  int32_t sub_done, nsub;
  int32_t work_nefc, work_mpr, work_newton, stp_fixed;
  uint32_t clk;              // s_memtime / 64 summed over this env-step's chunks
  int32_t yielded;           // yields so far this env-step (at most GmChunkQ::max_yields)
  int32_t steps_left;        // env-steps of this launch's job still to run, the current one included
  int32_t step_idx;          // index of the current env-step in the launch (rollout records)
  int32_t job_yields;        // yields over the whole job (gm_chunk_job_stats)
};
// Counter words (GmChunkQ::ctr; zeroed by gm_dispatch_order_kernel before every launch), one
// 128-B line per contended word: ring r = x * GM_CQ_NB + bucket has its head at [r * 32], its
// tail at [r * 32 + 1]; the launch's at GM_CQ_FRESH + GmCqCounter, the previous one's at GM_CQ_LAST
#define GM_CQ_FRESH (8 * GM_CQ_NB * 32)
enum GmCqCounter {
  GM_CQC_FRESH = 0,          // the next unstarted env (index into the dispatch order)
  GM_CQC_DONE = 32,          // envs whose job finished
  GM_CQC_YIELDS,
  GM_CQC_RESUMES,
  GM_CQC_CMAX,               // this launch's bucket scale (written by the order kernel)
  GM_CQC_STEALS,             // resumes on another XCD than the one that queued the env
  GM_CQC_CLAIM_WAITS,        // claims whose slot was still empty (its producer had not stored yet)
  GM_CQC_CLAIM_POLLS,        // polls those claims made
  GM_CQC_N
};
#define GM_CQ_WORDS (GM_CQ_FRESH + 64)
#define GM_CQ_LAST GM_CQ_WORDS
#define GM_CQ_ALLOC (GM_CQ_WORDS + 64)
static_assert(GM_CQC_N <= 64, "the launch's counters fit their block");
// Time words (GmChunkQ::st; 100 MHz clock): the launch's, the previous launch's (gm_chunk_stats),
// then the timeline (gm_chunk_timeline): each workgroup's last work, each env's first pick / finish
enum GmCqTime {
  GM_CQT_FIRST_PICK = 0,
  GM_CQT_FIRST_EMPTY,        // first pick that found no unstarted env
  GM_CQT_LAST_DONE,          // last env finished
  GM_CQT_BUSY,               // wave-busy and
  GM_CQT_POLL,               // wave-polling sums
  GM_CQT_N,
  GM_CQT_LAST = 8,
  GM_CQT_TIMELINE = 16
};
__host__ __device__ inline size_t cq_time_of_wave(int w) { return (size_t)GM_CQT_TIMELINE + (size_t)w; }
__host__ __device__ inline size_t cq_time_of_env(int grid, int env) { return cq_time_of_wave(grid) + 2 * (size_t)env; }
struct GmChunkQ {
  uint32_t* ctr;             // GM_CQ_ALLOC words
  uint64_t* ring;            // [8 * GM_CQ_NB][cap] (predicted work left << 32) | (env + 1), 0 = empty
  GmChunkCarry* carry;       // [n_envs]
  int cap;                   // ring slots per bucket: n_envs + launched waves
  int chunk;                 // substeps between preemption tests (0: the one-shot kernel)
  int margin;                // yield when work left * (100 + margin) < next unstarted env's * 100
  int max_yields;            // per env per env-step
  int cmargin;               // yield to a yielded env with cmargin percent more work left (< 0: off)
  unsigned long long* st;    // GmCqTime words
  int steal;                 // an idle wave may resume a yielded env of another XCD
  int prio;                  // > 0: issue priority by predicted work left (job_prio)
  GmRolloutJob job;          // what each env runs (steps = 1, no driver: gm_step's plain env-step)
};
// Preemption test of the chunked env-step (substep_loop): every `every` substeps the
// loop yields when the predicted work left in this env, own * left / total (the env's last
// dispatch cost, shader clocks / 64, spread evenly over its substeps), has dropped below the
// next unstarted env's cost -- longest-remaining-work-first at substep granularity.
struct GmPreempt {
  const uint32_t* fresh_head;   // the queue's next-unstarted index (agent-scope loads)
  const int32_t* order;
  const uint32_t* cost;
  uint32_t n, own;
  int left, total, every;       // every = 0: never yield
  int margin;                   // percent
  // the XCD's yielded envs: a running env also yields to the best bucket when that bucket's
  // lower edge (cmax * b / GM_CQ_NB) exceeds its own work left by cmargin percent (< 0: off)
  const uint32_t* bq;
  uint32_t cmax;
  int cmargin;
  int prio;                     // > 0: the wave's issue priority follows the work left (job_prio)
  int steps;                    // env-steps per job: the cost array holds per-env-step costs
};
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ld_agent64(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t add_agent(uint32_t* p, uint32_t v) {
  return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t* cq_counter(const GmChunkQ& q, GmCqCounter c) { return q.ctr + GM_CQ_FRESH + c; }
// The wave's VALU issue priority from its job's predicted work left (rem) against the launch's
// heaviest job (cmax): 0..3 in quarters.  Two waves share a SIMD's issue by priority, then age
// (MI355X_MICROARCH.md); the persistent grid's waves never change age, so without this the job
// with the most work left runs at the younger wave's pace on half the SIMDs.
__device__ __forceinline__ void job_prio(uint64_t rem, uint32_t cmax, int mode) {
  if (mode <= 0) return;
  const uint32_t p = __builtin_amdgcn_readfirstlane((uint32_t)(rem * 4u / (uint64_t)(cmax ? cmax : 1u)));
  if (p >= 3) __builtin_amdgcn_s_setprio(3);
  else if (p == 2) __builtin_amdgcn_s_setprio(2);
  else if (p == 1) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
}
// The cost recorded for the next launch's dispatch order, per env-step, from a job of `steps`
// env-steps: the measured clocks / 64 (co-residency noise) averaged with a work model (fixed
// part, Hessian work per constraint row, collider latency per substep that ran it, Newton
// iterations; fitted on C3, tools/tail_bench.py; LPT makespan 1.17 vs 1.21 of the ideal)
__device__ __forceinline__ uint32_t dispatch_cost(uint32_t clocks, uint32_t steps, int work_nefc, int work_mpr,
                                                  int work_newton) {
  const uint32_t model = 14000u * steps + 19u * (uint32_t)work_nefc + 188u * (uint32_t)work_mpr +
                         940u * (uint32_t)work_newton;
  return ((clocks >> 1) + (model >> 1)) / steps;
}
// A job's length in env-steps (costs are per env-step) and its work left / total in substeps
// (s_nom: nominal substeps per env-step).  (Scalars: a struct return cost 16 B more scratch.)
__device__ __forceinline__ int cq_job_scale(const GmChunkQ& q) { return q.job.steps > 1 ? q.job.steps : 1; }
__device__ __forceinline__ int cq_job_left(const GmChunkCarry& cr, int s_nom) {
  return (cr.steps_left - 1) * s_nom + (cr.nsub - cr.sub_done);
}
__device__ __forceinline__ int cq_job_total(const GmChunkQ& q, const GmChunkCarry& cr, int s_nom) {
  return q.job.steps > 1 ? q.job.steps * s_nom : cr.nsub;
}
// Claim the next entry of a yielded-env bucket (head at b[0], tail at b[1]; lane 0): the head
// advances only while it is below the tail, so every claimed slot was reserved by a producer
// that is about to store it -- two waves that saw the same last entry cannot both claim, and
// the loser parks on no slot that a future yield would have to fill.  Returns the slot or -1.
__device__ __forceinline__ int64_t claim_bucket(uint32_t* b) {
  uint32_t h = ld_agent(b);
  for (;;) {
    if (h >= ld_agent(b + 1)) return -1;
    if (__hip_atomic_compare_exchange_strong(b, &h, h + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return (int64_t)h;
  }
}
// Lane 0 takes the next yielded env of a bucket (counters b, ring rb; stolen: another XCD's):
// claims a slot, waits for its producer's entry (acquire, pairs with its release), clears it.
// Returns 0 when the entry went to another wave; else 1 and pick, unless all finished meanwhile.
__device__ __forceinline__ int cq_claim(const GmChunkQ& q, uint32_t* b, uint64_t* rb, uint32_t n, bool stolen,
                                        int& pick) {
  const int64_t c = claim_bucket(b);
  if (c < 0) return 0;
  const uint32_t i = (uint32_t)c % (uint32_t)q.cap;
  uint64_t v;
  uint32_t polls = 0;
  while ((v = __hip_atomic_load(rb + i, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) == 0ull &&
         ld_agent(cq_counter(q, GM_CQC_DONE)) < n) {
    __builtin_amdgcn_s_sleep(2);
    polls++;
  }
  if (polls) { add_agent(cq_counter(q, GM_CQC_CLAIM_WAITS), 1u); add_agent(cq_counter(q, GM_CQC_CLAIM_POLLS), polls); }
  if (v != 0ull) {
    st_agent(rb + i, 0ull);
    add_agent(cq_counter(q, GM_CQC_RESUMES), 1u);
    if (stolen) add_agent(cq_counter(q, GM_CQC_STEALS), 1u);
    pick = (int)(uint32_t)v - 1;
  }
  return 1;
}
struct GmCqWave {            // one wave's view of the queue
  int xcc;                   // the XCD it runs on (HW_REG_XCC_ID),
  uint32_t* bq;              // that XCD's bucket counters
  uint64_t* ring;            // and rings
  uint32_t n;                // envs of the launch
  uint32_t cmax;             // bucket scale: the launch's heaviest last cost + 1, times the job length
  bool saw_empty;            // a pick of this wave has found no unstarted env
};
__device__ __forceinline__ GmCqWave cq_wave(const GmChunkQ& q, int n_envs) {
  int xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  xcc &= 7;
  return {xcc, q.ctr + xcc * GM_CQ_NB * 32, q.ring + (size_t)xcc * GM_CQ_NB * q.cap, (uint32_t)n_envs,
          *cq_counter(q, GM_CQC_CMAX) * (uint32_t)cq_job_scale(q), false};
}
// Take work: a continuation queued on this XCD when it is the longer job, else the next unstarted
// env in cost order (fresh = 1), else (q.steal) another XCD's best yielded env; -1: all finished
struct GmCqPick { int env, fresh; };
__device__ __forceinline__ GmCqPick cq_take_work(const GmChunkQ& q, GmCqWave& w, const int32_t* __restrict__ order,
                                                 const uint32_t* __restrict__ cost, int lane) {
  uint32_t* fresh_head = cq_counter(q, GM_CQC_FRESH);
  const uint32_t* n_done = cq_counter(q, GM_CQC_DONE);
  const uint32_t n = w.n;
  int pick = -1, fresh = 0;
  for (;;) {
    // bucket occupancy, one lane per bucket; the highest non-empty bucket is the best yielded
    // env (its exact work left rides in the entry; an entry in flight reads 0, counts as large)
    uint32_t hb = 0, tb = 0;
    if (lane < GM_CQ_NB) { hb = ld_agent(w.bq + lane * 32); tb = ld_agent(w.bq + lane * 32 + 1); }
    const unsigned long long ne = __ballot(lane < GM_CQ_NB && hb < tb);
    const uint32_t fh = __builtin_amdgcn_readfirstlane(ld_agent(fresh_head));
    const bool have_f = fh < n;
    if (!have_f && !w.saw_empty) {
      w.saw_empty = true;
      if (lane == 0)
        __hip_atomic_fetch_min(q.st + GM_CQT_FIRST_EMPTY, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    const int bsel = ne ? 63 - __builtin_clzll(ne) : -1;
    bool take_c = bsel >= 0;
    if (take_c && have_f) {
      const uint32_t h = __builtin_amdgcn_readlane(hb, bsel);
      const uint64_t e = ld_agent64(w.ring + (size_t)bsel * q.cap + h % (uint32_t)q.cap);
      take_c = e == 0ull || (uint64_t)(uint32_t)(e >> 32) >= (uint64_t)cost[order[fh]] * (uint64_t)cq_job_scale(q);
    }
    if (take_c) {
      int got = 0;
      if (lane == 0) got = cq_claim(q, w.bq + bsel * 32, w.ring + (size_t)bsel * q.cap, n, false, pick);
      if (__builtin_amdgcn_readfirstlane(got)) break;   // pick < 0: everything finished while waiting
      continue;                                          // the entry went to another wave: poll again
    }
    if (have_f) {
      if (lane == 0) {
        const uint32_t i = add_agent(fresh_head, 1u);
        if (i < n) { pick = order[i]; fresh = 1; }
      }
      if (__builtin_amdgcn_readfirstlane(pick) >= 0) break;
    } else if (q.steal) {
      // nothing unstarted or yielded on this XCD: the best yielded env of another (agent-scope
      // release / acquire).  Lane l looks at XCD l / 8, buckets 15 - l % 8 and 7 - l % 8.
      const int x2 = lane >> 3;
      const uint32_t* bq2 = q.ctr + x2 * GM_CQ_NB * 32;
      const int bh = 15 - (lane & 7), bl = 7 - (lane & 7);
      const bool other = x2 != w.xcc;
      const bool nh = other && ld_agent(bq2 + bh * 32) < ld_agent(bq2 + bh * 32 + 1);
      const bool nl = other && ld_agent(bq2 + bl * 32) < ld_agent(bq2 + bl * 32 + 1);
      const unsigned long long mh = __ballot(nh), ml = __ballot(nl);
      if (mh | ml) {
        // the highest non-empty bucket over the other XCDs (lowest lane among equals)
        int src = -1, sb = -1;
        for (int r = 0; r < 8 && src < 0; r++) {   // bucket 15 - r in the high half, lanes with lane % 8 == r
          const unsigned long long m8 = mh & (0x0101010101010101ull << r);
          if (m8) { src = (int)__builtin_ctzll(m8) >> 3; sb = 15 - r; }
        }
        for (int r = 0; r < 8 && src < 0; r++) {
          const unsigned long long m8 = ml & (0x0101010101010101ull << r);
          if (m8) { src = (int)__builtin_ctzll(m8) >> 3; sb = 7 - r; }
        }
        int got = 0;
        if (lane == 0)
          got = cq_claim(q, q.ctr + src * GM_CQ_NB * 32 + sb * 32,
                         q.ring + (size_t)src * GM_CQ_NB * q.cap + (size_t)sb * q.cap, n, true, pick);
        if (__builtin_amdgcn_readfirstlane(got)) break;   // pick < 0: everything finished while waiting
      }
    }
    if (__builtin_amdgcn_readfirstlane(ld_agent(n_done)) >= n) break;
    __builtin_amdgcn_s_sleep(2);
  }
  return {__builtin_amdgcn_readfirstlane(pick), __builtin_amdgcn_readfirstlane(fresh)};
}
// Publish a yielded env whose state and carry this wave has stored (MI355X_MICROARCH.md,
// inter-workgroup visibility, valid forms): stores drained, the env's own sync, lane 0's
// agent-scope release (visible on ANY XCD after an acquire), drained again, then the relaxed
// agent ring store into the bucket of the job's work left, own * left / total (own: job cost)
__device__ __forceinline__ void cq_publish_yield(const GmChunkQ& q, const GmCqWave& w, uint64_t own, int left,
                                                 int total, int env, int lane) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (lane == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint64_t rem = own * (uint64_t)left / (uint64_t)total;
    add_agent(cq_counter(q, GM_CQC_YIELDS), 1u);
    const uint32_t b = rem * GM_CQ_NB / w.cmax < GM_CQ_NB - 1 ? (uint32_t)(rem * GM_CQ_NB / w.cmax) : GM_CQ_NB - 1;
    const uint32_t t = add_agent(w.bq + b * 32 + 1, 1u) % (uint32_t)q.cap;
    __hip_atomic_store(w.ring + (size_t)b * q.cap + t,
                       ((rem > 0xFFFFFFFFull ? 0xFFFFFFFFull : rem) << 32) | ((uint64_t)env + 1u), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
}
