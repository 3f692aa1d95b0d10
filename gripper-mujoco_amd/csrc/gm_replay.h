// gm_replay.h -- the DQN replay memory's device side shared by the batched kernels (gm_replay.hip)
// and the fused rollout (gm_rollout.h): the ring-row rule, the keyed bijection behind the
// without-replacement draw (host and device, gm_replay_indices / gm_replay_sample) and the fused
// recorder replay_record.
//
// Reference: rl/agents/DQN.py:11-62 ReplayMemory (a deque of Transition(state, action, next_state,
// reward, terminal); push appends, batch is random.sample: without replacement) and
// rl/Trainer.py:659-684 (one push per env-step, next_state always the post-step observation).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gm_policy_net.h"

// The device view of a caller's gm_replay and the ring position of a call (gm_capi.hip fills it;
// gm_policy_rollout_replay hands the kernel a device copy through GmRolloutJob::replay).
struct GrArgs {
  float* state;              // [capacity][n_obs]
  int32_t* action;           // [capacity]
  float* next_state;         // [capacity][n_obs]
  float* reward;             // [capacity]
  uint8_t* end;              // [capacity] gm_episode_end_code's values
  long long capacity;
  long long row0;            // transitions pushed before the call, reduced modulo capacity
  int n_obs, pad;
};

// Ring row of env `env` at env-step k of a call: (pushed + k n_envs + env) % capacity -- the
// reference's deque with every env pushed in env order each step.  row0 = pushed % capacity and a
// call writes no row twice (n_steps * n_envs <= capacity), so one subtraction reduces the sum.
__host__ __device__ inline long long gr_row(long long row0, int k, int n_envs, int env, long long capacity) {
  const long long r = row0 + (long long)k * n_envs + env;
  return r >= capacity ? r - capacity : r;
}

// The draw: index i of draw `draw` is the image of i under a keyed bijection of [0, size) -- a
// balanced Feistel network of 4 rounds over b bits, b the smallest even count with 2^b >= size,
// round function gp_mix(key + round constant + R) masked to b / 2 bits, cycle-walked until the
// value is < size (2^b < 4 size: fewer than 4 expected walks).  Distinct i give distinct rows:
// a batch without replacement, like random.sample, from a counter-based stream.
#define GR_ROUNDS 4
__host__ __device__ inline uint64_t gr_key(uint64_t seed, uint64_t draw) { return gp_mix(seed ^ gp_mix(draw)); }
__host__ __device__ inline int gr_half_bits(uint64_t size) {
  int h = 0;
  while (h < 32 && (1ull << (2 * h)) < size) h++;
  return h;
}
__host__ __device__ inline uint64_t gr_index(uint64_t size, uint64_t key, uint64_t i) {
  const int h = gr_half_bits(size);
  const uint64_t mask = (1ull << h) - 1ull;
  uint64_t x = i;
  do {
    uint64_t L = x >> h, R = x & mask;
    for (int r = 0; r < GR_ROUNDS; r++) {
      const uint64_t f = gp_mix(key + (uint64_t)(r + 1) * 0xD1B54A32D192ED03ull + R) & mask;
      const uint64_t t = L ^ f;
      L = R;
      R = t;
    }
    x = (L << h) | R;
  } while (x >= size);
  return x;
}

// The fused recorder (gm_policy_rollout_replay): one env's part of gm_policy_push_begin (phase 0:
// the observation the action was chosen from, and the action) or gm_policy_push_end (phase 1: the
// post-step observation, the reward, the end code) on the env's own wave, between env-steps only.
// obs: the env's observation row, written by this wave (the epilogue, a reset) or by an earlier
// wave of the env -- read as gp_forward_one reads it: the wave's stores drained, then agent-scope
// loads past this CU's L1.  code: the action (phase 0) or the end code (phase 1); rew: the env's
// reward (phase 1, read by lane 0).  The rows go out as plain vector stores: nothing reads them
// before the launch ends.
__device__ __noinline__ void replay_record(int phase, const GrArgs* __restrict__ Rp, const float* obs, int env,
                                           int n_envs, int k, int code, const float* rew, int lane) {
  const GrArgs& R = *Rp;
  const size_t row = (size_t)gr_row(R.row0, k, n_envs, env, R.capacity);
  float* dst = (phase == 0 ? R.state : R.next_state) + row * (size_t)R.n_obs;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  for (int j = lane; j < R.n_obs; j += 64) dst[j] = __hip_atomic_load(obs + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (lane == 0) {
    if (phase == 0) {
      R.action[row] = code;
    } else {
      R.reward[row] = *rew;
      R.end[row] = (uint8_t)code;
    }
  }
}
