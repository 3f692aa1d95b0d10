// gm_replay.hip -- the batched kernels of the DQN replay memory: the two halves of a push
// (gm_policy_push_begin / gm_policy_push_end), the gather of a sampled batch (gm_replay_sample)
// and the TD target (gm_policy_td_target).  The ring rule, the draw and the fused rollout's
// recorder are gm_replay.h's; the forward and the softmax are gm_policy_net.h's.
#pragma once
#include "gm_state.h"
#include "gm_replay.h"

// ReplayMemory.push, first half (after gm_policy_act): state and action of every env into its
// ring row.  One thread per observation element; the thread of element 0 writes the scalar.
__global__ __launch_bounds__(256) void gm_replay_push_begin_kernel(const float* __restrict__ obs,
                                                                   const int32_t* __restrict__ actions, int n_envs,
                                                                   GrArgs R) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n_envs * R.n_obs) return;
  const int env = (int)(i / R.n_obs), j = (int)(i - (long long)env * R.n_obs);
  const size_t row = (size_t)gr_row(R.row0, 0, n_envs, env, R.capacity);
  R.state[row * (size_t)R.n_obs + j] = obs[i];
  if (j == 0) R.action[row] = actions[env];
}

// ReplayMemory.push, second half (after gm_step, before the auto-reset): the post-step
// observation, the reward and the end code (gm_episode_end_code: 1 terminal, 2 truncated only)
__global__ __launch_bounds__(256) void gm_replay_push_end_kernel(const float* __restrict__ obs,
                                                                 const GmEnvState* __restrict__ states,
                                                                 const float* __restrict__ rew,
                                                                 const uint8_t* __restrict__ done, int n_envs,
                                                                 int max_ep, GrArgs R) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n_envs * R.n_obs) return;
  const int env = (int)(i / R.n_obs), j = (int)(i - (long long)env * R.n_obs);
  const size_t row = (size_t)gr_row(R.row0, 0, n_envs, env, R.capacity);
  R.next_state[row * (size_t)R.n_obs + j] = obs[i];
  if (j == 0) {
    R.reward[row] = rew[env];
    R.end[row] = (uint8_t)gm_episode_end_code(done[env], states[env].num_action_steps, max_ep);
  }
}

// ReplayMemory.batch: row b of the batch is ring row gr_index(size, key, b).  One thread per
// observation element, so a wave reads and writes whole rows contiguously; every thread of a
// row walks the same few rounds of the bijection (cheaper than a second launch for the indices).
__global__ __launch_bounds__(256) void gm_replay_sample_kernel(GrArgs R, long long size, int batch, uint64_t key,
                                                               gm_replay_batch out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)batch * R.n_obs) return;
  const int b = (int)(i / R.n_obs), j = (int)(i - (long long)b * R.n_obs);
  const size_t row = (size_t)gr_index((uint64_t)size, key, (uint64_t)b);
  out.state[i] = R.state[row * (size_t)R.n_obs + j];
  out.next_state[i] = R.next_state[row * (size_t)R.n_obs + j];
  if (j == 0) {
    out.action[b] = R.action[row];
    out.reward[b] = R.reward[row];
    out.end[b] = R.end[row];
    out.index[b] = (int32_t)row;
  }
}

// The TD target of n batch rows, one wave per 16 rows (Agent_DQN.optimise_model,
// rl/agents/DQN.py:294-315): y = reward + gamma v, with v the maximum of the target net's softmax
// outputs on next_state or, with an online net (oparams != NULL: double DQN), the target net's
// output at the online net's first argmax.  mask_terminal: v = 0 where end == 1 (a truncated
// row, end == 2, keeps its bootstrap).  The second forward reuses the LDS rows behind
// gp_forward_tile's leading barrier.
__global__ __launch_bounds__(64) void gm_td_target_kernel(const float* __restrict__ next_state,
                                                          const float* __restrict__ reward,
                                                          const uint8_t* __restrict__ end, int n,
                                                          const float* __restrict__ tparams, GpNet T,
                                                          const float* __restrict__ oparams, GpNet O, float gamma,
                                                          int mask_terminal, float* __restrict__ y,
                                                          float* __restrict__ next_value) {
  __shared__ float act[2][GP_TILE][GP_ROW];
  const int lane = threadIdx.x;
  const int e0 = blockIdx.x * GP_TILE;
  const bool mine = lane < GP_TILE && e0 + lane < n;
  const int n_out = T.width[T.n_layers];
  int a = -1;
  if (oparams) {   // (uniform over the launch)
    const int cur = gp_forward_tile(next_state, nullptr, e0, n, oparams, O, GP_ACT_RELU, act, lane);
    if (mine) a = gp_softmax_argmax(act[cur][lane], n_out, nullptr, nullptr);
  }
  const int cur = gp_forward_tile(next_state, nullptr, e0, n, tparams, T, GP_ACT_RELU, act, lane);
  if (mine) {
    const size_t row = (size_t)(e0 + lane);
    float v;
    float* q = act[cur ^ 1][lane];   // the other buffer's row: the target's softmax
    gp_softmax_argmax(act[cur][lane], n_out, q, &v);
    if (a >= 0) v = q[a];
    if (mask_terminal && end[row] == 1) v = 0.0f;
    if (next_value) next_value[row] = v;
    y[row] = reward[row] + gamma * v;
  }
}
