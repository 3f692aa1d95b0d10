// gm_ac.hip -- the batched PPO actor-critic kernels (gm_ac_act / gm_ac_record / gm_ac_finish)
// and the GAE-lambda scan.  The forward is gm_policy_net.h's gp_forward_tile with each net's
// activation code; sampling is gm_ac_net.h's ga_sample / ga_sample_cat (both shared with
// gm_rollout's per-env driver, gm_rollout.h ac_rollout_driver).
#pragma once
#include "gm_ac_net.h"

// what: 0 gm_ac_act (row k: obs, mu, act, logp, val), 1 gm_ac_record (row k: rew, end, boot),
// 2 gm_ac_finish (last_val).  One wave per 16 envs.
__global__ __launch_bounds__(64) void gm_ac_kernel(int what, const float* __restrict__ obs,
                                                   const GmEnvState* __restrict__ states,
                                                   const float* __restrict__ rew, const uint8_t* __restrict__ done,
                                                   int n_envs, long long env_offset, GaArgs A, int k, int max_ep) {
  __shared__ float act[2][GP_TILE][GP_ROW];
  __shared__ float asamp[GP_TILE][GA_MAX_ACT];
  const int lane = threadIdx.x;
  const int e0 = blockIdx.x * GP_TILE;
  const bool mine = lane < GP_TILE && e0 + lane < n_envs;
  const size_t env = (size_t)(e0 + lane);
  const size_t row = (size_t)k * (size_t)n_envs + env;
  const float* cparams = A.params + A.net.critic_off;
  if (what == 0) {
    const int n_obs = A.net.actor.width[0];
    const int na = A.net.actor.width[A.net.actor.n_layers];
    int cur = gp_forward_tile(obs, A.t_obs + (size_t)k * n_envs * n_obs, e0, n_envs, A.params, A.net.actor,
                              A.net.act_actor, act, lane);
    if (mine && A.net.categorical) {   // logits: the index as a float is the row's one action, the logits go to mu
      const float* x = act[cur][lane];
      A.t_logp[row] = ga_sample_cat(x, na, A.sample, A.seed, A.decision0 + (uint64_t)k,
                                    (uint64_t)(env_offset + (long long)env), asamp[lane]);
      A.t_act[row] = asamp[lane][0];
      if (A.t_idx) A.t_idx[env] = (int)asamp[lane][0];
      if (A.t_mu)
        for (int i = 0; i < na; i++) A.t_mu[row * na + i] = x[i];
    } else if (mine) {
      const float* mu = act[cur][lane];
      A.t_logp[row] = ga_sample(mu, A.params + A.net.log_std_off, na, A.sample, A.noise, A.seed,
                                A.decision0 + (uint64_t)k, (uint64_t)(env_offset + (long long)env), asamp[lane]);
      for (int i = 0; i < na; i++) {
        A.t_act[row * na + i] = asamp[lane][i];
        if (A.t_mu) A.t_mu[row * na + i] = mu[i];
      }
    }
    cur = gp_forward_tile(obs, nullptr, e0, n_envs, cparams, A.net.critic, A.net.act_critic, act, lane);
    if (mine) A.t_val[row] = act[cur][lane][0];
    return;
  }
  if (what == 1) {
    int end = 0;
    if (mine) end = gm_episode_end_code(done[env], states[env].num_action_steps, max_ep);
    float b = 0.0f;
    if (__ballot(end == 2) != 0ull) {   // (wave-uniform) some env of the tile was truncated
      const int cur = gp_forward_tile(obs, nullptr, e0, n_envs, cparams, A.net.critic, A.net.act_critic, act, lane);
      if (end == 2) b = act[cur][lane][0];
    }
    if (mine) {
      A.t_rew[row] = rew[env];
      A.t_end[row] = (uint8_t)end;
      A.t_boot[row] = b;
    }
    return;
  }
  const int cur = gp_forward_tile(obs, nullptr, e0, n_envs, cparams, A.net.critic, A.net.act_critic, act, lane);
  if (mine) A.t_last_val[env] = act[cur][lane][0];
}

// GAE-lambda advantages and rewards-to-go over a trajectory buffer (PPOBuffer.finish_trajectory,
// rl/agents/PolicyGradient.py:355-380, per env and per trajectory segment).  One thread per
// env, scanning k backwards: every load and store is coalesced across envs.
//   next_v = end == 1 ? 0 : end == 2 ? boot[k] : (k == K - 1 ? last_val : val[k + 1])
//   delta  = rew[k] + gamma next_v - val[k]
//   adv[k] = delta + (end ? 0 : gamma lam adv[k + 1])                       (adv[K] = 0)
//   ret[k] = rew[k] + gamma (end == 1 ? 0 : end == 2 ? boot[k] : (k == K - 1 ? last_val : ret[k + 1]))
__global__ __launch_bounds__(64) void gm_ac_gae_kernel(const float* __restrict__ rew, const float* __restrict__ val,
                                                       const uint8_t* __restrict__ end, const float* __restrict__ boot,
                                                       const float* __restrict__ last_val, int n_envs, int K,
                                                       float gamma, float lam, float* __restrict__ adv,
                                                       float* __restrict__ ret) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs) return;
  const float lv = last_val[env];
  float v_next = lv, r_next = lv, a_next = 0.0f;
  for (int k = K - 1; k >= 0; k--) {
    const size_t i = (size_t)k * (size_t)n_envs + (size_t)env;
    const int e = end[i];
    const float r = rew[i], v = val[i];
    const float tail = e == 1 ? 0.0f : boot[i];
    const float nv = e ? tail : v_next;
    const float delta = r + gamma * nv - v;
    const float a = e ? delta : delta + gamma * lam * a_next;
    const float g = r + gamma * (e ? tail : r_next);
    adv[i] = a;
    ret[i] = g;
    v_next = v;
    r_next = g;
    a_next = a;
  }
}
