// gm_ac_net.h -- on-device PPO actor-critic: GaNet / GaArgs, the sampler ga_sample and the
// one-env critic ga_value_one (shared by gm_ac.hip's batched kernels and the rollout driver
// in gm_rollout.h).
//
// Reference: rl/agents/PolicyGradient.py:449-552 MLPGaussianActor / MLPCritic /
// MLPActorCriticPG.step and :1348-1386 Agent_PPO.select_action:
//   mu = mu_net(obs)          mlp([n_obs, *hidden, n_actions], Tanh), identity output layer
//   std = exp(log_std)        log_std a free vector of n_actions
//   a = mu + std z            z ~ N(0, 1)
//   logp = sum_i ( -(a_i - mu_i)^2 / (2 std_i^2) - log_std_i - 0.5 log(2 pi) )
//   v = v_net(obs)            mlp([n_obs, *hidden, 1], Tanh)
// and, with exploration noise > 0, a uniform draw in [-noise, noise) per action added to a
// AFTER logp is taken.  The stored action is the noisy, unclipped one; the env clips it.
//
// Arithmetic and layout are the DQN network's (gm_policy_net.h): f32, v_mfma_f32_16x16x4_f32,
// each net packed by gm_policy_pack's B-fragment layout.  One parameter blob holds
//   [actor net | critic net | log_std[n_actions]]
// (GaNet::critic_off / log_std_off, in floats).  The forward itself is gm_policy_net.h's
// (gp_forward_tile in gm_ac_kernel, gp_forward_one in the rollout driver), called with each
// net's hidden activation code (GaNet::act_*); the DQN passes GP_ACT_RELU as a constant.
//
// Random draws.  Counter-based, keyed by (seed, global env id, decision index, action index),
// so they depend neither on sharding nor on which wave runs the env:
//   h   = gp_mix(seed ^ gp_mix(gid * 0x100000001B3 + decision))      (the eps-greedy key)
//   c_j = gp_mix(h + 3 i + j)   for action i, j = 1, 2, 3            (64-bit wrap-around)
//   u1 = ((c_1 >> 40) + 1) / 2^24   in (0, 1]      u2 = (c_2 >> 40) / 2^24   in [0, 1)
//   z  = sqrt(-2 log(u1)) cos(2 pi u2)                                (Box-Muller)
//   u3 = (c_3 >> 40) / 2^24,  noise draw = noise (2 u3 - 1)           in [-noise, noise)
// gmx/ppo.py normal_draws / noise_draws mirror this in float64.
//
// The categorical actor (MLPCategoricalActor, rl/agents/PolicyGradient.py:429-447, built by
// MLPActorCriticPG(continous_actions=False)): the same MLP with its outputs read as logits,
//   pi = Categorical(logits = logits_net(obs)),  a ~ pi,  logp = pi.log_prob(a)
// and no log_std: the blob is [actor net | critic net] (GaNet::categorical, log_std_off then
// the blob's end).  ga_sample_cat has the arithmetic; its one uniform per env is
//   u = (gp_mix(h + 1) >> 40) / 2^24   in [0, 1)          (gmx/ppo.py categorical_uniforms)
// and the action is the inverse CDF of the unnormalised e_j = exp(x_j - max x) at u * sum e.
#pragma once
#include "gm_policy_net.h"

#define GA_MAX_ACT 40                     // n_actions the sampler's LDS rows hold
#define GA_ONE_FLOATS (2 * GP_ROW + GA_MAX_ACT)   // the one-env driver's LDS scratch, in floats

struct GaNet {
  GpNet actor, critic;
  int act_actor, act_critic;    // hidden activation codes (GP_ACT_*)
  long long critic_off;         // float offset of the critic's packed net in the blob
  long long log_std_off;        // and of log_std
  int categorical;              // the actor's outputs are logits; no log_std (log_std_off: the blob's end)
};

// one rollout launch's (or per-step call's) arguments; the trajectory pointers are indexed
// [k][env] with n_envs envs per step (include/gripper_mi355x.h gm_ac_traj)
struct GaArgs {
  GaNet net;
  const float* params;
  float* t_obs; float* t_act; float* t_logp; float* t_val; float* t_rew; uint8_t* t_end; float* t_boot;
  float* t_last_val; float* t_mu;
  int32_t* t_idx;               // categorical gm_ac_act: the chosen index per env for the discrete-action path, or NULL
  int sample;                   // 0: a = mu (categorical: the argmax)
  float noise;
  uint64_t seed, decision0;     // env-step k of the launch draws with decision0 + k
  int one_row, pad;             // != 0 (gm_ac_evaluate): every env-step of the launch writes trajectory row 0
};

// Sampling and log-probability for ONE env on ONE lane (the batched kernel and the rollout
// driver both call this, never a copy of it, so a and logp are bit for bit the same for the
// same mu).  mu, a: n_act floats; returns logp.
__device__ __noinline__ float ga_sample(const float* mu, const float* __restrict__ log_std, int n_act, int sample,
                                        float noise, uint64_t seed, uint64_t decision, uint64_t gid, float* a) {
  const uint64_t h = gp_mix(seed ^ gp_mix(gid * 0x100000001B3ull + decision));
  float logp = 0.0f;
  for (int i = 0; i < n_act; i++) {
    const float ls = log_std[i];
    const float sd = expf(ls);
    const float m = mu[i];
    float ai = m;
    if (sample) {
      const uint64_t c1 = gp_mix(h + 3ull * (uint64_t)i + 1ull), c2 = gp_mix(h + 3ull * (uint64_t)i + 2ull);
      const float u1 = (float)((double)((c1 >> 40) + 1ull) * (1.0 / 16777216.0));
      const float u2 = (float)((double)(c2 >> 40) * (1.0 / 16777216.0));
      const float z = sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
      ai = m + sd * z;
    }
    const float d = ai - m;
    logp += -(d * d) / (2.0f * (sd * sd)) - ls - 0.91893853320467274178f;
    if (noise > 0.0f) {
      const uint64_t c3 = gp_mix(h + 3ull * (uint64_t)i + 3ull);
      const float u3 = (float)((double)(c3 >> 40) * (1.0 / 16777216.0));
      ai = ai + noise * (2.0f * u3 - 1.0f);
    }
    a[i] = ai;
  }
  return logp;
}

// The categorical actor's draw and log-probability for ONE env on ONE lane (as ga_sample: the
// batched kernel and the rollout driver call this one function).  x: n logits.  In f32, in this order:
//   m = max_j x_j;  e_j = expf(x_j - m);  s = sum_j e_j in index order;  lse = m + logf(s)
//   logp_j = x_j - lse     (never logf(p_j): a p_j that underflows to 0 keeps a finite logp_j)
//   t = u s;  a = the first j whose running sum of e exceeds t, else the last j with e_j > 0
// (no division; the running sum is s's own, so it ends at s > t unless u s rounds up to s).
// sample == 0: the argmax, the lowest index on a tie.  Returns logp_a; *idx = the index a in
// [0, n) as a float, as the trajectory stores it (a caller's row, like ga_sample's a: a pointer to
// a local would cost the batched kernel a stack slot).
__device__ __noinline__ float ga_sample_cat(const float* x, int n, int sample, uint64_t seed, uint64_t decision,
                                            uint64_t gid, float* idx) {
  float m = x[0];
  int a = 0;
  for (int j = 1; j < n; j++)
    if (x[j] > m) { m = x[j]; a = j; }
  float s = 0.0f;
  for (int j = 0; j < n; j++) s += expf(x[j] - m);
  const float lse = m + logf(s);
  if (sample) {
    const uint64_t h = gp_mix(seed ^ gp_mix(gid * 0x100000001B3ull + decision));
    const uint64_t c = gp_mix(h + 1ull);
    const float u = (float)((double)(c >> 40) * (1.0 / 16777216.0));
    const float t = u * s;
    float run = 0.0f;
    int last = 0;
    a = -1;
    for (int j = 0; j < n && a < 0; j++) {
      const float e = expf(x[j] - m);
      if (e > 0.0f) last = j;
      run += e;
      if (run > t) a = j;
    }
    if (a < 0) a = last;
  }
  *idx = (float)a;
  return x[a] - lse;
}

// The critic alone for one env (gm_ac_record's bootstrap value, gm_ac_finish's last value).
__device__ __forceinline__ float ga_value_one(const float* obs, const GaArgs& A, float* act, int lane) {
  const int cur = gp_forward_one(obs, nullptr, A.params + A.net.critic_off, A.net.critic, A.net.act_critic, act, lane);
  return act[cur * GP_ROW];
}
