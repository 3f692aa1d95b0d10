// gm_sac_net.h -- on-device SAC collection side: GsNet / GsArgs, the squashed-Gaussian sampler
// gs_sample and the memory's device view GsReplay (shared by gm_sac.hip's batched kernels and the
// rollout driver in gm_rollout.h).
//
// Reference: rl/agents/ActorCritic.py SquashedGaussianMLPActor / MLPQFunction / MLPActorCriticAC
// and Agent_SAC.select_action:
//   h = mlp([n_obs, *hidden], act, act)(obs)      the activation follows every hidden Linear
//   mu = mu_layer(h)   log_std = clamp(log_std_layer(h), log_std_min, log_std_max)
//   u = mu + exp(log_std) z,  z ~ N(0, 1)         (u = mu when deterministic)
//   logp = sum_i Normal(mu, std).log_prob(u)_i - sum_i 2 (log 2 - u_i - softplus(-2 u_i))
//   a = action_limit tanh(u)
//   q_j = mlp([n_obs + n_actions, *hidden, 1], act)(cat(obs, a)),  j = 1, 2
// and, while the agent is still in its random start, a_i = 2 U[0, 1) - 1 with no net at all.
//
// The actor is ONE MLP of sizes [n_obs, *hidden, 2 n_actions]: its identity output layer is
// mu_layer stacked over log_std_layer, so the head row is [mu | log_std] and the forward is
// gm_policy_net.h's (gp_forward_tile / gp_forward_one) unchanged.  One parameter blob holds
//   [pi | q1 | q2]
// each in gm_policy_pack's B-fragment layout (GsNet::q1_off / q2_off, in floats); the two critics
// have the same sizes and share one GpNet.
//
// Random draws: gm_ac_net.h's counters, keyed by (seed, global env id, decision, action index):
// c_1 and c_2 feed Box-Muller for z; c_3's u3 gives the uniform action 2 u3 - 1 (exact in f32:
// u3 has 24 bits).  gmx/sac.py normal_draws / uniform_action_draws mirror them in float64.
#pragma once
#include "gm_ac_net.h"

#define GM_SAC_MEAN 0      // u = mu
#define GM_SAC_SAMPLE 1    // u = mu + std z
#define GM_SAC_RANDOM 2    // a = 2 u3 - 1, the net is not consulted; u, logp (mu, log_std) are written as 0

struct GsNet {
  GpNet pi, q;                 // pi: [n_obs, *hidden, 2 n_act]; q: both critics' [n_obs + n_act, *hidden, 1]
  int act;                     // hidden activation code (GP_ACT_*), all three nets
  int n_act;
  long long q1_off, q2_off;    // float offsets of the critics' packed nets in the blob
  float limit, ls_min, ls_max; // action_limit and the log_std clamp
  int pad;
};

// The device view of a caller's gm_sac_replay and the ring position of a call (gm_replay.h's
// rules: gr_row).  The second half of a push needs no action, so it goes through gm_replay.h's
// GrArgs with a NULL action (gm_replay_push_end_kernel, replay_record phase 1).
struct GsReplay {
  float* state;                // [capacity][n_obs]
  float* action;               // [capacity][n_act]
  long long capacity, row0;
};

// one rollout launch's arguments (GmRolloutJob::sac points at a device copy)
struct GsArgs {
  GsNet net;
  const float* params;
  GsReplay rep;                // rep.state == NULL: nothing is recorded
  int mode, pad;
  uint64_t seed, decision0;    // env-step k of the launch draws with decision0 + k
};

// softplus(x) = log(1 + exp(x)), the stable form: no overflow for large x, no cancellation for
// very negative x
__device__ __forceinline__ float gs_softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }

// Sampling, squashing and log-probability for ONE env on ONE lane (the batched kernel and the
// rollout driver both call this, never a copy of it, so a, u and logp are bit for bit the same
// for the same head row).  head: [mu[n_act] | log_std[n_act]] as the actor's last layer left
// them (not read in GM_SAC_RANDOM); a, u: n_act floats each; ls (may be NULL): the clamped
// log_std.  Returns logp.  The tanh correction is taken from u, never from 1 - a^2, so logp stays
// finite where tanh(u) rounds to +-1.
__device__ __noinline__ float gs_sample(const float* head, int n_act, int mode, float limit, float ls_min,
                                        float ls_max, uint64_t seed, uint64_t decision, uint64_t gid, float* a,
                                        float* u, float* ls_out) {
  const uint64_t h = gp_mix(seed ^ gp_mix(gid * 0x100000001B3ull + decision));
  if (mode == GM_SAC_RANDOM) {
    for (int i = 0; i < n_act; i++) {
      const uint64_t c3 = gp_mix(h + 3ull * (uint64_t)i + 3ull);
      const float u3 = (float)((double)(c3 >> 40) * (1.0 / 16777216.0));
      a[i] = 2.0f * u3 - 1.0f;
      u[i] = 0.0f;
      if (ls_out) ls_out[i] = 0.0f;
    }
    return 0.0f;
  }
  float lp = 0.0f, corr = 0.0f;
  for (int i = 0; i < n_act; i++) {
    const float ls = fminf(fmaxf(head[n_act + i], ls_min), ls_max);
    const float sd = expf(ls);
    const float m = head[i];
    float ui = m;
    if (mode == GM_SAC_SAMPLE) {
      const uint64_t c1 = gp_mix(h + 3ull * (uint64_t)i + 1ull), c2 = gp_mix(h + 3ull * (uint64_t)i + 2ull);
      const float u1 = (float)((double)((c1 >> 40) + 1ull) * (1.0 / 16777216.0));
      const float u2 = (float)((double)(c2 >> 40) * (1.0 / 16777216.0));
      const float z = sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
      ui = m + sd * z;
    }
    const float d = ui - m;
    lp += -(d * d) / (2.0f * (sd * sd)) - ls - 0.91893853320467274178f;
    corr += 2.0f * (0.69314718055994530942f - ui - gs_softplus(-2.0f * ui));
    a[i] = limit * tanhf(ui);
    u[i] = ui;
    if (ls_out) ls_out[i] = ls;
  }
  return lp - corr;
}
