// gm_ppo_learn.h -- what the PPO learner's kernels (gm_ppo_learn.hip) and its host side
// (gm_capi.hip) share: the launch arguments, the blob's layout and the walk between gm_ac_create's
// flat parameter order and gm_ac_pack's device order.
//
// Reference: rl/agents/PolicyGradient.py:1440-1522 (Agent_PPO.compute_loss_v, compute_loss_pi,
// optimise_model) and :384-407 (PPOBuffer.get's advantage normalisation).  As on the DQN side
// (gm_learn.h) gradients and moments live in the packed layout, here the blob
//   [actor net | critic net | log_std[n_actions]]
// the steps update gm_ac's d_params in place and nothing is repacked.  Padding entries stay 0 by
// gm_learn.h's argument: a padding weight's activation column or delta column is 0, so its
// gradient is 0, and 0 stays 0 under Adam and AdamW (log_std has no padding).  A categorical
// actor's blob (GaNet::categorical) is [actor net | critic net]: log_std has no entries, in the
// blob, the flat order, either optimiser's range or the state calls.
//
// Tiles and workgroups.  A batch of n rows is ceil(n / 16) tiles of 16 rows.  A learner has a
// fixed number G of workgroups; workgroup g takes tiles g, g + G, g + 2 G, ... in that order and
// keeps the running sum of their gradients (the first tile stores, every later one adds: each entry
// is read and written by the same lane every time) in LDS behind the rows where the packed net
// fits there (gq_lds_part; written to partials[g] once at the end) and else in place in its own
// partials[g][blob floats]; its loss and info sums go to wg_info[g].  The reduce kernel adds
// partials 0 .. min(G, tiles) - 1 in that order.  No float atomic, no workgroup waits for another:
// the same inputs with the same G give the same bytes.
#pragma once
#include "gm_learn.h"
#include "gm_ac_net.h"

#define GQ_DEFAULT_GROUPS 512   // profiles/ppo_learn.json: the G sweep at n = 40,960, (64, 64) nets
#define GQ_MAX_GROUPS 4096
#define GQ_LDS_FLOATS 16320     // floats of dynamic LDS a gradient workgroup may take (64 KB less the static rows)
#define GQ_INFO 4               // floats of wg_info per workgroup: loss sum, kl sum, clipped rows, entropy sum (categorical)
// gq_grad's instantiations: the critic, the Gaussian policy, the categorical policy
#define GQ_VF 0
#define GQ_PI 1
#define GQ_CAT 2

// one launch of gm_ppo_grad_pi_kernel / gm_ppo_grad_vf_kernel
struct GqGradArgs {
  const float* obs;             // [n][n_obs]
  const float* act;             // [n][n_act]     (actor; categorical: [n][1], the index as a float)
  const float* logp_old;        // [n]            (actor)
  const float* adv;             // [n]            (actor)
  const float* ret;             // [n]            (critic)
  long long n;
  const float* params;          // the blob
  GpNet net;                    // the actor's or the critic's
  GlPlan plan;                  // its row plan
  long long net_off;            // the net's float offset in the blob
  long long net_total;          // and its packed float count
  int lds_part;                 // the workgroup's partial of this net lives in LDS behind the rows (gq_lds_part)
  long long log_std_off;
  int n_groups;
  int use_kl;                   // the KL-penalty loss instead of the clipped surrogate
  float clip_lo, clip_hi;       // 1 - eps, 1 + eps, each rounded from double as torch does
  float beta;                   // kl_penalty_coefficient
  float* spill;                 // [n_groups][spill_stride] rows that do not fit LDS
  long long spill_stride;
  float* partials;              // [n_groups][total]
  long long total;              // blob floats
  float* wg_info;               // [n_groups][GQ_INFO]
  const int* stop;              // NULL, or the KL stop's latch: nonzero makes the launch a no-op
  int use_ent;                  // (categorical) the entropy term's gradient goes into the output deltas
  float c_ent;                  // entropy_coefficient
};

// gm_ppo_learner_read's / gm_ppo_info's scalar order
#define GQ_LOSS_PI 0
#define GQ_LOSS_V 1
#define GQ_KL 2
#define GQ_ENT 3
#define GQ_CF 4
#define GQ_SCALARS 5

// one launch of gm_ppo_reduce_kernel: grad[e] = sum over the partials, in order, for the `count`
// elements of one optimiser: e = first + i, and gap_len further on from i >= gap_at (the policy's
// [actor | log_std] around the critic); thread 0 forms the mean loss and the info scalars
struct GqReduceArgs {
  const float* partials;
  long long total;
  int n_parts;                  // min(G, tiles)
  long long count, first, gap_at, gap_len;
  float* grad;                  // [total]
  const float* wg_info;
  long long n;
  int policy;                   // 1: loss_pi, kl, ent, cf and the stop; 0: loss_v
  int use_kl, use_ent;
  float beta, c_ent;
  const float* params;
  long long log_std_off;
  int n_act;
  float* scalars;               // [GQ_SCALARS]
  float* first_out;             // [GQ_SCALARS] or NULL: gm_ppo_learner_update's first iteration
  float* last_out;              // [GQ_SCALARS] or NULL: and its last one
  int* stop;                    // NULL: no stop; else [0] the latch, [1] policy iterations that stepped
  double kl_stop;               // max_kl_ratio * target_kl
  int categorical;              // ent = wg_info's fourth sum / n, and no log_std term
};

// the rows of the plan stay in LDS and the net's packed partial fits behind them
inline bool gq_lds_part(const GlPlan& L, long long net_total) {
  return L.total <= GL_ARENA && (long long)L.total + net_total <= GQ_LDS_FLOATS;
}

// ---- host: layout and the flat <-> packed walk
inline int64_t gq_layout(const int32_t* asz, int na, const int32_t* csz, int nc, GaNet* net, int64_t* n_raw,
                         int categorical = 0) {
  GaNet N{};
  const int64_t ta = gl_layout(asz, na, &N.actor);
  const int64_t tc = gl_layout(csz, nc, &N.critic);
  if (ta < 0 || tc < 0) return -1;
  N.act_actor = N.act_critic = GP_ACT_TANH;
  N.critic_off = ta;
  N.log_std_off = ta + tc;
  N.categorical = categorical != 0;
  const int n_ls = categorical ? 0 : asz[na - 1];
  if (net) *net = N;
  if (n_raw) *n_raw = gl_flat_count(N.actor) + gl_flat_count(N.critic) + n_ls;
  return ta + tc + n_ls;
}
template <class F>
inline void gq_for_each_param(const GaNet& N, F f) {   // f(flat index, packed index)
  const int64_t fa = gl_flat_count(N.actor), fc = gl_flat_count(N.critic);
  gl_for_each_param(N.actor, [&](int64_t i, int64_t k) { f(i, k); });
  gl_for_each_param(N.critic, [&](int64_t i, int64_t k) { f(fa + i, (int64_t)N.critic_off + k); });
  const int n_act = N.categorical ? 0 : N.actor.width[N.actor.n_layers];
  for (int i = 0; i < n_act; i++) f(fa + fc + i, (int64_t)N.log_std_off + i);
}
// packed [total] -> flat [n_raw], and back (padding entries 0)
inline void gq_unpack(const GaNet& N, const float* packed, float* flat) {
  gq_for_each_param(N, [&](int64_t i, int64_t k) { flat[i] = packed[k]; });
}
inline void gq_pack(const GaNet& N, int64_t total, const float* flat, float* packed) {
  for (int64_t k = 0; k < total; k++) packed[k] = 0.0f;
  gq_for_each_param(N, [&](int64_t i, int64_t k) { packed[k] = flat[i]; });
}
