// gm_sac_learn.h -- what the SAC learner's kernels (gm_sac_learn.hip) and its host side
// (gm_capi.hip) share: the launch arguments, where a tile's rows live and the walk between
// MLPActorCriticAC's flat parameter order and the blob's device order.
//
// Reference: rl/agents/ActorCritic.py:396-500 (Agent_SAC.compute_loss_q, compute_loss_pi,
// optimise_model).  As on the DQN and PPO sides (gm_learn.h, gm_ppo_learn.h) gradients and moments
// live in the packed layout, here gm_sac_net.h's blob
//   [pi | q1 | q2]
// and the steps update gm_sac's d_params in place; nothing is repacked.  q_optimiser owns the
// contiguous range [q1 | q2], pi_optimiser the range [pi] (DESIGN.md "SAC learner": the AdamW
// owner reading).  Padding entries stay 0 by gm_learn.h's argument.
//
// Tiles.  A batch of n <= GL_MAX_BATCH rows is ceil(n / 16) tiles of 16 rows, one wave each.
//   critic loss   grid (tiles, 2): workgroup (t, j) runs critic j on tile t and writes its share of
//                 the gradient to part_q[t][j's range of [q1 | q2]] and its loss sum to tile_loss
//   actor loss    grid (tiles): workgroup t runs the actor, both critics and the way back through
//                 them on tile t and writes part_pi[t][pi's packed count] and its loss sum
// gm_learn_step_kernel then adds the tiles in tile order.  No float atomic, no workgroup waits for
// another: the same inputs give the same bytes.
//
// Rows.  The critic-loss workgroup keeps one critic's plan (GlPlan of GsNet::q); the actor-loss
// workgroup keeps three, [actor | q1 | q2], at gsl_pi_rows' offsets.  Each set lives in LDS where
// it fits GL_ARENA and else in the learner's global spill.
#pragma once
#include "gm_learn.h"
#include "gm_sac_net.h"

// one launch of gm_sac_grad_q_kernel
struct GslQArgs {
  const float* state;           // [n][n_obs]
  const float* action;          // [n][n_act]
  const float* y;               // [n] the backup
  int n, pad;
  const float* params;          // the blob
  GsNet net;
  GlPlan plan;                  // the critics' row plan
  float* spill;                 // [tiles][2][plan.total] where the plan does not fit GL_ARENA
  float* partials;              // [tiles][2 x q's packed count]: [q1 | q2] in packed order
  long long q_total;            // one critic's packed count
  float* tile_loss;             // [2][GL_MAX_TILES]: critic j's loss sum of tile t at [j * GL_MAX_TILES + t]
};

// one launch of gm_sac_grad_pi_kernel
struct GslPiArgs {
  const float* state;           // [n][n_obs]
  int n, pad;
  const float* params;          // the blob (the critics as q_optimiser's step left them)
  GsNet net;
  GlPlan plan_pi, plan_q;
  float* spill;                 // [tiles][gsl_pi_rows] where the three plans do not fit GL_ARENA
  float* partials;              // [tiles][pi's packed count]
  long long pi_total;
  float* tile_loss;             // [GL_MAX_TILES]
  float alpha;
  uint64_t seed, draw;          // row i draws with (seed, i, draw): gs_sample's counters
  // optional debug outputs (NULL: not written)
  float* z;                     // [n][n_act] the standard normal draws
  float* u;                     // [n][n_act] the pre-squash sample
  float* a;                     // [n][n_act] the squashed action
  float* logp;                  // [n]
  float* q1;                    // [n] both critics on (state, a)
  float* q2;
};

// the actor-loss workgroup's rows: [actor's plan | q1's | q2's], in floats
__host__ __device__ inline long long gsl_pi_rows(const GlPlan& Lpi, const GlPlan& Lq) {
  return (long long)Lpi.total + 2ll * Lq.total;
}

// ---- host: the flat <-> packed walk.  Flat is MLPActorCriticAC's parameters() order: the actor's
// hidden layers, mu_layer.W, mu_layer.b, log_std_layer.W, log_std_layer.b, q1's layers, q2's; the
// packed actor is ONE net whose output layer is mu_layer stacked over log_std_layer.
inline int64_t gsl_flat_count(const GsNet& N) { return gl_flat_count(N.pi) + 2 * gl_flat_count(N.q); }
template <class F>
inline void gsl_for_each_param(const GsNet& N, F f) {   // f(flat index, packed index)
  const GpNet& P = N.pi;
  const int L = P.n_layers, na = N.n_act;
  GpNet hidden = P;
  hidden.n_layers = L - 1;
  gl_for_each_param(hidden, [&](int64_t i, int64_t k) { f(i, k); });
  int64_t i = gl_flat_count(hidden);
  const int in = P.width[L - 1], ks = P.kpad[L - 1] / 4;
  for (int head = 0; head < 2; head++) {              // mu_layer: output rows 0 .. na - 1; log_std_layer: na .. 2 na - 1
    for (int r = 0; r < na; r++) {
      const int j = head * na + r;
      for (int k = 0; k < in; k++)
        f(i++, (int64_t)P.woff[L - 1] + ((int64_t)(j >> 4) * ks + (k >> 2)) * 64 + (k & 3) * 16 + (j & 15));
    }
    for (int r = 0; r < na; r++) f(i++, (int64_t)P.boff[L - 1] + head * na + r);
  }
  const int64_t fp = i, fq = gl_flat_count(N.q);
  gl_for_each_param(N.q, [&](int64_t ii, int64_t k) { f(fp + ii, (int64_t)N.q1_off + k); });
  gl_for_each_param(N.q, [&](int64_t ii, int64_t k) { f(fp + fq + ii, (int64_t)N.q2_off + k); });
}
// packed [total] -> flat [gsl_flat_count], and back (padding entries 0)
inline void gsl_unpack(const GsNet& N, const float* packed, float* flat) {
  gsl_for_each_param(N, [&](int64_t i, int64_t k) { flat[i] = packed[k]; });
}
inline void gsl_pack(const GsNet& N, int64_t total, const float* flat, float* packed) {
  for (int64_t k = 0; k < total; k++) packed[k] = 0.0f;
  gsl_for_each_param(N, [&](int64_t i, int64_t k) { packed[k] = flat[i]; });
}
