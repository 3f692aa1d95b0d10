// gm_sac.hip -- the batched SAC kernels: the squashed actor on 16 rows per wave (gm_sac_act and
// gm_sac_target's first launch), the first half of a push with its float action row
// (gm_sac_push_begin; the second half is gm_replay.hip's, which needs no action), the gather of a
// sampled batch (gm_sac_replay_sample) and both critics with the soft Bellman backup (gm_sac_q,
// gm_sac_target's second launch).  The forwards are gm_policy_net.h's, the sampler gm_sac_net.h's
// gs_sample (shared with gm_rollout.h sac_rollout_driver), ring rule and draw gm_replay.h's.
#pragma once
#include "gm_state.h"
#include "gm_replay.h"
#include "gm_sac_net.h"

// what the actor kernel writes, each [n][...] and each optional (NULL: not written)
struct GsActOut {
  float* act;      // [n][n_act] the squashed action
  float* logp;     // [n]
  float* u;        // [n][n_act] the pre-squash sample
  float* mu;       // [n][n_act]
  float* ls;       // [n][n_act] the clamped log_std
};

// SquashedGaussianMLPActor.forward on rows e0 .. e0 + 15 of obs[n][n_obs], one wave per 16 rows;
// row i draws with id id0 + i.  GM_SAC_RANDOM skips the forward (uniform over the launch).
__global__ __launch_bounds__(64) void gm_sac_actor_kernel(const float* __restrict__ obs, int n, long long id0,
                                                          const float* __restrict__ params, GsNet N, int mode,
                                                          uint64_t seed, uint64_t decision, GsActOut out) {
  __shared__ float act[2][GP_TILE][GP_ROW];
  __shared__ float samp[GP_TILE][2 * GA_MAX_ACT];
  __shared__ float lsr[GP_TILE][GA_MAX_ACT];
  const int lane = threadIdx.x;
  const int e0 = blockIdx.x * GP_TILE;
  const bool mine = lane < GP_TILE && e0 + lane < n;
  const int na = N.n_act;
  int cur = 0;
  if (mode != GM_SAC_RANDOM) cur = gp_forward_tile(obs, nullptr, e0, n, params, N.pi, N.act, act, lane);
  if (!mine) return;
  const size_t row = (size_t)(e0 + lane);
  const float* head = act[cur][lane];
  float* a = samp[lane];
  float* u = samp[lane] + GA_MAX_ACT;
  const float logp = gs_sample(head, na, mode, N.limit, N.ls_min, N.ls_max, seed, decision,
                               (uint64_t)(id0 + (long long)row), a, u, lsr[lane]);
  if (out.logp) out.logp[row] = logp;
  for (int i = 0; i < na; i++) {
    if (out.act) out.act[row * na + i] = a[i];
    if (out.u) out.u[row * na + i] = u[i];
    if (out.mu) out.mu[row * na + i] = mode == GM_SAC_RANDOM ? 0.0f : head[i];
    if (out.ls) out.ls[row * na + i] = lsr[lane][i];
  }
}

// ReplayMemory.push, first half (after gm_sac_act): state and the squashed action row of every
// env into its ring row.  One thread per observation element; the threads of a row share its
// action elements among them.
__global__ __launch_bounds__(256) void gm_sac_push_begin_kernel(const float* __restrict__ obs,
                                                                const float* __restrict__ actions, int n_envs,
                                                                int n_obs, int n_act, GsReplay R) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n_envs * n_obs) return;
  const int env = (int)(i / n_obs), j = (int)(i - (long long)env * n_obs);
  const size_t row = (size_t)gr_row(R.row0, 0, n_envs, env, R.capacity);
  R.state[row * (size_t)n_obs + j] = obs[i];
  for (int k = j; k < n_act; k += n_obs) R.action[row * (size_t)n_act + k] = actions[(size_t)env * n_act + k];
}

// ReplayMemory.batch with float action rows: row b of the batch is ring row gr_index(size, key,
// b), as gm_replay_sample_kernel's.  One thread per observation element.
__global__ __launch_bounds__(256) void gm_sac_replay_sample_kernel(gm_sac_replay R, int n_obs, int n_act,
                                                                   long long size, int batch, uint64_t key,
                                                                   gm_sac_batch out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)batch * n_obs) return;
  const int b = (int)(i / n_obs), j = (int)(i - (long long)b * n_obs);
  const size_t row = (size_t)gr_index((uint64_t)size, key, (uint64_t)b);
  out.state[i] = R.state[row * (size_t)n_obs + j];
  out.next_state[i] = R.next_state[row * (size_t)n_obs + j];
  for (int k = j; k < n_act; k += n_obs) out.action[(size_t)b * n_act + k] = R.action[row * (size_t)n_act + k];
  if (j == 0) {
    out.reward[b] = R.reward[row];
    out.end[b] = R.end[row];
    out.index[b] = (int32_t)row;
  }
}

// the soft Bellman backup's inputs and outputs (y == NULL: the kernel only evaluates the critics)
struct GsBackup {
  const float* reward;    // [n]
  const uint8_t* end;     // [n]
  const float* logp2;     // [n]
  float gamma, alpha;
  int bootstrap_truncated, pad;
  float* y;               // [n]
  float* qmin;            // [n] (may be NULL)
};

// rows e0 .. e0 + 15 of cat(state, action) straight into the LDS activation rows gp_layers_tile
// reads, zero beyond n and beyond the input width (the leading barrier: every lane has read the
// previous net's outputs)
__device__ __forceinline__ void gs_q_rows(const float* __restrict__ state, const float* __restrict__ action, int e0,
                                          int n, int n_obs, int n_act, int k0, float (*act)[GP_TILE][GP_ROW],
                                          int lane) {
  __syncthreads();
  for (int i = lane; i < GP_TILE * k0; i += 64) {
    const int r = i / k0, k = i - r * k0;
    float v = 0.0f;
    if (e0 + r < n) {
      if (k < n_obs) v = state[(size_t)(e0 + r) * n_obs + k];
      else if (k < n_obs + n_act) v = action[(size_t)(e0 + r) * n_act + (k - n_obs)];
    }
    act[0][r][k] = v;
  }
}

// MLPQFunction x 2 on n rows, one wave per 16 rows: q1, q2 (each may be NULL) and, with B.y, the
// backup of compute_loss_q:  y = reward + gamma (min(q1, q2) - alpha logp2)  where the row
// bootstraps (end == 0, or end == 2 with bootstrap_truncated), y = reward exactly where not.
__global__ __launch_bounds__(64) void gm_sac_q_kernel(const float* __restrict__ state,
                                                      const float* __restrict__ action, int n,
                                                      const float* __restrict__ params, GsNet N,
                                                      float* __restrict__ q1, float* __restrict__ q2, GsBackup B) {
  __shared__ float act[2][GP_TILE][GP_ROW];
  const int lane = threadIdx.x;
  const int e0 = blockIdx.x * GP_TILE;
  const bool mine = lane < GP_TILE && e0 + lane < n;
  const int n_obs = N.pi.width[0];
  gs_q_rows(state, action, e0, n, n_obs, N.n_act, N.q.kpad[0], act, lane);
  int cur = gp_layers_tile(params + N.q1_off, N.q, N.act, act, lane);
  const float v1 = act[cur][lane & 15][0];
  gs_q_rows(state, action, e0, n, n_obs, N.n_act, N.q.kpad[0], act, lane);
  cur = gp_layers_tile(params + N.q2_off, N.q, N.act, act, lane);
  const float v2 = act[cur][lane & 15][0];
  if (!mine) return;
  const size_t row = (size_t)(e0 + lane);
  if (q1) q1[row] = v1;
  if (q2) q2[row] = v2;
  if (B.y) {
    const float qm = fminf(v1, v2);
    const int e = B.end[row];
    const bool boots = e == 0 || (e == 2 && B.bootstrap_truncated);
    const float r = B.reward[row];
    if (B.qmin) B.qmin[row] = qm;
    B.y[row] = boots ? r + B.gamma * (qm - B.alpha * B.logp2[row]) : r;
  }
}
