// gm_policy_net.h -- the on-device MLP (network layout and the only two MFMA forwards,
// gp_forward_tile for 16 envs per wave and gp_forward_one for one env on its own wave) and the
// DQN action selection on top of it ("fused on-device DQN inference").
// The DQN callers (gm_policy_kernel, gp_select_one) pass GP_ACT_RELU as a constant; the PPO
// actor-critic (gm_ac_net.h, gm_ac.hip, ac_rollout_driver) and SAC (gm_sac_net.h, gm_sac.hip,
// sac_rollout_driver) pass each net's run-time code.  gp_forward_tile is its load of the rows
// followed by gp_layers_tile, which the SAC critics call on rows they assemble themselves.
//
// Reference: rl/networks.py:7-41 VariableNetwork.forward (Linear + ReLU per hidden
// layer, a final Linear, Softmax over dim 1) and rl/agents/DQN.py:184-209
// Agent_DQN.select_action (a uniform random action with probability eps_threshold,
// otherwise policy_net(state).max(1)[1]).  The canonical network is
// [n_obs = 63, 150, 100, 50, n_actions = 8] (launch_training.py:850-857).
//
// f32 throughout (torch's default dtype).  The layer products run on the f32-input MFMA
// v_mfma_f32_16x16x4_f32, whose result is bit-for-bit a k-ordered fmaf chain.  One wave
// handles a tile of 16 envs: activations live in LDS as [16 envs][width] f32 (ping-pong
// between layers); weights are repacked on the host into B-fragment order -- for each
// 16-output tile and 4-wide k step, 64 floats in lane order (lane l holds
// W[16 t + (l & 15)][4 s + (l >> 4)]) -- so every MFMA's B operand is one coalesced
// 256-byte load from L2 (the canonical network is 119 KB).  Zero padding in k and in
// the output tiles keeps every lane's arithmetic defined.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#define GP_MAX_LAYERS 8
#define GP_MAX_WIDTH 256
#define GP_TILE 16
#define GP_ROW (GP_MAX_WIDTH + 4)   // floats per activation row in LDS
#define GP_ACT_RELU 0               // hidden activation codes
#define GP_ACT_TANH 1

struct GpNet {
  int n_layers;                   // Linear layers
  int width[GP_MAX_LAYERS + 1];   // layer sizes: width[0] = n_obs, width[n_layers] = n_actions
  int kpad[GP_MAX_LAYERS];        // width[l] rounded up to 4 (MFMA k step)
  int tiles[GP_MAX_LAYERS];       // ceil(width[l + 1] / 16)
  long long woff[GP_MAX_LAYERS];  // float offset of layer l's packed weights
  long long boff[GP_MAX_LAYERS];  // float offset of layer l's bias (padded to tiles * 16)
};

typedef float gp_f32x4 __attribute__((ext_vector_type(4)));

// counter-based uniform in [0, 1) and integer draws for epsilon-greedy: splitmix64 of
// (seed, global env id, decision index) -- one independent stream per env, so actions do
// not depend on how envs are sharded (the reference draws from one numpy Generator per
// agent, which a batched device policy cannot reproduce draw for draw); also the host's
// (gm_replay_indices)
__host__ __device__ __forceinline__ uint64_t gp_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the hidden activation; a caller's literal code folds the other branch away
__device__ __forceinline__ float gp_activate(float v, int code) {
  return code == GP_ACT_TANH ? tanhf(v) : fmaxf(v, 0.0f);
}

// softmax over the logits (nn.Softmax(dim=1)) and its argmax (first maximum, like torch's max
// on CPU).  One lane, one row; q_out (may be NULL) gets the softmax, qbest_out (may be NULL)
// its maximum.  Shared by select_action (gp_choose) and the TD target (gm_replay.hip).
__device__ __forceinline__ int gp_softmax_argmax(const float* x, int n_out, float* q_out, float* qbest_out) {
  float m = x[0];
  for (int j = 1; j < n_out; j++) m = fmaxf(m, x[j]);
  float sum = 0.0f;
  for (int j = 0; j < n_out; j++) sum += expf(x[j] - m);
  int best = 0;
  float qbest = -1.0f;
  for (int j = 0; j < n_out; j++) {
    const float q = expf(x[j] - m) / sum;
    if (q_out) q_out[j] = q;
    if (q > qbest) { qbest = q; best = j; }
  }
  if (qbest_out) *qbest_out = qbest;
  return best;
}
// Agent_DQN.select_action on the softmax: its argmax or, with probability eps, a uniform random
// action from the env's own counter-based stream.  One lane, one env; q (may be NULL) gets the softmax.
__device__ __forceinline__ int gp_choose(const float* x, int n_out, float eps, uint64_t seed, uint64_t decision,
                                         uint64_t gid, float* q_out) {
  int best = gp_softmax_argmax(x, n_out, q_out, nullptr);
  const uint64_t h1 = gp_mix(seed ^ gp_mix(gid * 0x100000001B3ull + decision));
  const uint64_t h2 = gp_mix(h1);
  const float u = (float)((h1 >> 40) * (1.0 / 16777216.0));   // 24-bit uniform in [0, 1)
  if (u < eps) best = (int)(h2 % (uint64_t)n_out);
  return best;
}

// The layers of gp_forward_tile on rows already in act[0] ([16][kpad[0]], zero where a row or a
// column is padding; written by any lanes of the workgroup: the leading barrier orders them):
// the only MFMA loop of the tile form.  gm_sac.hip's critic kernel assembles [state | action]
// rows there itself.  Returns cur.
__device__ __forceinline__ int gp_layers_tile(const float* __restrict__ params, const GpNet& P, int code,
                                              float (*act)[GP_TILE][GP_ROW], int lane) {
  __syncthreads();
  int cur = 0;
  for (int l = 0; l < P.n_layers; l++) {
    const float* __restrict__ W = params + P.woff[l];
    const float* __restrict__ Bv = params + P.boff[l];
    const int ksteps = P.kpad[l] >> 2;
    const bool last = (l == P.n_layers - 1);
    const int outw = P.width[l + 1];
    for (int t = 0; t < P.tiles[l]; t++) {
      gp_f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
      const float* Wt = W + (size_t)t * ksteps * 64;
      for (int s = 0; s < ksteps; s++) {
        const float a = act[cur][lane & 15][4 * s + (lane >> 4)];
        const float b = Wt[s * 64 + lane];
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
      }
      // D fragment: output column j = 16 t + (lane & 15), env row (lane >> 4) * 4 + r
      const int j = t * 16 + (lane & 15);
      const float bias = Bv[j];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        float v = c[r] + bias;
        if (!last) v = gp_activate(v, code);
        act[cur ^ 1][(lane >> 4) * 4 + r][j] = (j < outw) ? v : 0.0f;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  return cur;
}

// One net's forward for a tile of 16 envs, one wave per tile (gm_policy_kernel, gm_ac_kernel):
// observations of envs e0 .. e0 + 15 of obs[n_envs][n_obs] -> act[cur][env row][output]; returns
// cur.  Hidden layers get gp_activate(code), the last layer none.  copy, when non-NULL, receives
// the observations as loaded ([n_envs][n_obs]).  The leading barrier lets a second net reuse
// the rows once every lane has read the first one's outputs.
__device__ __forceinline__ int gp_forward_tile(const float* __restrict__ obs, float* __restrict__ copy, int e0,
                                               int n_envs, const float* __restrict__ params, const GpNet& P, int code,
                                               float (*act)[GP_TILE][GP_ROW], int lane) {
  const int n_obs = P.width[0];
  const int k0 = P.kpad[0];
  __syncthreads();
  for (int i = lane; i < GP_TILE * k0; i += 64) {
    const int r = i / k0, k = i - r * k0;
    const bool in = e0 + r < n_envs && k < n_obs;
    const float o = in ? obs[(size_t)(e0 + r) * n_obs + k] : 0.0f;
    act[0][r][k] = o;
    if (copy && in) copy[(size_t)(e0 + r) * n_obs + k] = o;
  }
  return gp_layers_tile(params, P, code, act, lane);
}

// The same forward for ONE env on its own wave (gm_rollout's drivers, gm_rollout.h
// chunked_env_steps and ac_rollout_driver): the tile form's MFMA tiles with this env in row 0
// and zero rows below it.  MFMA rows are independent, so every output is bit for bit the tile
// form's for the same observation.  obs: the env's observation (read with agent-scope loads,
// past this CU's L1: the env-step epilogue or a reset on another CU may have written it); copy,
// when non-NULL, receives it as loaded.  act: 2 x GP_ROW floats of LDS scratch; the wave-level
// fences order its rows (the workgroup may hold a second wave that must not be waited for).
// Returns the buffer (0 / 1) whose row holds the outputs.
__device__ __forceinline__ int gp_forward_one(const float* obs, float* copy, const float* __restrict__ params,
                                              const GpNet& P, int code, float* act, int lane) {
  const int n_obs = P.width[0];
  const int k0 = P.kpad[0];
  // this wave's own stores of the observation (the previous env-step's epilogue or reset,
  // other lanes) have reached L2 before the loads below go there
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  for (int k = lane; k < k0; k += 64) {
    const float o = k < n_obs ? __hip_atomic_load(obs + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
    act[k] = o;
    if (copy && k < n_obs) copy[k] = o;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  int cur = 0;
  for (int l = 0; l < P.n_layers; l++) {
    const float* __restrict__ Wl = params + P.woff[l];
    const float* __restrict__ Bv = params + P.boff[l];
    const int ksteps = P.kpad[l] >> 2;
    const bool last = (l == P.n_layers - 1);
    const int outw = P.width[l + 1];
    const float* src = act + cur * GP_ROW;
    float* dst = act + (cur ^ 1) * GP_ROW;
    for (int t = 0; t < P.tiles[l]; t++) {
      gp_f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
      const float* Wt = Wl + (size_t)t * ksteps * 64;
      for (int s = 0; s < ksteps; s++) {
        const float a = (lane & 15) == 0 ? src[4 * s + (lane >> 4)] : 0.0f;
        const float b = Wt[s * 64 + lane];
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
      }
      // row 0 of the D fragment: lanes 0..15, element 0; column j = 16 t + lane
      const int j = t * 16 + (lane & 15);
      if (lane < 16) {
        float v = c[0] + Bv[j];
        if (!last) v = gp_activate(v, code);
        dst[j] = (j < outw) ? v : 0.0f;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    cur ^= 1;
  }
  return cur;
}

// select_action for ONE env on its own wave (gm_rollout's policy driver, gm_rollout.h
// chunked_env_steps): the ReLU forward, then lane 0 chooses.  act: 2 x GP_ROW floats of LDS
// scratch.  Returns the action on every lane.
__device__ __forceinline__ int gp_select_one(const float* obs, const float* __restrict__ params, const GpNet& P,
                                             float eps, uint64_t seed, uint64_t decision, uint64_t gid, float* act,
                                             int lane) {
  const int cur = gp_forward_one(obs, nullptr, params, P, GP_ACT_RELU, act, lane);
  int best = 0;
  if (lane == 0) best = gp_choose(act + cur * GP_ROW, P.width[P.n_layers], eps, seed, decision, gid, nullptr);
  return __builtin_amdgcn_readfirstlane(best);
}
