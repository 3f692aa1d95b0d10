// gm_policy.hip -- the batched select_action kernel: gm_policy_net.h's tile forward (shared
// with the actor-critic kernels) with ReLU, then the selection (shared with gm_rollout's
// per-env policy driver, gp_select_one).
#pragma once
#include "gm_policy_net.h"

__global__ __launch_bounds__(64) void gm_policy_kernel(const float* __restrict__ obs, int n_envs, long long env_offset,
                                                       const float* __restrict__ params, GpNet P, float eps,
                                                       uint64_t seed, uint64_t decision, int32_t* __restrict__ actions,
                                                       float* __restrict__ qout) {
  __shared__ float act[2][GP_TILE][GP_ROW];
  const int lane = threadIdx.x;
  const int e0 = blockIdx.x * GP_TILE;
  const int cur = gp_forward_tile(obs, nullptr, e0, n_envs, params, P, GP_ACT_RELU, act, lane);
  // softmax over the logits (nn.Softmax(dim=1)), then select_action (gp_choose)
  if (lane < GP_TILE && e0 + lane < n_envs) {
    const size_t env = (size_t)(e0 + lane);
    const int n_out = P.width[P.n_layers];
    actions[env] = gp_choose(act[cur][lane], n_out, eps, seed, decision, (uint64_t)(env_offset + (long long)env),
                             qout ? qout + env * n_out : nullptr);
  }
}
