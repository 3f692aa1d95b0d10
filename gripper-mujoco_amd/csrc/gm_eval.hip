// gm_eval.hip -- the evaluation launch's instantiations of the env-step kernel
// (gm_step_kernel<CL, false, DUO, true>: gm_rollout.h chunked_env_steps with EVAL), compiled as a
// translation unit of its own like the calibration variant (gm_calib.hip), so that they compile
// beside the rollouts' kernels and leave those kernels' code alone ("Evaluation
// launch").  The physics is the same source with the same flags.
// The host side is eval_launch in gm_capi.hip.
#include "gm_kernels.hip"

// One persistent launch of an evaluation job on the chunked queue q (grid: its resident
// workgroups; duo: the context's DUO workgroups), the arguments gm_capi.hip's launch_step passes
hipError_t gm_eval_launch_step(int n_seg, bool duo, int grid, hipStream_t st, GmEnvState* states, const gm_model* m,
                               const gm_config* C, const GmTopo* T, float* obs, float* rew, uint8_t* done, int n_envs,
                               const int32_t* order, uint32_t* cost, const GmChunkQ& q) {
  DebugOut dbg{nullptr, nullptr, nullptr, nullptr, nullptr};
  switch (n_seg) {
#define X(N)                                                                                                  \
  case N:                                                                                                     \
    if (duo)                                                                                                  \
      hipLaunchKernelGGL((gm_step_kernel<N + 2, false, true, true>), dim3(grid), dim3(2 * NT), 0, st, states, \
                         m, C, T, obs, rew, done, n_envs, 0, dbg, order, cost, q);                            \
    else                                                                                                      \
      hipLaunchKernelGGL((gm_step_kernel<N + 2, false, false, true>), dim3(grid), dim3(NT), 0, st, states, m, \
                         C, T, obs, rew, done, n_envs, 0, dbg, order, cost, q);                               \
    return hipGetLastError();
    GM_NSEG_LIST
#undef X
    default: return hipErrorInvalidValue;
  }
}
