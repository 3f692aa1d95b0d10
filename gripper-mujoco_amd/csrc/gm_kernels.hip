// gm_kernels.hip -- the MI355X (gfx950) batched env-step hot path.
//
// One 64-lane workgroup (one wavefront) per env.  A launch runs a whole
// MjClass::action_step() (mjclass.cpp:1483-1508): S = sim_steps_per_action
// physics substeps, each = MuJoCo-style mj_step1 / control / mj_step2
// (myfunctions.cpp:1873-1898) + after_step/update_all (1900-1908, 2110-2284)
// + monitor_sensors (mjclass.cpp:741-898), then sense_gripper_state,
// update_env, get_observation, is_done and reward -- without leaving the chip.
// Per-env state is moved HBM -> LDS once at entry and back once at exit; all
// per-substep working data (kinematics, mass matrix, contacts, constraint
// rows) stays in LDS / VGPRs.  Lane mapping per stage:
//   - kinematic chains (3 fingers, palm, object): one lane per chain
//   - mass-matrix rows, bias/passive/actuator forces: one lane per dof
//   - collision: one lane per candidate geom pair (63 pairs <= 64 lanes)
//   - constraint rows (pyramid edges + motor locks): one lane per row; the
//     row's Delassus column A[:, j] lives in that lane's VGPRs and projected
//     Gauss-Seidel broadcasts each row's update with v_readlane (no LDS, no
//     reductions in the inner loop)
//   - reference scalar logic (stepper in fp64, events, RNG): lane 0
// The algorithm is the engine spec restated in oracle/oracle.c (fp64); this file
// and the stage headers it includes are the fp64 device implementation of the same spec (MuJoCo's mjtNum is double),
// with fp32 only where the reference itself uses float (sensor windows, observations).
// The stages live in headers of their own (map: DESIGN.md section 5).  Both translation units
// get gm_rollout.h: step_kernel_body names chunked_env_steps under `if constexpr (!CAL)`.
#pragma once
#include "gm_rollout.h"

// mode 0: action_step + obs/done/reward; mode 1: calibrate_reset settle (400 substeps,
// no sensors); mode 2: one full substep with diagnostics
#ifndef GM_WPS
#define GM_WPS 2   // waves per SIMD the register allocation is held to
#endif
// DUO workgroups (small batches, gm_capi.hip launch_step): the second wave of the
// workgroup runs each substep's collider for the env the first wave owns, between the
// first two barriers of physics_substep_body, with its own box-box hit slots, then the
// factor of integrate's Euler damping solve while the owner runs the constraint solve
// (third barrier, in integrate); duo_cmd = 0 releases it.
template <int CL>
__device__ __forceinline__ void duo_helper(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T) {
  __shared__ real hit[GM_BB_SLOTS][8][4];
  for (;;) {
    __syncthreads();
    if (S.duo_cmd == 0) return;
    collision<CL>(S, m, T, fresh_lane(), false, hit);
    {
      // the constraint setup's contact rows for the owner (contact_rows), the body
      // velocities in the hit slots (dead once the contacts are written).  (Measured: only
      // on the substeps whose collider ran no MPR, the owner forming them on the rest, was
      // no better: tools/duo_rows_ab.sh, profiles/r06_ab_duo_rows.txt)
      static_assert(sizeof(hit) >= sizeof(real) * 12 * SharedT<CL>::NB, "two velocity sets fit the hit slots");
      const int ln = fresh_lane();
      real (*V)[6] = reinterpret_cast<real (*)[6]>(&hit[0][0][0]);
      real cD, caref[4], jq[4];
      bool oo;
      contact_rows<CL, false>(S, m, T, ln, V, V + SharedT<CL>::NB, cD, caref, jq, oo);
      DuoRows<CL>* dr = duo_rows<CL>();
      if (ln < GM_MAX_CON) {
        dr->cD[ln] = cD;
#pragma unroll
        for (int e = 0; e < 4; e++) { dr->caref[e][ln] = caref[e]; dr->jq[e][ln] = jq[e]; }
      }
      if (ln == 0) dr->obj_only = oo ? 1 : 0;
    }
    __syncthreads();
    // M is formed (the owner wave's mass_and_forces ran before the barrier): the Euler
    // damping factor for integrate, while the owner runs the constraint solve
    if (m->mujoco_actuators != 0) {
      const int ln = fresh_lane();
      real L[CL + 1], lb, invd;
      const real sch = euler_factor<CL>(S, T, m->timestep, ln, L, lb, invd);
      real* ef = duo_ef<CL>();
#pragma unroll
      for (int j = 1; j <= CL; j++) ef[(j - 1) * 64 + ln] = L[j];
      ef[CL * 64 + ln] = lb;
      ef[(CL + 1) * 64 + ln] = invd;
      if (ln == 0) ef[64 * (CL + 2)] = sch;
    }
    __syncthreads();
  }
}
template <int CL, bool CAL, bool DUO, bool EVAL = false>
__device__ __forceinline__ void step_kernel_body(SharedT<CL>& S,
    GmEnvState* __restrict__ states, const gm_model* __restrict__ m, const gm_config* __restrict__ C,
    const GmTopo* __restrict__ T, float* __restrict__ obs, float* __restrict__ rew,
    uint8_t* __restrict__ done, int n_envs, int mode, DebugOut dbg, const int32_t* __restrict__ order,
    uint32_t* __restrict__ cost, const GmChunkQ& q, int lane) {
  if constexpr (!CAL) {
    if (q.chunk > 0) {   // chunked work queue (gm_step): the grid is the resident wave slots
      chunked_env_steps<CL, DUO, EVAL>(S, states, m, C, T, obs, rew, done, n_envs, order, cost, q, lane);
      return;
    }
  }
  if constexpr (EVAL) return;   // (an evaluation launch is a queue launch: gm_eval.hip)
  if ((int)blockIdx.x >= n_envs) return;
  // cost-sorted dispatch: workgroups start in blockIdx order, so the envs that were the
  // most expensive last env-step are started first (longest-processing-time list
  // scheduling over the resident slots; see gm_dispatch_order_kernel)
  const int env = order ? order[blockIdx.x] : (int)blockIdx.x;
  const unsigned long long t_start = cost ? __builtin_amdgcn_s_memtime() : 0;
  load_state(S, states + env, lane);
  const bool settle = (mode == 1);          // calibrate_reset settle: 400 substeps, no sensors
  const bool calib = CAL;                   // calibration run (mode 3): S.s.cal_steps substeps, no sensors
  const bool prof = !settle && dbg.phase != nullptr;
  if (prof && lane < GM_NPHASE) S.tph[lane] = 0;
  // profiling timeline: start / end on the 100 MHz constant clock and the wave's CU, for
  // the dispatch-occupancy analysis (tools/tail_bench.py)
  if (prof && lane == 0) { S.tph[25] = __builtin_amdgcn_s_memrealtime(); S.tph[27] = __smid(); }
  if (lane == 0) { S.work_nefc = 0; S.work_mpr = 0; S.work_newton = 0; S.stp_fixed = 0; }
  const unsigned long long t_kernel = prof ? clock64() : 0;
  GM_ENV_SYNC();
  const int nsub = settle ? 400 : calib ? S.s.cal_steps : (mode == 2) ? 1 : C->sim_steps_per_action + S.s.extra_substeps;
  // a calibration run starts from a reset's mj_forward pose
  if (calib && lane < T->nlock) S.lock_pre[lane] = S.s.qpos[m->lock_dof[lane]];
  int ran;
  if constexpr (DUO) {   // (profiled: the owner wave's clocks; its "collision" is the wait for the helper)
    ran = prof ? substep_loop<CL, CAL, true, true>((GM_AS_LDS SharedT<CL>*)&S, (const GM_AS_GLOBAL gm_model*)m,
                                                   (const GM_AS_GLOBAL GmTopo*)T, (const GM_AS_GLOBAL gm_config*)C, lane,
                                                   prof, nsub, settle, GmPreempt{})
               : substep_loop<CL, CAL, false, true>((GM_AS_LDS SharedT<CL>*)&S, (const GM_AS_GLOBAL gm_model*)m,
                                                    (const GM_AS_GLOBAL GmTopo*)T, (const GM_AS_GLOBAL gm_config*)C, lane,
                                                    false, nsub, settle, GmPreempt{});
  } else {
    ran = prof ? substep_loop<CL, CAL, true>((GM_AS_LDS SharedT<CL>*)&S, (const GM_AS_GLOBAL gm_model*)m,
                                             (const GM_AS_GLOBAL GmTopo*)T, (const GM_AS_GLOBAL gm_config*)C, lane,
                                             prof, nsub, settle, GmPreempt{})
               : substep_loop<CL, CAL, false>((GM_AS_LDS SharedT<CL>*)&S, (const GM_AS_GLOBAL gm_model*)m,
                                              (const GM_AS_GLOBAL GmTopo*)T, (const GM_AS_GLOBAL gm_config*)C, lane,
                                              false, nsub, settle, GmPreempt{});
  }
  // a calibration run reports the substeps it made (the unstable one included: the loop
  // stops right after it, as the reference's retry resumes after it)
  if (calib && lane == 0) S.s.cal_steps = S.s.badqacc ? ran + 1 : ran;
  if (settle || calib) {
    store_state(S, states + env, lane);
    return;
  }
  if (mode == 2) {
    if (lane == 0) { dbg.ncon[env] = S.ncon; dbg.nefc[env] = S.nefc; }
    if (lane < GM_MAX_CON) {
      double* o = dbg.contact + ((size_t)env * GM_MAX_CON + lane) * 16;
      for (int k = 0; k < 16; k++) o[k] = 0;
      if (lane < S.ncon) {
        const real* Cc = S.con[lane];
        o[0] = Cc[0];
        for (int k = 0; k < 3; k++) o[1 + k] = Cc[1 + k];
        for (int k = 0; k < 6; k++) o[4 + k] = Cc[4 + k];
        cross3(o + 10, Cc + 4, Cc + 7);
        o[13] = S.cgeom[lane][0]; o[14] = S.cgeom[lane][1]; o[15] = Cc[10];
      }
    }
    for (int r = lane; r < GM_MAX_EFC; r += NT)
      dbg.efc_force[(size_t)env * GM_MAX_EFC + r] = r < S.nefc ? S.dbg.efc[r] : 0.0;
    if (lane < GM_MAX_DOF) dbg.qacc[(size_t)env * GM_MAX_DOF + lane] = lane < T->nv ? S.qacc[lane] : 0.0;
    {
      real w[6];
      object_net_wrench(S, T, lane, w);
      if (lane == 0) for (int k = 0; k < 6; k++) dbg.wrench[(size_t)env * 6 + k] = w[k];
    }
    store_state(S, states + env, lane);
    return;
  }
  unsigned long long t0 = prof ? clock64() : 0;
  env_step_epilogue(S, m, C, T, obs, rew, done, env, lane, prof, t0);
  if (prof) {
    if (lane == 0) {
      S.tph[23] = clock64() - t_kernel;   // whole env-step on this wave
      S.tph[26] = __builtin_amdgcn_s_memrealtime();
    }
    GM_ENV_SYNC();
    if (lane < GM_NPHASE) dbg.phase[(size_t)env * GM_NPHASE + lane] = S.tph[lane];
  }
  if (cost && lane == 0)   // recorded for the next launch's order
    cost[n_envs + env] = dispatch_cost((uint32_t)((__builtin_amdgcn_s_memtime() - t_start) >> 6), 1u, S.work_nefc,
                                       S.work_mpr, S.work_newton);
  store_state(S, states + env, lane);
}
// EVAL: the evaluation launch's instantiations (gm_eval.hip; chunked_env_steps)
template <int CL, bool CAL, bool DUO = false, bool EVAL = false>
__global__ __launch_bounds__(DUO ? 2 * NT : NT, GM_WPS) void gm_step_kernel(
    GmEnvState* __restrict__ states, const gm_model* __restrict__ m, const gm_config* __restrict__ C,
    const GmTopo* __restrict__ T, float* __restrict__ obs, float* __restrict__ rew,
    uint8_t* __restrict__ done, int n_envs, int mode, DebugOut dbg, const int32_t* __restrict__ order,
    uint32_t* __restrict__ cost, GmChunkQ q) {
  __shared__ SharedT<CL> S;
  if constexpr (DUO) {
    static_assert(!CAL, "DUO workgroups run the env-step only");
    if (threadIdx.x >= NT) {
      duo_helper<CL>(S, m, T);
      return;
    }
  }
  step_kernel_body<CL, CAL, DUO, EVAL>(S, states, m, C, T, obs, rew, done, n_envs, mode, dbg, order, cost, q, (int)threadIdx.x);
  if constexpr (DUO) {
    // every path of the owner wave ends here: release the helper
    if (threadIdx.x == 0) S.duo_cmd = 0;
    __syncthreads();
  }
}
