// gm_substep.h -- one physics substep (mj_step1 / control / mj_step2, myfunctions.cpp:1873-1898)
// and an env-step's outlined substep loop with update_all (1900-1908), monitor_sensors and the
// work queue's preemption test.  SharedT: writes lock_pre, duo_cmd, next_read, tph
// (calibration: s.lock_active, s.lock_q); the rest through the stages it calls.
#pragma once
#include "gm_dynamics.h"
#include "gm_collide.h"
#include "gm_newton.hip"
#include "gm_integrate.h"
#include "gm_gripper.h"
#include "gm_sensors.h"
// the chunked work queue: GmRolloutJob, GmChunkQ, GmPreempt and the scheduler's pieces
#include "gm_chunkq.h"

// ============================================================ one full substep
template <int CL, bool CAL, bool DUO>
__device__ __forceinline__ void physics_substep_body(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T,
                                                     int lane, bool prof) {
  unsigned long long t0 = prof ? clock64() : 0;
  if (lane < T->nlock) S.lock_pre[lane] = S.s.qpos[m->lock_dof[lane]];
  kinematics<CL>(S, m, T, fresh_lane(), prof);
  PH(0);
  if constexpr (DUO) {
    // the collider needs only the poses: the helper wave runs it (duo_helper) while this
    // wave forms the inertia and forces; the two barriers are the handshake
    if (lane == 0) S.duo_cmd = 1;
    __syncthreads();
    crb_rne<CL, CAL>(S, m, T, fresh_lane(), prof);
    PH(1);
    mass_and_forces<CL, CAL>(S, m, T, fresh_lane());
    PH(2);
    __syncthreads();
  } else {
    crb_rne<CL, CAL>(S, m, T, fresh_lane(), prof);
    PH(1);
    mass_and_forces<CL, CAL>(S, m, T, fresh_lane());
    PH(2);
    collision(S, m, T, fresh_lane(), prof, S.cl.hit);
  }
  PH(5);
  newton_solve<CL, CAL, DUO>(S, m, T, fresh_lane(), prof);
  PH(6);
  integrate<CL, CAL, DUO>(S, m, T, fresh_lane(), prof);
  PH(8);
}

#define GM_AS_LDS __attribute__((address_space(3)))
#define GM_AS_GLOBAL __attribute__((address_space(1)))
#define GM_AS_CONST __attribute__((address_space(4)))
// The model and topology pointers arrive in VGPRs (callee ABI); read back as wave-uniform
// constant-address-space pointers, every access with a uniform index is a scalar load
// through the scalar cache instead of a vector memory round trip.
template <typename P>
__device__ __forceinline__ const GM_AS_CONST P* uniform_const_ptr(const GM_AS_GLOBAL P* p) {
  const uint64_t a = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return (const GM_AS_CONST P*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}
// The substep loop: one outlined call per env-step.  Its own register allocation (the
// kernel around it keeps the env-step epilogue's state), parameters typed with their
// address spaces so the body issues scalar / global loads for the model and LDS
// instructions for the per-env image rather than generic (flat) accesses.  The
// callee-saved registers it uses are saved and restored once per env-step (an outlined
// call per substep paid that, ~92 VGPRs x 64 lanes x 2, every substep: 12 GB of scratch
// traffic per 4096-env launch).  update_all and monitor_sensors are small calls of
// their own inside the loop, so the loop body keeps the physics' register allocation.
// Built with MachineLICM off (gmx/build.py): hoisting the sincos / polynomial constant
// materialisations out of the loop would hold them live across the whole body and spill.
template <int CL>
__device__ __noinline__ void update_all_call(GM_AS_LDS SharedT<CL>* S_, const GM_AS_GLOBAL gm_model* m_,
                                             const GM_AS_GLOBAL GmTopo* T_, int lane) {
  update_all<CL>(*(SharedT<CL>*)S_, (const gm_model*)uniform_const_ptr(m_), (const GmTopo*)uniform_const_ptr(T_), lane);
}
template <int CL>
__device__ __noinline__ void monitor_call(GM_AS_LDS SharedT<CL>* S_, const GM_AS_GLOBAL gm_model* m_,
                                          const GM_AS_GLOBAL gm_config* C_, const GM_AS_GLOBAL GmTopo* T_, int lane) {
  monitor_sensors<CL>(*(SharedT<CL>*)S_, (const gm_model*)uniform_const_ptr(m_), (const gm_config*)uniform_const_ptr(C_),
                      (const GmTopo*)uniform_const_ptr(T_), lane);
}
// returns the substeps run (nsub unless the preemption test yielded).  PROF = false
// compiles the per-phase clock reads (PH) out: no uniform branch at every phase boundary,
// so the scheduler's regions span them (the env-step kernel's chunked path runs this one)
template <int CL, bool CAL, bool PROF, bool DUO = false>
__device__ __noinline__ int substep_loop(GM_AS_LDS SharedT<CL>* S_, const GM_AS_GLOBAL gm_model* m_,
                                         const GM_AS_GLOBAL GmTopo* T_, const GM_AS_GLOBAL gm_config* C_, int lane_in,
                                         bool prof_in, int nsub_in, bool settle_in, GmPreempt pre) {
  // nothing but scalars is carried across the loop body: the loop bounds and flags are
  // wave-uniform (SGPRs), the lane id is recomputed, the next sensor-read time lives in LDS
  SharedT<CL>& S = *(SharedT<CL>*)S_;
  const GM_AS_CONST gm_model* m_s = uniform_const_ptr(m_);
  const GM_AS_CONST GmTopo* T_s = uniform_const_ptr(T_);
  const gm_config* C = (const gm_config*)uniform_const_ptr(C_);
  const int nsub = __builtin_amdgcn_readfirstlane(nsub_in);
  const bool prof = PROF && __builtin_amdgcn_readfirstlane((int)prof_in) != 0;
  const bool settle = __builtin_amdgcn_readfirstlane((int)settle_in) != 0;
  (void)lane_in;
  const int every = CAL ? 0 : __builtin_amdgcn_readfirstlane(pre.every);
  if (__lane_id() == 0) S.next_read = (settle || CAL) ? 0.0 : next_sensor_read(S.s, C->s);
  GM_WAVE_SYNC();
  int i = 0;
#pragma nounroll
  for (; i < nsub; i++) {
    if (every > 0 && i > 0 && i % every == 0) {
      // work left in the units of the cost array, times pre.total
      const uint64_t left = (uint64_t)__builtin_amdgcn_readfirstlane(pre.own) *
                            (uint64_t)(__builtin_amdgcn_readfirstlane(pre.left) - i);
      const uint64_t total = (uint64_t)__builtin_amdgcn_readfirstlane(pre.total);
      const int pm = __builtin_amdgcn_readfirstlane(pre.prio);
      if (pm > 0) job_prio(left / (total ? total : 1u), __builtin_amdgcn_readfirstlane(pre.cmax), pm);
      const uint32_t fh = __builtin_amdgcn_readfirstlane(ld_agent(pre.fresh_head));
      const uint32_t n = __builtin_amdgcn_readfirstlane(pre.n);
      if (fh < n) {
        const uint64_t next = (uint64_t)__builtin_amdgcn_readfirstlane(pre.cost[pre.order[fh]]) *
                              (uint64_t)__builtin_amdgcn_readfirstlane(pre.steps);
        // (with a margin: a yield costs a state hand-off)
        if (left * (uint64_t)(100 + __builtin_amdgcn_readfirstlane(pre.margin)) < next * total * 100u) break;
      }
      const int cm = __builtin_amdgcn_readfirstlane(pre.cmargin);
      if (cm >= 0) {
        const int ln = __lane_id();
        uint32_t hb = 0, tb = 0;
        if (ln < GM_CQ_NB) { hb = ld_agent(pre.bq + ln * 32); tb = ld_agent(pre.bq + ln * 32 + 1); }
        const unsigned long long ne = __ballot(ln < GM_CQ_NB && hb < tb);
        if (ne) {
          const uint64_t b = 63 - __builtin_clzll(ne);
          const uint64_t lower = b * (uint64_t)__builtin_amdgcn_readfirstlane(pre.cmax) / GM_CQ_NB;
          if (left * (uint64_t)(100 + cm) < lower * total * 100u) break;
        }
      }
    }
    // opaque per iteration: nothing derived from the lane id or the model / topology
    // pointers is hoisted out of the loop and held live across the whole body
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    // (the opaque copy keeps the constant address space: every model / topology access
    // stays a scalar load when its index is uniform, a global load otherwise -- a generic
    // pointer would make them flat loads that wait on LDS traffic too)
    const GM_AS_CONST gm_model* mc = m_s;
    const GM_AS_CONST GmTopo* Tc = T_s;
    asm volatile("" : "+s"(mc), "+s"(Tc));
    const gm_model* m = (const gm_model*)mc;
    const GmTopo* T = (const GmTopo*)Tc;
    if (CAL && S.s.tip_force != 0.0 && lane < T->nlock && m->lock_kind[lane] == 0) {
      S.s.lock_active[lane] = 1;
      S.s.lock_q[lane] = S.lock_pre[lane];
    }
    const unsigned long long tc = prof ? clock64() : 0;
    physics_substep_body<CL, CAL, DUO>(S, m, T, lane, prof);
    unsigned long long t0 = prof ? clock64() : 0;
    if (prof && lane == 0) S.tph[22] += t0 - tc;
    update_all<CL>(S, m, T, fresh_lane());
    PH(9);
    if (!settle && !CAL && S.s.time > S.next_read) {
      monitor_call<CL>((GM_AS_LDS SharedT<CL>*)&S, (const GM_AS_GLOBAL gm_model*)(uintptr_t)m,
                       (const GM_AS_GLOBAL gm_config*)(uintptr_t)C, (const GM_AS_GLOBAL GmTopo*)(uintptr_t)T, __lane_id());
      if (__lane_id() == 0) S.next_read = next_sensor_read(S.s, C->s);
      GM_WAVE_SYNC();
    }
    PH(10);
    if (CAL && S.s.badqacc) break;
  }
  return i;
}
