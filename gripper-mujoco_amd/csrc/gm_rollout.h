// gm_rollout.h -- the chunked env-step's rollout job: the scripted / random / program drivers
// (gm_scripted_actions, gm_random_actions, gm_program_actions), the actor-critic driver, the
// SAC driver, the in-kernel auto-reset and chunked_env_steps, a resident wave's loop over the queue's jobs.
// SharedT: s through the stages it calls; st (activations, spawn buffers), stp_fixed, work_*.
#pragma once
#include "gm_substep.h"
#include "gm_readout.h"
#include "gm_reset.h"
#include "gm_chunkq.h"
#include "gm_policy_net.h"
#include "gm_ac_net.h"
#include "gm_replay.h"
#include "gm_sac_net.h"

// ------------------------------ chunked env-step: the rollout job (its work queue: gm_chunkq.h)
// the grasp program's inputs (gm_state.h gm_program_fraction) from an env's state and its
// SI sensor windows
__device__ __forceinline__ gm_program_in program_input(const GmEnvHot& s, RingRef R, const gm_model* __restrict__ m) {
  gm_program_in in;
  in.x = s.end.x; in.y = s.end.y; in.z = s.end.z;
  in.base_z = s.base[2];
  in.q_base = s.qpos[m->jnt_qposadr[m->body_jnt[m->body_base]]];
  in.q_palm = s.qpos[m->jnt_qposadr[m->body_jnt[m->body_palm]]];
  in.obj_z = s.qpos[m->jnt_qposadr[m->body_jnt[m->body_obj]] + 2];
  in.obj_top = gm_program_obj_top(s.obj_type, s.obj_size);
  in.z_root = m->body_pos[m->body_base][2];
  in.palm_drop = (m->finger_length - 165e-3) + 0.004;
  const float g0 = ring_latest(s, R, ST_SI_GAUGE), g1 = ring_latest(s, R, ST_SI_GAUGE + 1),
              g2 = ring_latest(s, R, ST_SI_GAUGE + 2);
  in.g_max = fmaxf(g0, fmaxf(g1, g2));
  in.palm = ring_latest(s, R, ST_SI_PALM);
  return in;
}
// the scripted drivers' fraction for action i of kind `kind` (mode: GM_DRV_SCRIPT, _RANDOM,
// _PROGRAM or _MIX)
__device__ __forceinline__ float driver_fraction(const GmEnvHot& s, RingRef R, const gm_model* __restrict__ m,
                                                 const gm_config* __restrict__ C, int mode, uint64_t seed, float jitter,
                                                 int64_t gid, int i, int kind) {
  if (mode == GM_DRV_PROGRAM || (mode == GM_DRV_MIX && gm_program_episode(seed, gid, s.episode))) {
    if (kind < 0) return 0.0f;
    const gm_action* acts[GM_N_ACTION_KINDS] = {
#define GM_AA(n, u, vv, sg) &C->s.n,
#include "gm_settings.def"
    };
    const gm_program_in in = program_input(s, R, m);
    return gm_program_fraction(&in, kind, acts[kind]->value, acts[kind]->sign);
  }
  if (mode == GM_DRV_SCRIPT || mode == GM_DRV_MIX) return gm_script_fraction(seed, gid, s.episode, s.num_action_steps, i, kind, jitter);
  return gm_random_fraction(seed, gid, s.episode, s.num_action_steps, i);
}
// the rollout driver's actions for the env's next env-step (lane 0): the same fractions
// gm_scripted_actions / gm_random_actions / gm_program_actions produce, applied as
// gm_set_action applies them
__device__ __noinline__ void driver_actions(GmEnvHot& s, RingRef R, const gm_model* __restrict__ m,
                                            const gm_config* __restrict__ C, int mode, uint64_t seed, float jitter,
                                            int64_t gid) {
  const int na = C->n_actions;
  float f[GM_ACTION_CODE_COUNT];
  // every fraction from the state before any action moves a target (the program reads them)
  for (int i = 0; i < na; i++) {
    const int code = C->action_options[i];
    const int kind = (code >= 0 && code < GM_ACTION_TERMINATION) ? code / 3 : -1;
    float v = driver_fraction(s, R, m, C, mode, seed, jitter, gid, i, kind);
    f[i] = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
  }
  for (int i = 0; i < na; i++) set_action_one(s, m, C, i, f[i]);
}

// GM_DRV_SAC (gm_sac_rollout): the SAC actor's part of one env's env-step on the env's own wave,
// called at the begin of an env-step only (through ac_rollout_driver's phase 3): gm_sac_act on this env alone and gm_sac_push_begin's
// row -- the observation into the memory's state row (as loaded for the forward), the head row
// through gs_sample, the squashed action into the action row, then lane 0 applies the clipped
// actions in order.  gm_sac_push_end's half is replay_record's phase 1 through J.replay (it needs
// no action), so the end of an env-step has no SAC code.  scratch: 2 x GP_ROW floats of LDS; the
// row the forward did not leave its outputs in holds a and u (2 n_act <= GP_ROW floats).
__device__ __noinline__ void sac_rollout_driver(const GsArgs* __restrict__ Ap, const float* obs, int env, int n_envs,
                                                int k, int64_t gid, float* scratch, GmEnvHot& s,
                                                const gm_model* __restrict__ m, const gm_config* __restrict__ C,
                                                int lane) {
  const GsArgs& A = *Ap;
  static_assert(2 * GA_MAX_ACT <= GP_ROW, "a and u fit one activation row");
  const int n_obs = A.net.pi.width[0];
  const int na = A.net.n_act;
  const size_t row = A.rep.state ? (size_t)gr_row(A.rep.row0, k, n_envs, env, A.rep.capacity) : 0;
  float* srow = A.rep.state ? A.rep.state + row * (size_t)n_obs : nullptr;
  int cur = 0;
  if (A.mode != GM_SAC_RANDOM) {
    cur = gp_forward_one(obs, srow, A.params, A.net.pi, A.net.act, scratch, lane);
  } else if (srow) {   // (replay_record's read: the wave's stores drained, then agent-scope loads)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int j = lane; j < n_obs; j += 64) srow[j] = __hip_atomic_load(obs + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (lane == 0) {
    float* a = scratch + (cur ^ 1) * GP_ROW;
    gs_sample(scratch + cur * GP_ROW, na, A.mode, A.net.limit, A.net.ls_min, A.net.ls_max, A.seed,
              A.decision0 + (uint64_t)k, (uint64_t)gid, a, a + GA_MAX_ACT, nullptr);
    for (int i = 0; i < na; i++) {
      float f = a[i];
      if (A.rep.action) A.rep.action[row * (size_t)na + i] = f;
      if (f < -1.0f) f = -1.0f; else if (f > 1.0f) f = 1.0f;
      set_action_one(s, m, C, i, f);
    }
  }
}

// GM_DRV_AC (gm_ac_rollout): the actor-critic's part of one env's env-step on the env's own
// wave, kept out of the substep loop's instruction stream (called between env-steps only).
//   phase 0, before the env-step: gm_ac_act on this env alone -- observation, mu, the sampled
//     action, logp and V(obs) into trajectory row k, then lane 0 applies the clipped actions in
//     order (gm_action_kernel's loop); a categorical actor's row holds the logits, the
//     chosen index as a float and its logp, and lane 0 applies the index as GM_DRV_DQN does;
//   phase 1, after the epilogue and before the auto-reset: gm_ac_record -- reward, end code
//     and, for a truncated env only, the critic on the post-step observation;
//   phase 2, after the env's last env-step: gm_ac_finish -- the critic on the observation left
//     in the buffer (the reset one if the env was reset).
//   phase 3: GM_DRV_SAC's begin of an env-step, handed on to sac_rollout_driver (Ap is the
//     job's GsArgs then: GmRolloutJob's union), so that the kernel has one call site for both.
// scratch: GA_ONE_FLOATS floats of LDS (the dynamics union, dead between env-steps).
__device__ __noinline__ void ac_rollout_driver(int phase, const GaArgs* __restrict__ Ap, const float* obs, int env,
                                               int n_envs, int k, int max_ep, int64_t gid, float* scratch,
                                               GmEnvHot& s, const gm_model* __restrict__ m,
                                               const gm_config* __restrict__ C, int lane) {
  if (phase == 3) {
    sac_rollout_driver(reinterpret_cast<const GsArgs*>(Ap), obs, env, n_envs, k, gid, scratch, s, m, C, lane);
    return;
  }
  const GaArgs& A = *Ap;
  // (an evaluation launch writes every env-step into the evaluator's one scratch row; the draws keep k)
  const size_t row = A.one_row ? (size_t)env : (size_t)k * (size_t)n_envs + (size_t)env;
  if (phase == 0) {
    const int n_obs = A.net.actor.width[0];
    const int na = A.net.actor.width[A.net.actor.n_layers];
    const int cur = gp_forward_one(obs, A.t_obs + row * n_obs, A.params, A.net.actor, A.net.act_actor, scratch, lane);
    float* a = scratch + 2 * GP_ROW;
    const bool cat = A.net.categorical != 0;   // (uniform) logits -> index, applied as GM_DRV_DQN applies its own
    if (lane == 0 && cat) {
      const float* x = scratch + cur * GP_ROW;
      A.t_logp[row] = ga_sample_cat(x, na, A.sample, A.seed, A.decision0 + (uint64_t)k, (uint64_t)gid, a);
      A.t_act[row] = a[0];
      if (A.t_mu)
        for (int i = 0; i < na; i++) A.t_mu[row * na + i] = x[i];
    } else if (lane == 0) {
      const float* mu = scratch + cur * GP_ROW;
      A.t_logp[row] = ga_sample(mu, A.params + A.net.log_std_off, na, A.sample, A.noise, A.seed,
                                A.decision0 + (uint64_t)k, (uint64_t)gid, a);
      for (int i = 0; i < na; i++) {
        A.t_act[row * na + i] = a[i];
        if (A.t_mu) A.t_mu[row * na + i] = mu[i];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const float v = ga_value_one(obs, A, scratch, lane);
    if (lane == 0) {
      A.t_val[row] = v;
      // One call site for both actors: the categorical index, or every clipped action in order.
      // a[0] holds the index as ga_sample_cat stored it: an integer below GA_MAX_ACT, exact in a
      // float, so (int) gives it back.  It has to survive the critic forward above: ga_value_one
      // uses scratch[0 .. 2 GP_ROW) only and must not touch a = scratch + 2 GP_ROW.
      for (int i = 0; i < (cat ? 1 : na); i++) {
        float f = a[i];
        int which = i;
        if (cat) { which = (int)f; f = 0.0f; }
        else if (f < -1.0f) f = -1.0f; else if (f > 1.0f) f = 1.0f;
        set_action_one(s, m, C, which, f);
      }
    }
  } else if (phase == 1) {
    const int end = __builtin_amdgcn_readfirstlane(gm_episode_end_code(s.done, s.num_action_steps, max_ep));
    float b = 0.0f;
    if (end == 2) b = ga_value_one(obs, A, scratch, lane);
    if (lane == 0) {
      A.t_rew[row] = s.reward;
      A.t_end[row] = (uint8_t)end;
      A.t_boot[row] = b;
    }
  } else {
    const float v = ga_value_one(obs, A, scratch, lane);
    if (lane == 0) A.t_last_val[env] = v;
  }
}

// One env's test report (gm_eval_out) from its state s at the episode's end (end: its
// gm_episode_end_code), one event column per lane: gm_get_event_rows' values and column order.
// The evaluation launch (rollout_end_step) and gm_eval_record's kernel both call this.
__device__ __noinline__ void eval_report(const GmEnvHot& s, const gm_eval_out o, int env, int end, int lane) {
  const int W = GM_N_BINARY + GM_N_LINEAR;
  for (int c = lane; c < W; c += 64) {
    const size_t i = (size_t)env * W + c;
    if (c < GM_N_BINARY) {
      o.rows[i] = s.bev_row[c]; o.abs[i] = s.bev_abs[c]; o.last[i] = (float)s.bev_last[c];
    } else {
      o.rows[i] = s.lev_row[c - GM_N_BINARY]; o.abs[i] = s.lev_abs[c - GM_N_BINARY];
      o.last[i] = s.lev_last[c - GM_N_BINARY];
    }
  }
  if (lane == 0) {
    o.ret[env] = s.cumulative_reward;
    o.length[env] = s.num_action_steps;
    o.end[env] = (uint8_t)end;
  }
}

// Where the drivers plug into the queue's env-steps ("The seam between the queue
// and the drivers"): one env of job J on its wave, its state in the LDS image S, g its HBM record;
// scratch: the union S.st.  (The begin of an env-step is in chunked_env_steps: a function cost a VGPR.)
__device__ __forceinline__ int64_t rollout_gid(const GmRolloutJob& J, int env) { return J.sr.env_offset + env; }
// End env-step k, after the epilogue: gm_autoreset_episodes on this env -- the episode-end
// record, the actor-critic's trajectory record or the DQN replay memory's second half (gm_replay.h
// replay_record), then MjEnv.reset and the reset observation.  In an evaluation launch (EVAL)
// an env whose episode ended writes its test report instead, is not reset, and the call returns
// nonzero: the env retires (chunked_env_steps ends its job there).  Returns 0 otherwise.
template <int CL, bool EVAL>
__device__ __forceinline__ int rollout_end_step(SharedT<CL>& S, GmEnvState* g, float* __restrict__ obs, int env,
                                                 int n_envs, const GmRolloutJob& J, int k, const gm_model* __restrict__ m,
                                                 const gm_config* __restrict__ C, const GmTopo* __restrict__ T, int lane) {
  if (J.driver < 0) return 0;
  const int end = __builtin_amdgcn_readfirstlane(gm_episode_end_code(S.s.done, S.s.num_action_steps, J.max_ep));
  if (lane == 0 && J.rec)
    J.rec[(size_t)k * (uint32_t)n_envs + env] =
        gm_episode_end_record(end, S.s.cumulative_reward, S.s.num_action_steps, S.s.bev_last[GM_EV_successful_grasp]);
  if constexpr (EVAL) {   // (nothing is recorded: no trajectory record, no replay memory)
    if (end) {
      GM_ENV_SYNC();   // lane 0's epilogue writes (the event rows) before the lanes read their columns
      eval_report(S.s, J.ev, env, end, lane);
    }
    return end;   // no reset: the env retires where its episode ended
  }
  if (J.driver == GM_DRV_AC)
    ac_rollout_driver(1, J.ac, obs + (size_t)env * C->n_obs, env, n_envs, k, J.max_ep, rollout_gid(J, env),
                      reinterpret_cast<float*>(&S.st), S.s, m, C, lane);
  if (J.replay) replay_record(1, J.replay, obs + (size_t)env * C->n_obs, env, n_envs, k, end, &S.s.reward, lane);
  if (end) {
    GM_ENV_SYNC();   // lane 0's epilogue writes (RNG, counters) before every lane reads them
    const GmResetKeep keep{S.s.rng, S.s.old_x, S.s.old_y, S.s.old_z, S.s.episode + 1, S.s.newton_caps};
    GM_ENV_SYNC();   // every lane has read what survives before the image is cleared
    static_assert(sizeof(S.st) >= sizeof(uint16_t) * (GM_SPAWN_MAX_XY + GM_SPAWN_MAX_ROT), "spawn buffers fit the union");
    uint16_t* sh_pxy = reinterpret_cast<uint16_t*>(&S.st);
    reset_env(S.s, *g, keep, m, C, T, J.eq, nullptr, J.objs, J.n_objects, env, J.scene, J.scene_tries, J.sr,
              sh_pxy, sh_pxy + GM_SPAWN_MAX_XY, lane);
    get_obs_lanes(S.s, g->ring, C, obs + (size_t)env * C->n_obs, lane);
  }
  return 0;
}
// Finish the job after its last env-step (k_end = J.steps): the actor-critic's last value
// (an evaluation keeps no trajectory: none)
template <int CL, bool EVAL>
__device__ __forceinline__ void rollout_finish(SharedT<CL>& S, GmEnvState* g, float* __restrict__ obs, int env,
                                               int n_envs, const GmRolloutJob& J, int k_end, const gm_model* __restrict__ m,
                                               const gm_config* __restrict__ C, int lane) {
  if (!EVAL && J.driver == GM_DRV_AC)
    ac_rollout_driver(2, J.ac, obs + (size_t)env * C->n_obs, env, n_envs, k_end, J.max_ep, rollout_gid(J, env),
                      reinterpret_cast<float*>(&S.st), S.s, m, C, lane);
}

// the persistent loop of gm_step_kernel's chunked mode (a mode of the one kernel, not a
// kernel of its own: substep_loop keeps its single caller and so its constant LDS base): take
// work; load state and carry; per env-step actions, substeps, epilogue, end; finish or yield.
// EVAL: the evaluation launch ("Evaluation launch"), instantiated in gm_eval.hip.
template <int CL, bool DUO, bool EVAL = false>
__device__ __forceinline__ void chunked_env_steps(SharedT<CL>& S, GmEnvState* __restrict__ states,
                                                  const gm_model* __restrict__ m, const gm_config* __restrict__ C,
                                                  const GmTopo* __restrict__ T, float* __restrict__ obs,
                                                  float* __restrict__ rew, uint8_t* __restrict__ done, int n_envs,
                                                  const int32_t* __restrict__ order, uint32_t* __restrict__ cost,
                                                  const GmChunkQ& q, int lane) {
  GmCqWave w = cq_wave(q, n_envs);
  const GmRolloutJob& J = q.job;
  unsigned long long busy = 0, poll = 0, last_end = 0;
  bool first = true;
  for (;;) {
    if (q.prio > 0) __builtin_amdgcn_s_setprio(0);   // looking for work: the partner wave first
    const unsigned long long tw = __builtin_amdgcn_s_memrealtime();
    const GmCqPick pick = cq_take_work(q, w, order, cost, lane);
    const unsigned long long tp = __builtin_amdgcn_s_memrealtime();
    poll += tp - tw;
    if (pick.env < 0) break;
    if (first && lane == 0)
      __hip_atomic_fetch_min(q.st + GM_CQT_FIRST_PICK, tp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    first = false;
    const int env = pick.env;
    uint64_t* env_t = reinterpret_cast<uint64_t*>(q.st) + cq_time_of_env(gridDim.x, env);
    if (pick.fresh && lane == 0) st_agent(env_t, tp);
    const unsigned long long t_start = __builtin_amdgcn_s_memtime();
    // lane 0's acquire load saw the entry: extend it to the whole wave's loads of the state
    if (!pick.fresh) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (EVAL && pick.fresh && J.active && !J.active[env]) {
      // an evaluation's inactive env (only ever a fresh pick: it never yields) finishes at once:
      // no state is loaded, no env-step runs, its cost slot keeps the last launch's value; the
      // diagnostics show a job of no clocks and no yields that ended when it was picked
      if (lane == 0) {
        J.ev.end[env] = 0;
        __hip_atomic_store(&q.carry[env].clk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&q.carry[env].job_yields, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        add_agent(cq_counter(q, GM_CQC_DONE), 1u);
        st_agent(env_t + 1, tp);
        __hip_atomic_fetch_max(q.st + GM_CQT_LAST_DONE, tp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      last_end = tp;
      continue;
    }
    GmEnvState* g = states + env;
    load_state(S, g, lane);
    GmChunkCarry cr;
    if (pick.fresh) {
      cr.sub_done = 0;
      cr.nsub = C->sim_steps_per_action + S.s.extra_substeps;
      cr.work_nefc = 0; cr.work_mpr = 0; cr.work_newton = 0; cr.stp_fixed = 0;
      cr.clk = 0; cr.yielded = 0; cr.step_idx = 0; cr.job_yields = 0;
      cr.steps_left = J.steps;
    } else {
      // agent-scope loads: never served by a scalar cache that the acquire does not reach
      const uint32_t* src = reinterpret_cast<const uint32_t*>(q.carry + env);
      uint32_t* dst = reinterpret_cast<uint32_t*>(&cr);
#pragma unroll
      for (int i = 0; i < (int)(sizeof(GmChunkCarry) / 4); i++) dst[i] = ld_agent(src + i);
    }
    if (lane == 0) {
      S.work_nefc = cr.work_nefc; S.work_mpr = cr.work_mpr; S.work_newton = cr.work_newton;
      S.stp_fixed = cr.stp_fixed;
    }
    GM_ENV_SYNC();
    const uint64_t own = (uint64_t)cost[env] * (uint64_t)cq_job_scale(q);   // the job's predicted cost
    const uint32_t est = (uint32_t)(own > 0xFFFFFFFFull ? 0xFFFFFFFFull : own);
    const int s_nom = C->sim_steps_per_action;
    bool finished = false;
    for (;;) {   // the env-steps of this pick
      if (cr.sub_done == 0 && J.driver >= 0) {
        // begin an env-step of a rollout: the driver's actions, applied as gm_set_action /
        // gm_set_discrete_action before gm_step (they may add the termination lift's substeps)
        const float* o = obs + (size_t)env * C->n_obs;
        if (J.driver == GM_DRV_DQN) {
          static_assert(sizeof(S.st) >= sizeof(float) * 2 * GP_ROW, "policy activations fit the union");
          const int a = gp_select_one(o, J.pparams, J.pnet, J.peps[cr.step_idx], J.seed,
                                      J.pdecision + (uint64_t)cr.step_idx, (uint64_t)rollout_gid(J, env),
                                      reinterpret_cast<float*>(&S.st), lane);
          if (J.replay) replay_record(0, J.replay, o, env, n_envs, cr.step_idx, a, nullptr, lane);
          if (lane == 0) {
            set_action_one(S.s, m, C, a, 0.0f);
            S.stp_fixed = 0;
          }
        } else if (J.driver == GM_DRV_AC || J.driver == GM_DRV_SAC) {
          static_assert(sizeof(S.st) >= sizeof(float) * GA_ONE_FLOATS, "actor-critic activations fit the union");
          // (one call for both: a call site of its own for sac_rollout_driver cost the DUO
          // instantiations N + 2 = 7 / 8 / 9 a VGPR and N + 2 = 12 DUO 16 B of scratch)
          ac_rollout_driver(J.driver == GM_DRV_SAC ? 3 : 0, J.ac, o, env, n_envs, cr.step_idx, J.max_ep,
                            rollout_gid(J, env), reinterpret_cast<float*>(&S.st), S.s, m, C, lane);
          if (lane == 0) S.stp_fixed = 0;
        } else if (lane == 0) {
          driver_actions(S.s, g->ring, m, C, J.driver, J.seed, J.jitter, rollout_gid(J, env));
          S.stp_fixed = 0;
        }
        GM_ENV_SYNC();
        cr.nsub = C->sim_steps_per_action + S.s.extra_substeps;
      }
      // run to the end of the env-step unless another env has become the longer job (whole jobs)
      const int job_left = cq_job_left(cr, s_nom), job_total = cq_job_total(q, cr, s_nom);
      const GmPreempt pre{cq_counter(q, GM_CQC_FRESH), order, cost, w.n, est, job_left, job_total,
                          cr.yielded < q.max_yields ? q.chunk : 0, q.margin, w.bq, w.cmax, q.cmargin, q.prio,
                          cq_job_scale(q)};
      job_prio((uint64_t)est * (uint64_t)job_left / (uint64_t)(job_total > 0 ? job_total : 1), w.cmax, q.prio);
      cr.sub_done += substep_loop<CL, false, false, DUO>(
          (GM_AS_LDS SharedT<CL>*)&S, (const GM_AS_GLOBAL gm_model*)m, (const GM_AS_GLOBAL GmTopo*)T,
          (const GM_AS_GLOBAL gm_config*)C, lane, false, cr.nsub - cr.sub_done, false, pre);
      if (cr.sub_done < cr.nsub) break;   // yielded
      unsigned long long t0 = 0;
      env_step_epilogue(S, m, C, T, obs, rew, done, env, lane, false, t0);
      // (an evaluation's env whose episode ended retires: this was its job's last env-step)
      if (rollout_end_step<CL, EVAL>(S, g, obs, env, n_envs, J, cr.step_idx, m, C, T, lane)) cr.steps_left = 1;
      cr.steps_left -= 1;
      cr.step_idx += 1;
      if (cr.steps_left <= 0) {
        rollout_finish<CL, EVAL>(S, g, obs, env, n_envs, J, cr.step_idx, m, C, lane);
        finished = true;
        break;
      }
      cr.sub_done = 0;
      cr.yielded = 0;
      GM_ENV_SYNC();
    }
    if (finished) {
      if (cost && lane == 0) {
        const uint32_t clk = cr.clk + (uint32_t)((__builtin_amdgcn_s_memtime() - t_start) >> 6);
        // for the next launch's order, per env-step actually run: cr.step_idx, the job's length
        // except where an evaluation's env retired early
        cost[w.n + env] = dispatch_cost(clk, (uint32_t)(EVAL ? cr.step_idx : cq_job_scale(q)), S.work_nefc, S.work_mpr,
                                        S.work_newton);
        // diagnostics (gm_chunk_job_stats): the job's busy clocks / 64 and its yields
        __hip_atomic_store(&q.carry[env].clk, clk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&q.carry[env].job_yields, cr.job_yields, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      store_state(S, g, lane);
      if (lane == 0) {
        add_agent(cq_counter(q, GM_CQC_DONE), 1u);
        st_agent(env_t + 1, __builtin_amdgcn_s_memrealtime());
        __hip_atomic_fetch_max(q.st + GM_CQT_LAST_DONE, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
      }
    } else {
      store_state(S, g, lane);
      if (lane == 0) {
        cr.work_nefc = S.work_nefc; cr.work_mpr = S.work_mpr; cr.work_newton = S.work_newton;
        cr.stp_fixed = S.stp_fixed;
        cr.yielded += 1; cr.job_yields += 1;
        cr.clk += (uint32_t)((__builtin_amdgcn_s_memtime() - t_start) >> 6);
        q.carry[env] = cr;
      }
      cq_publish_yield(q, w, own, cq_job_left(cr, s_nom), cq_job_total(q, cr, s_nom), env, lane);
    }
    GM_ENV_SYNC();   // LDS image reused by the next pick
    last_end = __builtin_amdgcn_s_memrealtime();
    busy += last_end - tp;
  }
  if (lane == 0) {
    __hip_atomic_fetch_add(q.st + GM_CQT_BUSY, busy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(q.st + GM_CQT_POLL, poll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // this workgroup's last work (gm_chunk_timeline), its XCD in the top four bits
    st_agent(reinterpret_cast<uint64_t*>(q.st) + cq_time_of_wave(blockIdx.x), last_end | ((uint64_t)w.xcc << 60));
  }
}
