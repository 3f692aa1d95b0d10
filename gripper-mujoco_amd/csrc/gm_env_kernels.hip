// gm_env_kernels.hip -- the thread-per-env and wave-per-env kernels around the env-step:
// dispatch order, actions, the synthetic drivers, spawns, resets, small setters and getters.
// Only gm_capi.hip includes it: the calibration unit launches none of them.
#pragma once
#include "gm_kernels.hip"

// Dispatch order for the next env-step: envs by descending cost of their last env-step
// (shader clocks / 64, written by gm_step_kernel), bucketed into 256 cost classes.
// One 1024-thread workgroup; the order only changes which env a workgroup slot runs
// first, never any result.
extern "C" __global__ __launch_bounds__(1024) void gm_dispatch_order_kernel(uint32_t* __restrict__ cost,
                                                                            int32_t* __restrict__ order, int n,
                                                                            uint32_t* __restrict__ chunk_ctr,
                                                                            unsigned long long* __restrict__ chunk_st) {
  __shared__ uint32_t cnt[256];
  __shared__ uint32_t cmax;
  const int t = threadIdx.x;
  if (chunk_ctr && t < GM_CQC_N) chunk_ctr[GM_CQ_LAST + t] = chunk_ctr[GM_CQ_FRESH + t];   // last launch's, for diagnostics
  __syncthreads();
  if (chunk_ctr)
    for (int w = t; w < GM_CQ_WORDS; w += 1024) chunk_ctr[w] = 0;   // the chunked launch's queue counters
  if (chunk_st && t < GM_CQT_LAST) {
    chunk_st[GM_CQT_LAST + t] = chunk_st[t];
    chunk_st[t] = (t == GM_CQT_FIRST_PICK || t == GM_CQT_FIRST_EMPTY) ? ~0ull : 0ull;   // (fetch_min targets)
  }
  if (t < 256) cnt[t] = 0;
  if (t == 0) cmax = 1;
  __syncthreads();
  uint32_t m = 1;
  for (int i = t; i < n; i += 1024) {
    const uint32_t c = cost[n + i];   // the costs the last launch recorded become current
    cost[i] = c;
    m = max(m, c);
  }
  atomicMax(&cmax, m);
  __syncthreads();
  const uint64_t cm = (uint64_t)cmax + 1;
  if (chunk_ctr && t == 0) chunk_ctr[GM_CQ_FRESH + GM_CQC_CMAX] = (uint32_t)cm;
  for (int i = t; i < n; i += 1024) {
    const int b = 255 - (int)(((uint64_t)cost[i] * 256) / cm);
    atomicAdd(&cnt[b], 1u);
  }
  __syncthreads();
  {
    // exclusive prefix over the 256 buckets: shuffle scans in the first four waves, then
    // each wave's offset from the wave totals (a serial loop on one thread took ~10 us)
    __shared__ uint32_t wsum[4];
    const uint32_t v = (t < 256) ? cnt[t] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(inc, o);
      if ((t & 63) >= o) inc += u;
    }
    if (t < 256 && (t & 63) == 63) wsum[t >> 6] = inc;
    __syncthreads();
    if (t < 256) {
      uint32_t base = 0;
      for (int w = 0; w < (t >> 6); w++) base += wsum[w];
      cnt[t] = base + inc - v;
    }
  }
  __syncthreads();
  for (int i = t; i < n; i += 1024) {
    const int b = 255 - (int)(((uint64_t)cost[i] * 256) / cm);
    order[atomicAdd(&cnt[b], 1u)] = i;
  }
}

extern "C" __global__ void gm_action_kernel(GmEnvState* __restrict__ states, const gm_model* __restrict__ m,
                                            const gm_config* __restrict__ C, const float* __restrict__ cont,
                                            const int32_t* __restrict__ disc, int n_envs) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs) return;
  GmEnvState& s = states[env];
  if (cont) {
    for (int i = 0; i < C->n_actions; i++) {
      float f = cont[(size_t)env * C->n_actions + i];
      if (f < -1.0f) f = -1.0f; else if (f > 1.0f) f = 1.0f;
      set_action_one(s, m, C, i, f);
    }
  } else {
    set_action_one(s, m, C, disc[env], 0.0f);
  }
}

// ---------------------------------------------------------------- scripted grasp mix
// The benchmark's / parity tests' synthetic driver (gmx.GraspScript mirrors it on the
// host bit for bit): per env and episode, phase lengths drawn from the counter-based
// hash (seed, global env id, episode) -- close the fingers, squeeze (tilt the tips), press
// the palm, lift the base -- indexed by the env's own episode step (num_action_steps),
// plus uniform jitter per (step, action).  Continuous action fractions in [-1, 1] for
// the in-use actions (MjClass::set_continous_action order).
// the driver's actions for the current state of every env (gm_scripted_actions, gm_random_actions,
// gm_program_actions), thread per env: the first loop of driver_actions written to memory, in
// mode GM_DRV_SCRIPT, _RANDOM (U[-1, 1) per (env, episode, episode step, action) from the
// counter-based hash, gm_state.h), _PROGRAM or _MIX
extern "C" __global__ void gm_driver_action_kernel(const GmEnvState* __restrict__ states, const gm_model* __restrict__ m,
                                                   const gm_config* __restrict__ C, float* __restrict__ out, int n_envs,
                                                   uint64_t seed, long long env_offset, float jitter, int mode) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs) return;
  const GmEnvState& s = states[env];
  const int na = C->n_actions;
  for (int i = 0; i < na; i++) {
    const float v = driver_fraction(s, const_cast<RingRef>(s.ring), m, C, mode, seed, jitter, env_offset + env, i,
                                    action_kind(C->action_options[i]));
    out[(size_t)env * na + i] = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
  }
}

extern "C" __global__ void gm_spawn_into_scene_kernel(GmEnvState* __restrict__ states, const gm_model* __restrict__ m,
                                                      const GmTopo* __restrict__ T, const gm_object* __restrict__ objs,
                                                      int n_objects, const uint8_t* __restrict__ mask,
                                                      const gm_spawn_params* __restrict__ params, int n_params,
                                                      uint8_t* __restrict__ ok, int n_envs) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs) return;
  if (mask && !mask[env]) { if (ok) ok[env] = 0; return; }
  const gm_spawn_params p = params[n_params == 1 ? 0 : env];
  uint16_t pxy[GM_SPAWN_MAX_XY], prot[GM_SPAWN_MAX_ROT];
  const int r = spawn_into_scene_dev(states[env], m, T, objs, n_objects, p, p.index, pxy, prot);
  if (ok) ok[env] = (uint8_t)r;
}

// MjEnv auto-reset bookkeeping (MjEnv.py:616-637, 2170-2263): an env whose episode
// terminated (is_done) or truncated (num_action_steps >= max_episode_steps) hands its
// episode return to `returns` and is flagged for gm_reset_kernel.
extern "C" __global__ void gm_autoreset_mask_kernel(const GmEnvState* __restrict__ states,
                                                    const uint8_t* __restrict__ done, int max_steps,
                                                    uint8_t* __restrict__ mask, float* __restrict__ returns,
                                                    gm_episode_end* __restrict__ episodes, int n_envs) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs) return;
  const GmEnvState& s = states[env];
  const int end = gm_episode_end_code(done[env], s.num_action_steps, max_steps);
  mask[env] = end ? 1 : 0;
  const gm_episode_end e = gm_episode_end_record(end, s.cumulative_reward, s.num_action_steps,
                                                 s.bev_last[GM_EV_successful_grasp]);
  if (returns) returns[env] = e.ret;
  if (episodes) episodes[env] = e;
}

// gm_eval_record, one wave per env: a still-active env whose episode has ended writes its test
// report (eval_report, the evaluation launch's own) and clears its active byte.  init != 0 is the
// entry points' first call, before any env-step: every inactive env's end becomes 0, nothing else.
extern "C" __global__ __launch_bounds__(64) void gm_eval_record_kernel(const GmEnvState* __restrict__ states,
                                                                       const uint8_t* __restrict__ done, int max_steps,
                                                                       uint8_t* __restrict__ active, gm_eval_out out,
                                                                       int n_envs, int init) {
  const int env = blockIdx.x;
  if (env >= n_envs) return;
  const int lane = threadIdx.x;
  if (init) {
    if (lane == 0 && !active[env]) out.end[env] = 0;
    return;
  }
  if (!active[env]) return;
  const GmEnvState& s = states[env];
  const int end = gm_episode_end_code(done[env], s.num_action_steps, max_steps);
  if (!end) return;
  eval_report(s, out, env, end, lane);
  __syncthreads();   // every lane has read the byte before lane 0 clears it
  if (lane == 0) active[env] = 0;
}

// One wave per env (grid = n_envs workgroups of 64; unmasked envs exit at once): the new
// record's hot part is built in LDS (lane 0's serial reset reads back what it wrote many
// times over) and stored to HBM in one coalesced sweep; the sensor windows are cleared in
// place.
extern "C" __global__ __launch_bounds__(64) void gm_reset_kernel(
    GmEnvState* __restrict__ states, const gm_model* __restrict__ m, const gm_config* __restrict__ C,
    const GmTopo* __restrict__ T, const double* __restrict__ eq_qpos, const uint8_t* __restrict__ mask,
    const gm_spawn* __restrict__ spawn, const gm_object* __restrict__ objs, int n_objects, int n_envs,
    const gm_spawn_params* __restrict__ scene, int scene_tries, float* __restrict__ obs, GmSpawnRand sr) {
  __shared__ uint16_t sh_pxy[GM_SPAWN_MAX_XY], sh_prot[GM_SPAWN_MAX_ROT];   // spawn grid shuffles
  const int env = blockIdx.x;
  if (env >= n_envs) return;
  if (mask && !mask[env]) return;
  __shared__ uint4 hot_words[GM_HOT_WORDS / 4];
  GmEnvHot& s = *reinterpret_cast<GmEnvHot*>(hot_words);
  GmEnvState& rec = states[env];
  // keep the per-env RNG stream and the function-static stepper flags (quirk)
  const GmResetKeep keep{rec.rng, rec.old_x, rec.old_y, rec.old_z, rec.episode + 1, rec.newton_caps};
  reset_env(s, rec, keep, m, C, T, eq_qpos, spawn, objs, n_objects, env, scene, scene_tries, sr, sh_pxy, sh_prot,
            (int)threadIdx.x);
  // MjEnv.reset returns _next_observation() of the fresh episode (MjEnv.py:2222-2263):
  // the observation buffer holds the reset env's sensor windows, not the last episode's;
  // sampled one stream per lane as in the env-step epilogue
  {
    uint4* w = reinterpret_cast<uint4*>(&rec);
    for (int i = threadIdx.x; i < GM_HOT_WORDS / 4; i += 64) w[i] = hot_words[i];
  }
  if (obs) get_obs_lanes(s, rec.ring, C, obs + (size_t)env * C->n_obs, threadIdx.x);
}

// settle initialisation (keyframe, targets home, locks off, flags true) for env 0
extern "C" __global__ void gm_settle_init_kernel(GmEnvState* __restrict__ states, const gm_model* __restrict__ m,
                                                 const GmTopo* __restrict__ T, const gm_object* __restrict__ objs) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  GmEnvState& s = states[0];
  uint32_t* w = reinterpret_cast<uint32_t*>(&s);
  for (int i = 0; i < GM_STATE_WORDS; i++) w[i] = 0;
  g_reset(s.end); g_reset(s.next);
  for (int k = 0; k < GM_MAX_QPOS; k++) s.qpos[k] = m->qpos0[k];
  s.dt = m->timestep;
  s.old_x = s.old_y = s.old_z = 1;
  for (int st = 0; st < GM_NSTREAM; st++) s.ring_i[st] = -1;
  const gm_object& o = objs[0];
  s.obj_type = o.type;
  s.obj_size[0] = o.size[0]; s.obj_size[1] = o.size[1]; s.obj_size[2] = o.size[2];
  s.obj_mass = o.mass;
  s.obj_friction = o.friction;
  if (o.type == GM_GEOM_BOX) {
    double a = 2 * o.size[0], bb = 2 * o.size[1], c = 2 * o.size[2];
    s.obj_inertia[0] = (o.mass * (bb * bb + c * c) / 12); s.obj_inertia[1] = (o.mass * (a * a + c * c) / 12);
    s.obj_inertia[2] = (o.mass * (a * a + bb * bb) / 12);
    s.obj_rbound = sqrt(o.size[0] * o.size[0] + o.size[1] * o.size[1] + o.size[2] * o.size[2]);
  } else if (o.type == GM_GEOM_CYLINDER) {
    double r = o.size[0], hh = 2 * o.size[1];
    s.obj_inertia[0] = s.obj_inertia[1] = (o.mass * (3 * r * r + hh * hh) / 12);
    s.obj_inertia[2] = (o.mass * r * r / 2);
    s.obj_rbound = sqrt(o.size[0] * o.size[0] + o.size[1] * o.size[1]);
  } else {
    double r = o.size[0];
    s.obj_inertia[0] = s.obj_inertia[1] = s.obj_inertia[2] = (2 * o.mass * r * r / 5);
    s.obj_rbound = r;
  }
  s.obj_invw[0] = 1.0 / o.mass;
  s.obj_invw[1] = ((1.0 / s.obj_inertia[0] + 1.0 / s.obj_inertia[1]) + 1.0 / s.obj_inertia[2]) / 3.0;
}

// per-env initialisation after the settle: RNG seeds and settled stepper flags
extern "C" __global__ void gm_init_envs_kernel(GmEnvState* __restrict__ states, uint32_t base_seed, long long env_offset,
                                               int n_envs, double dt) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs) return;
  GmEnvState& s = states[env];
  s.dt = dt;
  uint64_t seed = ((uint64_t)base_seed + (uint64_t)(env_offset + env) * 1000003ull) % 2147483647ull;
  s.rng = seed == 0 ? 1u : (uint32_t)seed;
  s.old_x = s.old_y = s.old_z = 0;
}

// MjClass::set_motor_target -> Gripper::set_xyz_m on the env's target (thread per env)
extern "C" __global__ void gm_motor_target_kernel(GmEnvState* __restrict__ states, const uint8_t* __restrict__ mask,
                                                  const double* __restrict__ xyz, int per_env,
                                                  uint8_t* __restrict__ in_limits, int n_envs) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs) return;
  if (mask && !mask[env]) return;
  const double* t = xyz + (per_env ? 3 * env : 0);
  in_limits[env] = (uint8_t)g_set_xyz_m(states[env].end, t[0], t[1], t[2]);
}
// the latest sim_sensors_SI_ readings (finger 1..3 gauges, palm, wrist Z), thread per env
extern "C" __global__ void gm_sensor_si_kernel(const GmEnvState* __restrict__ states, float* __restrict__ out, int n_envs) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs) return;
  const GmEnvState& s = states[env];
  RingRef R = const_cast<RingRef>(s.ring);
  const int st[5] = {ST_SI_GAUGE, ST_SI_GAUGE + 1, ST_SI_GAUGE + 2, ST_SI_PALM, ST_SI_WZ};
  for (int k = 0; k < 5; k++) out[5 * env + k] = ring_latest(s, R, st[k]);
}
// spawn only (MjClass::spawn_object after MjClass::reset, MjEnv.py:1212-1267)
extern "C" __global__ void gm_spawn_kernel(GmEnvState* __restrict__ states, const GmTopo* __restrict__ T,
                                           const uint8_t* __restrict__ mask, const gm_spawn* __restrict__ spawn,
                                           const gm_object* __restrict__ objs, int n_objects, int n_envs) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs) return;
  if (mask && !mask[env]) return;
  spawn_object(states[env], T, objs, n_objects, spawn[env]);
}
