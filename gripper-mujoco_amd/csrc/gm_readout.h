// gm_readout.h -- the env-step readout after the substeps: sense_gripper_state, update_env,
// the observation samplers, is_done, reward (mjclass.cpp:1483-1508, MjEnv.py:2170-2220) and the
// hot state's HBM <-> LDS moves.  SharedT: reads s, forces, overflow, gs; writes s, gs.
#pragma once
#include "gm_gripper.h"
#include "gm_sensors.h"

// ============================================================ env-step epilogue (lane 0)
__device__ __forceinline__ float normalise_between(float val, float mn, float mx) {
  if (val > mx) return 1.0f;
  else if (val < mn) return -1.0f;
  return 2 * (val - mn) / (mx - mn) - 1;
}

template <int CL>
GM_EPI_ATTR void sense_gripper_state(SharedT<CL>& S, const gm_model* __restrict__ m, const gm_config* __restrict__ C) {
  GmEnvHot& s = S.s;
  RingRef R = S.gs->ring;
  const gm_settings& st = C->s;
  const double* bmn = C->base_min;
  const double* bmx = C->base_max;
  double gx = normalise_between((float)s.end.x, (float)G_XY_MIN, (float)G_XY_MAX);
  double gy = normalise_between((float)s.end.y, (float)G_XY_MIN, (float)G_XY_MAX);
  double gz = normalise_between((float)s.end.z, (float)G_Z_MIN, (float)G_Z_MAX);
  double bx = normalise_between((float)s.base[0], (float)bmn[0], (float)bmx[0]);
  double by = normalise_between((float)s.base[1], (float)bmn[1], (float)bmx[1]);
  double bz = normalise_between((float)s.base[2], (float)bmn[2], (float)bmx[2]);
  double byaw = normalise_between((float)s.base[5], (float)bmn[5], (float)bmx[5]);
  gx = s_noise(s, st.motor_state_sensor, SL_MOTOR, (float)gx, 1);
  gy = s_noise(s, st.motor_state_sensor, SL_MOTOR, (float)gy, 2);
  gz = s_noise(s, st.motor_state_sensor, SL_MOTOR, (float)gz, 3);
  bx = s_noise(s, st.base_state_sensor_XY, SL_BASEXY, (float)bx, 1);
  by = s_noise(s, st.base_state_sensor_XY, SL_BASEXY, (float)by, 2);
  bz = s_noise(s, st.base_state_sensor_Z, SL_BASEZ, (float)bz, 1);
  byaw = s_noise(s, st.base_state_sensor_yaw, SL_YAW, (float)byaw, 1);
  ring_add(s, R, ST_MOTOR + 0, (float)gx);
  ring_add(s, R, ST_MOTOR + 1, (float)gy);
  ring_add(s, R, ST_MOTOR + 2, (float)gz);
  ring_add(s, R, ST_BASE + 0, (float)bx);
  ring_add(s, R, ST_BASE + 1, (float)by);
  ring_add(s, R, ST_BASE + 2, (float)bz);
  ring_add(s, R, ST_YAW, (float)byaw);
  // MAT cartesian contact points (get_fingerend_and_palm_xyz, myfunctions.cpp:3622-3688)
  double fsi[3] = {ring_latest(s, R, ST_SI_GAUGE), ring_latest(s, R, ST_SI_GAUGE + 1), ring_latest(s, R, ST_SI_GAUGE + 2)};
  double psi = ring_latest(s, R, ST_SI_PALM);
  double fx = s.end.x, fth = g_calc_th(s.end.x, s.end.y), pz = s.end.z;
  const double PI23 = 3.14159265358979323846 * (2.0 / 3.0);
  double ang[3] = {0.0, PI23, 2 * PI23};
  double unt = m->fingertip_clearance - s.base[2];
  double lift = m->finger_length * (1 - cos(fth));
  double tilted = unt + lift;
  const double ft = 0.2;
  for (int i = 0; i < 3; i++) {
    double tilt_x = fx - m->finger_length * sin(fth);
    double defl = fsi[i] * pow(m->finger_length, 3) / (3 * m->finger_EI);
    double fin_x = tilt_x + defl * cos(fth);
    double px = -fin_x * sin(ang[i] + s.base[5]) + s.base[0];
    double py = -fin_x * cos(ang[i] + s.base[5]) + s.base[1];
    double pzz = tilted - defl * sin(fth);
    bool on = fabs(fsi[i]) > ft;
    ring_add(s, R, ST_CART + 3 * i + 0, (float)(on ? px : 0.0));
    ring_add(s, R, ST_CART + 3 * i + 1, (float)(on ? py : 0.0));
    ring_add(s, R, ST_CART + 3 * i + 2, (float)(on ? pzz : 0.0));
  }
  bool pon = psi > ft;
  ring_add(s, R, ST_CART + 9, (float)(pon ? s.base[0] : 0.0));
  ring_add(s, R, ST_CART + 10, (float)(pon ? s.base[1] : 0.0));
  ring_add(s, R, ST_CART + 11, (float)(pon ? unt + 165e-3 - pz : 0.0));
}

__device__ float mag3f(const float* v) { return (float)sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); }

// MjClass::update_env (mjclass.cpp:966-1346) + update_events (5437-5469)
template <int CL>
GM_EPI_ATTR void update_env(SharedT<CL>& S, const gm_model* __restrict__ m, const gm_config* __restrict__ C,
                           const GmTopo* __restrict__ T) {
  GmEnvHot& s = S.s;
  RingRef R = S.gs->ring;
  const gm_settings& st = C->s;
  const double ftol = 1e-5;
  extract_forces(S, m, T);
  const float* F = S.forces;
  int qa = T->qadr_obj;
  double ox = s.qpos[qa], oy = s.qpos[qa + 1], oz = s.qpos[qa + 2];
  double relx = s.base[0] - ox, rely = s.base[1] - oy;
  float dist_from_gripper = (float)sqrt(pow(relx, 2) + pow(rely, 2));
  float f1m = mag3f(F + 0), f2m = mag3f(F + 3), f3m = mag3f(F + 6), pm = mag3f(F + 9), gm = mag3f(F + 12);
  float palm_axial = F[9];
  float lift_height = (float)(oz - (double)s.start_qpos[2]);
  float avg_finger = (float)(0.33333 * (f1m + f2m + f3m));
  float mn = F[1];
  if (F[4] < mn) mn = F[4];
  if (F[7] < mn) mn = F[7];
  float peak_lat = -1 * mn;
  float ov_avg = 0, ov_palm = 0, ov_lift = 0;
  if (avg_finger > ov_avg) ov_avg = avg_finger;
  if (palm_axial > ov_palm) ov_palm = palm_axial;
  if (peak_lat > s.grp_peak_lateral) s.grp_peak_lateral = peak_lat;
  if (lift_height > ov_lift) ov_lift = lift_height;
  float gripper_z_height = (float)(-1 * s.base[2]);
  float ga = F[19];
  if (F[20] < ga) ga = F[20];
  if (F[21] < ga) ga = F[21];
  float grp_peak_axial = -1 * ga;
  float g1 = ring_latest(s, R, ST_SI_GAUGE), g2 = ring_latest(s, R, ST_SI_GAUGE + 1), g3 = ring_latest(s, R, ST_SI_GAUGE + 2);
  float last_palm = ring_latest(s, R, ST_SI_PALM), last_wrist = ring_latest(s, R, ST_SI_WZ);
  float max_gauge = g1 > g2 ? g1 : g2;
  max_gauge = max_gauge > g3 ? max_gauge : g3;
  float avg_gauge = (float)((1.0 / 3.0) * (g1 + g2 + g3));
  int* B = s.bev_value;
  B[GM_EV_step_num] = 1;
  double closest = dist_from_gripper;
  int o_lifted = 0, o_oob = 0, o_l2h = 0, o_th = 0, o_stable = 0;
  if (gm < ftol && 0.0f < ftol) { B[GM_EV_lifted] = 1; o_lifted = 1; }
  if (ox > st.oob_distance || ox < -st.oob_distance || oy > st.oob_distance || oy < -st.oob_distance) { B[GM_EV_oob] = 1; o_oob = 1; }
  if (ov_lift > st.lift_height - ftol && o_lifted && !o_oob) { B[GM_EV_lifted_to_height] = 1; o_l2h = 1; }
  if (o_l2h && gripper_z_height > st.gripper_target_height - ftol) { B[GM_EV_target_height] = 1; o_th = 1; }
  if (f1m > ftol || f2m > ftol || f3m > ftol || pm > ftol) B[GM_EV_object_contact] = 1;
  if (f1m > st.stable_finger_force && f2m > st.stable_finger_force && f3m > st.stable_finger_force &&
      f1m < st.stable_finger_force_lim && f2m < st.stable_finger_force_lim && f3m < st.stable_finger_force_lim &&
      pm > st.stable_palm_force && pm < st.stable_palm_force_lim && B[GM_EV_lifted]) {
    B[GM_EV_object_stable] = 1; o_stable = 1;
  }
  if (o_stable && o_th) B[GM_EV_stable_height] = 1;
  if (s.termination_signal_sent) {
    if (st.lifted_termination.done) {
      if (o_l2h) B[GM_EV_lifted_termination] = 1; else B[GM_EV_failed_termination] = 1;
    } else {
      if (B[GM_EV_stable_height]) B[GM_EV_stable_termination] = 1; else B[GM_EV_failed_termination] = 1;
    }
  }
  if (dist_from_gripper < st.XY_distance_threshold) B[GM_EV_within_XY_distance] = 1;
  if (dist_from_gripper < closest) closest = dist_from_gripper;
  {
    int* R = s.bev_row;
    int v = (!R[GM_EV_dropped] * !B[GM_EV_lifted] * R[GM_EV_lifted]) ? 1
            : (B[GM_EV_lifted] ? 0 : (R[GM_EV_dropped] ? R[GM_EV_dropped] + 1 : 0));
    B[GM_EV_dropped] = v != 0;
  }
  float* Lv = s.lev_value;
  Lv[GM_LEV_exceed_axial] = grp_peak_axial;
  Lv[GM_LEV_exceed_lateral] = s.grp_peak_lateral;
  Lv[GM_LEV_palm_force] = ov_palm * B[GM_EV_lifted];
  Lv[GM_LEV_exceed_palm] = ov_palm;
  Lv[GM_LEV_finger_force] = ov_avg;
  Lv[GM_LEV_finger1_force] = f1m;
  Lv[GM_LEV_finger2_force] = f2m;
  Lv[GM_LEV_finger3_force] = f3m;
  Lv[GM_LEV_ground_force] = gm;
  Lv[GM_LEV_good_bend_sensor] = avg_gauge;
  Lv[GM_LEV_exceed_bend_sensor] = max_gauge;
  Lv[GM_LEV_dangerous_bend_sensor] = max_gauge;
  Lv[GM_LEV_good_palm_sensor] = last_palm;
  Lv[GM_LEV_exceed_palm_sensor] = last_palm;
  Lv[GM_LEV_dangerous_palm_sensor] = last_palm;
  Lv[GM_LEV_exceed_wrist_sensor] = last_wrist;
  Lv[GM_LEV_dangerous_wrist_sensor] = last_wrist;
  Lv[GM_LEV_action_penalty_lin] /= (float)(C->n_actions - st.use_termination_action);
  Lv[GM_LEV_action_penalty_sq] /= (float)(C->n_actions - st.use_termination_action);
  Lv[GM_LEV_object_XY_distance] = (float)(-closest);
  {
    int k = 0;
#define GM_BR(n, r, d, t)                                                                         \
    if (B[k] && st.n.reward >= (1.0 - 1e-5) && st.n.done && s.bev_row[k] + 1 >= st.n.trigger)    \
      B[GM_EV_successful_grasp] = 1;                                                              \
    k++;
#include "gm_settings.def"
  }
  // update_events
  for (int k = 0; k < GM_N_BINARY; k++) {
    s.bev_row[k] = s.bev_row[k] * s.bev_value[k] + s.bev_value[k];
    s.bev_abs[k] += s.bev_value[k];
    s.bev_last[k] = s.bev_value[k];
    s.bev_value[k] = 0;
  }
  {
    int k = 0;
#define GM_LR(n, r, d, t, a, b, o)                                                         \
    {                                                                                      \
      int active = (Lv[k] > st.n.min && (Lv[k] < st.n.overshoot || st.n.overshoot < 0));   \
      s.lev_row[k] = s.lev_row[k] * active + active;                                       \
      s.lev_abs[k] += active;                                                              \
      s.lev_last[k] = Lv[k];                                                               \
      Lv[k] = 0.0f;                                                                        \
    }                                                                                      \
    k++;
#include "gm_settings.def"
  }
}

__device__ int sample_stream(const GmEnvHot& s, RingRef R, int mode, int st, const gm_sensor& ss, float* out) {
  int prev = ss.prev_steps, rps = ss.readings_per_step, total = ss.total_readings;
  if (mode == GM_SAMPLE_RAW) {
    int n = total - 1;
    for (int j = n - 1, k = 0; j >= 0; j--, k++) out[k] = ring_read(s, R, st, j);
    return n;
  }
  out[0] = ring_read(s, R, st, total - 1);
  for (int i = 0; i < prev; i++) {
    int first = total - 1 - i * rps;
    out[2 * i + 2] = ring_read(s, R, st, first - rps);
    float a = out[2 * i], b = out[2 * i + 2];
    float r;
    if (mode == GM_SAMPLE_CHANGE) r = b - a;
    else if (mode == GM_SAMPLE_AVERAGE) {
      float acc = 0;
      for (int j = 0; j < rps + 1; j++) acc += ring_read(s, R, st, first - j);
      r = acc / (rps + 1);
    } else if (mode == GM_SAMPLE_MEDIAN) {
      float v[GM_RING + 1];
      int nv = rps + 1;
      for (int j = 0; j < nv; j++) v[j] = ring_read(s, R, st, first - j);
      for (int x = 1; x < nv; x++) { float t = v[x]; int y = x - 1; while (y >= 0 && v[y] > t) { v[y + 1] = v[y]; y--; } v[y + 1] = t; }
      int hn = nv / 2;
      float med = v[hn];
      if (!(nv & 1)) med = (v[hn - 1] + med) / 2.0f;
      r = med;
    } else if (mode == GM_SAMPLE_SIGN) {
      float ch = b - a;
      r = ch > 1e-6f ? 1.0f : (ch < -1e-6f ? -1.0f : 0.0f);
    } else if (mode == GM_SAMPLE_SCALED_CHANGE) {
      float sc = (b - a) / 0.07f;
      r = sc > 1.0f ? 1.0f : (sc < -1.0f ? -1.0f : sc);
    } else {
      float ch = fabsf(b - a);
      float sc = (b - a) * ch * (1.0f / (0.10f * 0.10f));
      r = sc > 1.0f ? 1.0f : (sc < -1.0f ? -1.0f : sc);
    }
    out[2 * i + 1] = r;
  }
  return 2 * prev + 1;
}

// MjClass::get_observation (mjclass.cpp:1707-1959)
__device__ int get_obs(const GmEnvHot& s, RingRef R, const gm_config* __restrict__ C, float* out) {
  const gm_settings& st = C->s;
  int sf = C->sensor_fcn, tf = C->state_fcn, n = 0;
  if (st.bending_gauge.in_use) for (int f = 0; f < 3; f++) n += sample_stream(s, R, sf, ST_GAUGE + f, st.bending_gauge, out + n);
  if (st.axial_gauge.in_use) for (int f = 0; f < 3; f++) n += sample_stream(s, R, sf, ST_AXIAL + f, st.axial_gauge, out + n);
  if (st.palm_sensor.in_use) n += sample_stream(s, R, sf, ST_PALM, st.palm_sensor, out + n);
  if (st.wrist_sensor_XY.in_use) {
    n += sample_stream(s, R, sf, ST_WX, st.wrist_sensor_XY, out + n);
    n += sample_stream(s, R, sf, ST_WY, st.wrist_sensor_XY, out + n);
  }
  if (st.wrist_sensor_Z.in_use) n += sample_stream(s, R, sf, ST_WZ, st.wrist_sensor_XY, out + n);
  if (st.motor_state_sensor.in_use) for (int k = 0; k < 3; k++) n += sample_stream(s, R, tf, ST_MOTOR + k, st.motor_state_sensor, out + n);
  if (st.base_state_sensor_XY.in_use) for (int k = 0; k < 2; k++) n += sample_stream(s, R, tf, ST_BASE + k, st.base_state_sensor_XY, out + n);
  if (st.base_state_sensor_Z.in_use) n += sample_stream(s, R, tf, ST_BASE + 2, st.base_state_sensor_Z, out + n);
  if (st.base_state_sensor_yaw.in_use) n += sample_stream(s, R, tf, ST_YAW, st.base_state_sensor_yaw, out + n);
  if (st.cartesian_contacts_XYZ.in_use)
    for (int k = 0; k < 12; k++) n += sample_stream(s, R, GM_SAMPLE_CHANGE, ST_CART + k, st.cartesian_contacts_XYZ, out + n);
  return n;
}

// get_obs with one stream per lane (the env-step epilogue): every lane walks the same
// in-use stream list, in get_obs's order, to find its stream's sampler, settings and
// output offset, then all streams are sampled at once -- the serial version's arithmetic
// per stream, without its chain of dependent window reads on one lane.
__device__ void get_obs_lanes(const GmEnvHot& s, RingRef R, const gm_config* __restrict__ C, float* out, int lane) {
  const gm_settings& st = C->s;
  const int sf = C->sensor_fcn, tf = C->state_fcn;
  int k = 0, n = 0, my_mode = 0, my_st = -1, my_n = 0;
  const gm_sensor* my_ss = nullptr;
  auto visit = [&](bool in_use, int count, int mode, int st0, const gm_sensor& ss) {
    if (!in_use) return;
    const int size = (mode == GM_SAMPLE_RAW) ? ss.total_readings - 1 : 2 * ss.prev_steps + 1;
    for (int c = 0; c < count; c++) {
      if (k == lane) { my_mode = mode; my_st = st0 + c; my_ss = &ss; my_n = n; }
      n += size;
      k++;
    }
  };
  visit(st.bending_gauge.in_use, 3, sf, ST_GAUGE, st.bending_gauge);
  visit(st.axial_gauge.in_use, 3, sf, ST_AXIAL, st.axial_gauge);
  visit(st.palm_sensor.in_use, 1, sf, ST_PALM, st.palm_sensor);
  visit(st.wrist_sensor_XY.in_use, 1, sf, ST_WX, st.wrist_sensor_XY);
  visit(st.wrist_sensor_XY.in_use, 1, sf, ST_WY, st.wrist_sensor_XY);
  visit(st.wrist_sensor_Z.in_use, 1, sf, ST_WZ, st.wrist_sensor_XY);   // XY's counts (quirk, as get_obs)
  visit(st.motor_state_sensor.in_use, 3, tf, ST_MOTOR, st.motor_state_sensor);
  visit(st.base_state_sensor_XY.in_use, 2, tf, ST_BASE, st.base_state_sensor_XY);
  visit(st.base_state_sensor_Z.in_use, 1, tf, ST_BASE + 2, st.base_state_sensor_Z);
  visit(st.base_state_sensor_yaw.in_use, 1, tf, ST_YAW, st.base_state_sensor_yaw);
  visit(st.cartesian_contacts_XYZ.in_use, 12, GM_SAMPLE_CHANGE, ST_CART, st.cartesian_contacts_XYZ);
  if (my_st >= 0) sample_stream(s, R, my_mode, my_st, *my_ss, out + my_n);
}

GM_EPI_ATTR int is_done(const GmEnvHot& s, const gm_config* __restrict__ C) {
  const gm_settings& st = C->s;
  int k = 0;
  int done = 0;
#define GM_BR(n, r, d, t) if (st.n.done && s.bev_row[k] >= st.n.done) done = 1; k++;
#include "gm_settings.def"
  k = 0;
#define GM_LR(n, r, d, t, a, b, o) if (st.n.done && s.lev_row[k] >= st.n.done) done = 1; k++;
#include "gm_settings.def"
  if (st.cap_reward && st.quit_if_cap_exceeded) {
    if (s.cumulative_reward - 1e-5 < st.reward_cap_lower_bound) done = 1;
    if (s.cumulative_reward + 1e-5 > st.reward_cap_upper_bound) done = 1;
  }
  return done;
}

__device__ float linear_reward(float val, float mn, float mx, float overshoot) {
  if (val < mn) return 0.0f;
  if (val > mx) {
    if (overshoot < mx) return 1.0f;
    if (val > overshoot) return 0.0f;
    mn = 0; mx = overshoot - mx; val = overshoot - val;
  }
  return (val - mn) / (mx - mn);
}
__device__ float reward(GmEnvHot& s, const gm_config* __restrict__ C) {
  const gm_settings& st = C->s;
  float r = 0;
  int k = 0;
#define GM_BR(n, rr, d, t) if (s.bev_row[k] >= st.n.trigger) r += st.n.reward; k++;
#include "gm_settings.def"
  k = 0;
#define GM_LR(n, rr, d, t, a, b, o)                                                        \
  if (s.lev_row[k] >= st.n.trigger) {                                                      \
    float fr = linear_reward(s.lev_last[k], st.n.min, st.n.max, st.n.overshoot);           \
    r += st.n.reward * fr;                                                                 \
  }                                                                                        \
  k++;
#include "gm_settings.def"
  s.cumulative_reward += r;
  if (s.cumulative_reward < st.reward_cap_lower_bound && st.cap_reward) {
    r += st.reward_cap_lower_bound - s.cumulative_reward;
    s.cumulative_reward = st.reward_cap_lower_bound;
  }
  if (s.cumulative_reward > st.reward_cap_upper_bound && st.cap_reward) {
    r += st.reward_cap_upper_bound - s.cumulative_reward;
    s.cumulative_reward = st.reward_cap_upper_bound;
  }
  return r;
}

// action_step's tail after the substeps: sense_gripper_state, update_env, the observation,
// is_done and reward (mjclass.cpp:1483-1508, MjEnv.py:2170-2220)
template <int CL>
__device__ __forceinline__ void env_step_epilogue(SharedT<CL>& S, const gm_model* __restrict__ m,
                                                  const gm_config* __restrict__ C, const GmTopo* __restrict__ T,
                                                  float* __restrict__ obs, float* __restrict__ rew,
                                                  uint8_t* __restrict__ done, int env, int lane, bool prof,
                                                  unsigned long long& t0) {
  if (lane == 0) {
    S.s.extra_substeps = 0;
    S.s.overflow = S.overflow;
    sense_gripper_state(S, m, C);
    PH(18);
    update_env(S, m, C, T);
    PH(19);
    S.s.num_action_steps += 1;
  }
  GM_WAVE_SYNC();   // lane 0's window appends (HBM) and indices (LDS) before the samplers
  get_obs_lanes(S.s, S.gs->ring, C, obs + (size_t)env * C->n_obs, lane);
  PH(20);
  if (lane == 0) {
    int d = is_done(S.s, C);
    float r = reward(S.s, C);
    S.s.done = d;
    S.s.reward = r;
    rew[env] = r;
    done[env] = (uint8_t)d;
    PH(21);
  }
}

template <int CL>
__device__ __forceinline__ void load_state(SharedT<CL>& S, GmEnvState* __restrict__ g, int lane) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(g);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&S.s);
  for (int i = lane; i < GM_HOT_WORDS; i += NT) dst[i] = src[i];
  S.gs = g;
  GM_ENV_SYNC();
}
template <int CL>
__device__ __forceinline__ void store_state(const SharedT<CL>& S, GmEnvState* __restrict__ g, int lane) {
  GM_ENV_SYNC();
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&S.s);
  uint32_t* dst = reinterpret_cast<uint32_t*>(g);
  for (int i = lane; i < GM_HOT_WORDS; i += NT) dst[i] = src[i];
}
