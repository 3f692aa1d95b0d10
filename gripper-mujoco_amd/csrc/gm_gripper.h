// gm_gripper.h -- lane-0 reference logic, part 1: luke::Gripper (gripper.cpp), update_all
// (myfunctions.cpp:2129-2284) and MjClass::set_action (mjclass.cpp:1528-1630) on a GmEnvHot.
// SharedT: reads s.time, s.end, s.qvel, lock_pre; writes s.next, s.lock_active, s.lock_q,
// s.old_x / _y / _z, s.last_step_time, stp_fixed, and zeroes a resting object's s.qvel.
#pragma once
#include "gm_real.h"

// ============================================================ reference scalar logic (lane 0)
// luke::Gripper in fp64 (gripper.cpp), bit-for-bit the same operations as the reference
#define G_XY_MIN 49e-3
#define G_XY_MAX 134e-3
#define G_Z_MIN 0e-3
#define G_Z_MAX 165e-3
#define G_TOL 1e-4
#define G_LEAD 35e-3
__device__ __forceinline__ double g_xy_step_m() { return 4.0 / (1.0 * 400 * 1e3); }
__device__ __forceinline__ double g_z_step_m() { return 4.8768 / (1 * 400 * 1e3); }
__device__ __forceinline__ double g_calc_th(double x, double y) { return asin((y - x) / G_LEAD) * 1; }
__device__ __forceinline__ double g_calc_y(const GmGrip& g, double th) { return g.x + 1 * G_LEAD * sin(th); }
__device__ __forceinline__ int g_xs(const GmGrip& g) { return (int)round((G_XY_MAX - g.x) / g_xy_step_m()); }
__device__ __forceinline__ int g_ys(const GmGrip& g) { return (int)round((G_XY_MAX - g.y) / g_xy_step_m()); }
__device__ __forceinline__ int g_zs(const GmGrip& g) { return (int)round(g.z / g_z_step_m()); }
__device__ __forceinline__ double g_th_deg(const GmGrip& g) { return (180.0 / 3.14159265358979323846) * g_calc_th(g.x, g.y); }
__device__ int g_update_xy(GmGrip& g) {
  const double to_rad = 3.14159265358979323846 / 180.0;
  const double th_min = -40 * to_rad, th_max = 40 * to_rad;
  const double hyp = sqrt(pow(235e-3, 2) + pow(35.0e-3, 2));
  const double rest = atan(35.0e-3 / 235e-3);
  int wl = 1;
  if (g.x > G_XY_MAX + G_TOL) { g.x = G_XY_MAX; wl = 0; }
  if (g.x < G_XY_MIN - G_TOL) { g.x = G_XY_MIN; wl = 0; }
  if (g.y > G_XY_MAX + G_TOL) { g.y = G_XY_MAX; wl = 0; }
  if (g.y < G_XY_MIN - G_TOL) { g.y = G_XY_MIN; wl = 0; }
  double nth = g_calc_th(g.x, g.y);
  if (nth > th_max) { nth = th_max; g.y = g_calc_y(g, th_max); wl = 0; }
  if (nth < th_min) { nth = th_min; g.y = g_calc_y(g, th_min); wl = 0; }
  g.th = nth;
  double th_lim = (asin((-1.0 - g.x) / hyp) + rest) * 1;
  if (g.th < th_lim) { g.y = g_calc_y(g, th_lim); g.th = th_lim; wl = 0; }
  g.sx = g_xs(g);
  g.sy = g_ys(g);
  return wl;
}
__device__ int g_update_z(GmGrip& g) {
  int wl = 1;
  if (g.z > G_Z_MAX + G_TOL) { g.z = G_Z_MAX; wl = 0; }
  if (g.z < G_Z_MIN - G_TOL) { g.z = G_Z_MIN; wl = 0; }
  g.sz = g_zs(g);
  return wl;
}
__device__ void g_reset(GmGrip& g) {
  g.x = G_XY_MAX - 1.0 * (4 * 1e-3 / 1.0);
  g.y = g.x;
  g.z = G_Z_MIN + 1.0 * (4.8768 * 1e-3 / 1);
  int a = g_update_xy(g); int b = g_update_z(g); (void)a; (void)b;
}
__device__ int g_set_xyz_m_rad(GmGrip& g, double x, double th, double z) {
  g.x = x; g.y = g_calc_y(g, th);
  int in_lim = g_update_xy(g);
  g.z = z;
  return g_update_z(g) ? in_lim : 0;
}
__device__ int g_set_xyz_m(GmGrip& g, double x, double y, double z) {
  g.x = x; g.y = y; g.z = z;
  int a = g_update_xy(g); int b = g_update_z(g);
  return a * b;
}
__device__ int g_set_xyz_step(GmGrip& g, int xs, int ys, int zs) {
  g.x = G_XY_MAX - g_xy_step_m() * xs; g.y = G_XY_MAX - g_xy_step_m() * ys;
  int in_lim = g_update_xy(g);
  g.z = g_z_step_m() * zs;
  return g_update_z(g) ? in_lim : 0;
}
__device__ int g_step_to(GmGrip& g, const GmGrip& t, int num) {
  int fin = 1;
  int xg = t.sx - g.sx, yg = t.sy - g.sy, zg = t.sz - g.sz;
  if (xg < 0) { if (-xg > num) { xg = -num; fin = 0; } } else if (xg > num) { xg = num; fin = 0; }
  if (yg < 0) { if (-yg > num) { yg = -num; fin = 0; } } else if (yg > num) { yg = num; fin = 0; }
  if (zg < 0) { if (-zg > num) { zg = -num; fin = 0; } } else if (zg > num) { zg = num; fin = 0; }
  g_set_xyz_step(g, g.sx + xg, g.sy + yg, g.sz + zg);
  return fin;
}

// update_all: update_stepper / update_constraints (myfunctions.cpp:2129-2284), antiroll
template <int CL>
GM_EPI_ATTR void update_all(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T, int lane) {
  GmEnvHot& s = S.s;
  const bool stepping = s.time > s.last_step_time + m->time_per_step;   // uniform (LDS broadcast)
  // Once a stepper update left `next` bit for bit unchanged, every later one in this
  // env-step does too (`end` only changes between env-steps, and g_step_to is a pure
  // function of the two grippers), and the lock-toggle tests see the same (end, next) as
  // that update did, so their flags already match: only the step time moves.
  const bool fixed = stepping && S.stp_fixed;
  int nx = 0, ny = 0, nz = 0;
  if (stepping && !fixed) {
    // the end (lane 0) and next (lane 1) grippers' step counts and angle in one pass of
    // the wave instead of two serial evaluations on lane 0 (an asin and two divisions each)
    const GmGrip& g = (lane & 1) ? s.next : s.end;
    const int xs = g_xs(g), zs = g_zs(g);
    const double th = g_th_deg(g);
    nx = __builtin_amdgcn_readlane(xs, 0) != __builtin_amdgcn_readlane(xs, 1);
    ny = !(fabs(readlane_real(th, 0) - readlane_real(th, 1)) < 5e-1);
    nz = __builtin_amdgcn_readlane(zs, 0) != __builtin_amdgcn_readlane(zs, 1);
  }
  if (lane == 0) {
    if (fixed) {
      s.last_step_time = s.time;
    } else if (stepping) {
      if (nx != s.old_x) {
        for (int k = 0; k < T->nlock; k++)
          if (m->lock_kind[k] == 0) { s.lock_active[k] = !nx; if (!nx) s.lock_q[k] = S.lock_pre[k]; }
        s.old_x = nx;
      }
      if (ny != s.old_y) s.old_y = ny;   // revolute locks disabled (myfunctions.cpp:479)
      if (nz != s.old_z) {
        for (int k = 0; k < T->nlock; k++)
          if (m->lock_kind[k] == 2) { s.lock_active[k] = !nz; if (!nz) s.lock_q[k] = S.lock_pre[k]; }
        s.old_z = nz;
      }
      s.last_step_time = s.time;
      const GmGrip before = s.next;
      g_step_to(s.next, s.end, m->stepper_num_steps);
      const GmGrip& a = s.next;
      S.stp_fixed = __double_as_longlong(a.x) == __double_as_longlong(before.x) &&
                    __double_as_longlong(a.y) == __double_as_longlong(before.y) &&
                    __double_as_longlong(a.z) == __double_as_longlong(before.z) &&
                    __double_as_longlong(a.th) == __double_as_longlong(before.th) && a.sx == before.sx &&
                    a.sy == before.sy && a.sz == before.sz;
    }
    const real* v = &s.qvel[T->dof_obj];
    real mag = sqrt_n(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);   // (= sqrt wherever it decides anything)
    if (mag < 1e-6) for (int k = 0; k < 6; k++) s.qvel[T->dof_obj + k] = 0;
  }
  GM_WAVE_SYNC();
}

// ---------------------------------------------------------------- actions
// MjClass::set_action for every action index (mjclass.cpp:1528-1630); one thread per env.
__device__ int move_base_target_m(GmEnvHot& s, const gm_config* __restrict__ C, double x, double y, double z) {
  double* b = s.base;
  b[0] += x; b[1] += y; b[2] += z;
  int wl = 1;
  for (int k = 0; k < 3; k++) {
    if (b[k] > C->base_max[k]) { b[k] = C->base_max[k]; wl = 0; }
    if (b[k] < C->base_min[k]) { b[k] = C->base_min[k]; wl = 0; }
  }
  return wl;
}
__device__ int call_action(GmEnvHot& s, const gm_config* __restrict__ C, int kind, double v) {
  const gm_action* acts[GM_N_ACTION_KINDS] = {
#define GM_AA(n, u, vv, sg) &C->s.n,
#include "gm_settings.def"
  };
  v *= acts[kind]->sign;
  switch (kind) {
    case GM_ACT_gripper_X: return g_set_xyz_m(s.end, s.end.x + v, s.end.y, s.end.z);
    case GM_ACT_gripper_Y: return g_set_xyz_m(s.end, s.end.x, s.end.y + v, s.end.z);
    case GM_ACT_gripper_prismatic_X: return g_set_xyz_m_rad(s.end, s.end.x + v, s.end.th, s.end.z);
    case GM_ACT_gripper_revolute_Y: return g_set_xyz_m_rad(s.end, s.end.x, s.end.th + v, s.end.z);
    case GM_ACT_gripper_Z: return g_set_xyz_m(s.end, s.end.x, s.end.y, s.end.z + v);
    case GM_ACT_base_X: return move_base_target_m(s, C, v, 0, 0);
    case GM_ACT_base_Y: return move_base_target_m(s, C, 0, v, 0);
    case GM_ACT_base_Z: return move_base_target_m(s, C, 0, 0, v);
    case GM_ACT_base_roll:
    case GM_ACT_base_pitch: return 1;
    default: {
      s.base[5] += v;
      int wl = 1;
      if (s.base[5] > C->base_max[5]) { s.base[5] = C->base_max[5]; wl = 0; }
      if (s.base[5] < C->base_min[5]) { s.base[5] = C->base_min[5]; wl = 0; }
      return wl;
    }
  }
}
__device__ void set_action_one(GmEnvHot& s, const gm_model* __restrict__ m, const gm_config* __restrict__ C,
                               int action, float frac) {
  const gm_settings& st = C->s;
  int wl = 1;
  s.termination_signal_sent = 0;
  if (action < 0 || action >= C->n_actions) return;
  int code = C->action_options[action];
  if (code == GM_ACTION_TERMINATION) {
    float value = st.continous_actions ? frac : 1.0f;
    if (value > st.termination_threshold) {
      s.termination_signal_sent = 1;
      if (st.lift_on_termination) {
        s.base[2] = -C->base_max[2];
        if (s.base[2] > C->base_max[2]) s.base[2] = C->base_max[2];
        if (s.base[2] < C->base_min[2]) s.base[2] = C->base_min[2];
        s.extra_substeps += C->sim_steps_per_action * 2;
      }
    }
    wl = 1;
  } else {
    const gm_action* acts[GM_N_ACTION_KINDS] = {
#define GM_AA(n, u, vv, sg) &st.n,
#include "gm_settings.def"
    };
    int kind = code / 3, sub = code % 3;
    if (sub == 0) wl = call_action(s, C, kind, acts[kind]->value);
    else if (sub == 1) wl = call_action(s, C, kind, -1 * acts[kind]->value);
    else {
      wl = call_action(s, C, kind, acts[kind]->value * frac);
      s.lev_value[GM_LEV_action_penalty_lin] += fabsf(frac);
      s.lev_value[GM_LEV_action_penalty_sq] += (frac * frac);
    }
  }
  // get_fingertip_z_height (myfunctions.cpp:3608-3620)
  float straight = (float)(-C->base_min[2] - s.base[2]);
  float tip_lift = (float)(m->finger_length * (1 - cos(g_calc_th(s.end.x, s.end.y))));
  float hgt = straight + tip_lift;
  float fz = (float)(hgt + C->base_min[2]);
  if (fz < st.fingertip_min_mm * 1e-3) wl = 0;
  s.bev_value[GM_EV_exceed_limits] = s.bev_value[GM_EV_exceed_limits] || !wl;
}

// action code -> action kind (gm_settings.def order, three codes a kind); -1: the termination action
__device__ __forceinline__ int action_kind(int code) {
  return (code >= 0 && code < GM_ACTION_TERMINATION) ? code / 3 : -1;
}
