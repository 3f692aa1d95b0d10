// gm_reset.h -- episode reset and object spawn on a GmEnvHot image and its HBM record (no
// SharedT field): MjClass::spawn_object (mjclass.cpp:2352-2420), spawn_into_scene (2475-2654,
// libstdc++'s uniform_int_distribution / shuffle over minstd_rand0), MjClass::reset (434-486).
#pragma once
#include "gm_gripper.h"
#include "gm_sensors.h"

// ---------------------------------------------------------------- reset + spawn
// MjClass::spawn_object -> ObjectHandler::spawn_object (mjclass.cpp:2352-2420,
// objecthandler.cpp:403-428): live object, pose on the ground at (x, y), z-rotation
__device__ void spawn_object(GmEnvHot& s, const GmTopo* __restrict__ T, const gm_object* __restrict__ objs,
                             int n_objects, gm_spawn sp) {
  int oi = sp.object_index;
  if (oi < 0 || oi >= n_objects) oi = 0;
  const gm_object& o = objs[oi];
  s.obj_index = oi;
  s.obj_type = o.type;
  s.obj_size[0] = o.size[0]; s.obj_size[1] = o.size[1]; s.obj_size[2] = o.size[2];
  s.obj_mass = o.mass;
  s.obj_friction = o.friction;
  double I0, I1, I2, rb, restz;
  if (o.type == GM_GEOM_BOX) {
    double a = 2 * o.size[0], bb = 2 * o.size[1], c = 2 * o.size[2];
    I0 = o.mass * (bb * bb + c * c) / 12; I1 = o.mass * (a * a + c * c) / 12; I2 = o.mass * (a * a + bb * bb) / 12;
    rb = sqrt(o.size[0] * o.size[0] + o.size[1] * o.size[1] + o.size[2] * o.size[2]);
    restz = o.size[2];
  } else if (o.type == GM_GEOM_CYLINDER) {
    double r = o.size[0], hh = 2 * o.size[1];
    I0 = I1 = o.mass * (3 * r * r + hh * hh) / 12; I2 = o.mass * r * r / 2;
    rb = sqrt(o.size[0] * o.size[0] + o.size[1] * o.size[1]);
    restz = o.size[1];
  } else {
    double r = o.size[0];
    I0 = I1 = I2 = 2 * o.mass * r * r / 5;
    rb = r;
    restz = r;
  }
  s.obj_inertia[0] = I0; s.obj_inertia[1] = I1; s.obj_inertia[2] = I2;
  s.obj_rbound = rb;
  s.obj_rest_z = restz;
  // body_invweight0 of the live object (mj_setConst at qpos0; oracle object_invweight)
  s.obj_invw[0] = 1.0 / o.mass;
  s.obj_invw[1] = ((1.0 / I0 + 1.0 / I1) + 1.0 / I2) / 3.0;
  int qa = T->qadr_obj;
  double x2, w2;
  gm_sincos(-sp.zrot / 2.0, &x2, &w2);   // shared with the oracle (gm_math.h)
  double q4[4] = {x2, 0, 0, w2};   // reference QPos quirk: qx lands in MuJoCo's w slot
  double nq = sqrt(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3]);
  s.qpos[qa + 0] = sp.x;
  s.qpos[qa + 1] = sp.y;
  s.qpos[qa + 2] = restz + 1e-6;
  for (int k = 0; k < 4; k++) s.qpos[qa + 3 + k] = q4[k] / nq;
  for (int k = 0; k < 7; k++) s.start_qpos[k] = s.qpos[qa + k];
  for (int k = 0; k < 6; k++) s.qvel[T->dof_obj + k] = 0;
}

// ---------------------------------------------------------------- spawn_into_scene
// MjClass::spawn_into_scene(SpawnParams) (mjclass.cpp:2475-2654), one thread per env.
//
// std::uniform_int_distribution<unsigned long>{a, b} driven by minstd_rand0, as libstdc++
// implements it (bits/uniform_int_dist.h): the engine's range 2^31 - 3 is neither 2^32 - 1
// nor 2^64 - 1, so the downscaling branch takes the two-division rejection path.
__device__ uint64_t uid_minstd(uint32_t& st, uint64_t a, uint64_t b) {
  const uint64_t urngrange = 2147483646ull - 1ull;   // max() - min()
  const uint64_t urange = b - a;
  uint64_t ret;
  if (urngrange > urange) {
    // every operand is below 2^31 here: 32-bit division, the same quotients as the
    // 64-bit ones libstdc++ computes (a 64-bit divide is a long software sequence)
    const uint32_t uerange = (uint32_t)urange + 1u;
    const uint32_t scaling = (uint32_t)urngrange / uerange;
    const uint32_t past = uerange * scaling;
    uint32_t r32;
    do r32 = lcg_next(st) - 1u; while (r32 >= past);
    ret = r32 / scaling;
  } else {
    ret = (uint64_t)lcg_next(st) - 1ull;   // urange == urngrange (grids are far smaller)
  }
  return ret + a;
}
// std::shuffle(first, first + n, minstd_rand0) as libstdc++ implements it
// (bits/stl_algo.h): when the engine range allows, positions are drawn two at a time
// from one uniform_int over [0, (k + 1)(k + 2) - 1] (__gen_two_uniform_ints), with a
// single leading {0, 1} draw for even n.  Shuffling indices permutes exactly like
// shuffling the elements.  (n <= GM_SPAWN_MAX_XY: the pair range and its quotients fit
// 32 bits.)
__device__ __forceinline__ void shuffle_minstd(uint16_t* v, int n, uint32_t& st) {
  if (n <= 0) return;
  const uint64_t urngrange = 2147483645ull, urange = (uint64_t)n;
  if (urngrange / urange >= urange) {
    int i = 1;
    if ((urange % 2) == 0) {
      const int j = (int)uid_minstd(st, 0, 1);
      const uint16_t t = v[i]; v[i] = v[j]; v[j] = t;
      i++;
    }
    while (i != n) {
      const uint32_t r = (uint32_t)i + 1u;
      const uint32_t x = (uint32_t)uid_minstd(st, 0, (uint64_t)r * (r + 1) - 1);
      const int p1 = (int)(x / (r + 1u)), p2 = (int)(x % (r + 1u));
      uint16_t t = v[i]; v[i] = v[p1]; v[p1] = t;
      i++;
      t = v[i]; v[i] = v[p2]; v[p2] = t;
      i++;
    }
  } else {
    for (int i = 1; i < n; i++) {
      const int j = (int)uid_minstd(st, 0, (uint64_t)i);
      const uint16_t t = v[i]; v[i] = v[j]; v[j] = t;
    }
  }
}
// luke::Box2d (customtypes.h:35-172): corners counter-clockwise from bottom-left
struct Box2 { double x[4], y[4]; };
__device__ void box_init_centre(Box2& b, double cx, double cy, double width, double height) {
  const double hw = width / 2.0, hh = height / 2.0;
  b.x[0] = cx - hw; b.y[0] = cy - hh;
  b.x[1] = cx + hw; b.y[1] = cy - hh;
  b.x[2] = cx + hw; b.y[2] = cy + hh;
  b.x[3] = cx - hw; b.y[3] = cy + hh;
}
__device__ void box_rotate(Box2& b, double theta) {
  const double cx = (b.x[0] + b.x[1] + b.x[2] + b.x[3]) / 4.0;
  const double cy = (b.y[0] + b.y[1] + b.y[2] + b.y[3]) / 4.0;
  const double c = cos(theta), s = sin(theta);
  for (int i = 0; i < 4; i++) {
    const double nx = cx + (b.x[i] - cx) * c - (b.y[i] - cy) * s;
    const double ny = cy + (b.x[i] - cx) * s + (b.y[i] - cy) * c;
    b.x[i] = nx; b.y[i] = ny;
  }
}
__device__ bool box_inbounds(const Box2& b, double xmin, double ymin, double xmax, double ymax) {
  for (int i = 0; i < 4; i++)
    if (b.x[i] < xmin || b.x[i] > xmax || b.y[i] < ymin || b.y[i] > ymax) return false;
  return true;
}
// Box2d::overlapsWith: SAT over this box's four edge normals only, with the reference's
// "containsOther" bookkeeping (true only if no axis separates by more than zero)
__device__ bool box_overlaps(const Box2& a, const Box2& o, double gap) {
  bool contains = true;
  for (int i = 0; i < 4; i++) {
    const int j = (i + 1) % 4;
    double px = -(a.y[j] - a.y[i]), py = a.x[j] - a.x[i];
    const double len = sqrt(px * px + py * py);
    px /= len; py /= len;
    double min1 = a.x[0] * px + a.y[0] * py, max1 = min1;
    double min2 = o.x[0] * px + o.y[0] * py, max2 = min2;
    for (int k = 1; k < 4; k++) {
      const double p1 = a.x[k] * px + a.y[k] * py;
      const double p2 = o.x[k] * px + o.y[k] * py;
      if (p1 < min1) min1 = p1;
      if (p1 > max1) max1 = p1;
      if (p2 < min2) min2 = p2;
      if (p2 > max2) max2 = p2;
    }
    if (max1 + gap < min2 || max2 + gap < min1) return false;
    if (max1 < min2 || max2 < min1) contains = false;
  }
  return contains;
}
// "Task object i" xyz bounding box (objecthandler.cpp:91-110): full extents of the
// synthetic object's geom (the MJCF numerics are unavailable)
__device__ __host__ inline void object_bbox(const gm_object& o, double* xyz) {
  if (o.type == GM_GEOM_BOX) { xyz[0] = 2 * o.size[0]; xyz[1] = 2 * o.size[1]; xyz[2] = 2 * o.size[2]; }
  else if (o.type == GM_GEOM_CYLINDER) { xyz[0] = xyz[1] = 2 * o.size[0]; xyz[2] = 2 * o.size[1]; }
  else { xyz[0] = xyz[1] = xyz[2] = 2 * o.size[0]; }
}
// returns 1 and spawns on success; 0 when no candidate pose is free
// pxy / prot: the shuffled grids' work buffers (GM_SPAWN_MAX_XY / GM_SPAWN_MAX_ROT entries):
// LDS in the reset kernel (its one working lane would otherwise wait on a scratch round
// trip per swap), private arrays in the thread-per-env kernel
__device__ __forceinline__ int spawn_into_scene_dev(GmEnvHot& s, const gm_model* __restrict__ m,
                                                    const GmTopo* __restrict__ T, const gm_object* __restrict__ objs,
                                                    int n_objects, const gm_spawn_params& p, int index,
                                                    uint16_t* pxy, uint16_t* prot) {
  const int num_x = (int)(((2 * p.xrange) / p.xy_increment) + 1);
  const int num_y = (int)(((2 * p.yrange) / p.xy_increment) + 1);
  const int num_r = (int)(((2 * p.rotrange) / p.rot_increment) + 1);
  const int nxy = num_x * num_y;
  if (num_x < 1 || num_y < 1 || num_r < 1 || nxy > GM_SPAWN_MAX_XY || num_r > GM_SPAWN_MAX_ROT) return 0;
  for (int i = 0; i < nxy; i++) pxy[i] = (uint16_t)i;
  for (int i = 0; i < num_r; i++) prot[i] = (uint16_t)i;
  {
    uint32_t rng = s.rng;   // in a register through both shuffles, not the env's HBM record
    if (nxy > 1) shuffle_minstd(pxy, nxy, rng);
    if (num_r > 1) shuffle_minstd(prot, num_r, rng);
    s.rng = rng;
  }
  // object footprint
  int oi = index;
  if (oi < 0 || oi >= n_objects) oi = 0;
  double bb[3];
  object_bbox(objs[oi], bb);
  // initial fingertip boxes: Env::reset (mjclass.h:895-904) from
  // get_finger_hook_locations (myfunctions.cpp:3717-3761), straight fingers at the target
  Box2 tips[3];
  {
    const double PI_23 = M_PI * (2.0 / 3.0);
    const double angles[3] = {0.0, PI_23, 2 * PI_23};
    const double fing_x = s.end.x;
    const double hook_th = m->hook_angle_degrees * (M_PI / 180.000);
    for (int i = 0; i < 3; i++) {
      const double hook_x = 0.5 * m->hook_length * sin(hook_th);
      const double x = -(fing_x - hook_x) * sin(angles[i]) + s.base[0];
      const double y = -(fing_x - hook_x) * cos(angles[i]) + s.base[1];
      box_init_centre(tips[i], x, y, m->finger_width, m->hook_length);
      box_rotate(tips[i], -angles[i]);
    }
  }
  const int total = nxy > num_r ? nxy : num_r;
  int ixy = -1, ir = -1;
  for (int i = 0; i < total; i++) {
    ixy += 1; ir += 1;
    if (ixy >= nxy) ixy = 0;
    if (ir >= num_r) ir = 0;
    const int kx = pxy[ixy] / num_y, ky = pxy[ixy] % num_y;
    const double px = num_x > 1 ? -p.xrange + kx * p.xy_increment + p.x : p.x;
    const double py = num_y > 1 ? -p.yrange + ky * p.xy_increment + p.y : p.y;
    const double pr = num_r > 1 ? -p.rotrange + prot[ir] * p.rot_increment + p.zrot : p.zrot;
    Box2 ob;
    box_init_centre(ob, px, py, bb[0], bb[1]);
    box_rotate(ob, pr);
    if (!box_inbounds(ob, p.xmin, p.ymin, p.xmax, p.ymax)) continue;
    bool good = true;
    for (int f = 0; f < 3 && good; f++)
      if (box_overlaps(ob, tips[f], p.smallest_gap)) good = false;
    if (!good) continue;
    spawn_object(s, T, objs, n_objects, gm_spawn{index, px, py, pr});
    return 1;
  }
  return 0;
}

// what survives a reset (see reset_env)
struct GmResetKeep {
  uint32_t rng;
  int32_t ox, oy, oz, episode, newton_caps;
};
// MjClass::reset (mjclass.cpp:434-486) -> luke::reset / calibrate_reset (non-first call),
// configure_settings RNG draws, random_base_Z_movement, then spawn_object.
// The whole reset of one env by one wave on an LDS image `s` of its hot state (rec: its HBM
// record, whose sensor windows are cleared in place): the image is cleared with coalesced
// 16-byte stores, then lane 0 runs the reference's serial reset (RNG draws, spawn search --
// pxy / prot: LDS work buffers of GM_SPAWN_MAX_XY / GM_SPAWN_MAX_ROT entries).  What survives
// a reset (the per-env RNG stream, the function-static stepper flags -- a reference quirk --,
// the episode counter, the solver diagnostics) comes in as arguments, read by the caller
// before the clear.  Used by gm_reset_kernel and by the rollout's in-kernel auto-reset.
__device__ __noinline__ void reset_env(GmEnvHot& s, GmEnvState& rec, GmResetKeep keep, const gm_model* __restrict__ m,
                                       const gm_config* __restrict__ C, const GmTopo* __restrict__ T,
                                       const double* __restrict__ eq_qpos, const gm_spawn* __restrict__ spawn,
                                       const gm_object* __restrict__ objs, int n_objects, int env,
                                       const gm_spawn_params* __restrict__ scene, int scene_tries, GmSpawnRand sr,
                                       uint16_t* sh_pxy, uint16_t* sh_prot, int lane) {
  {
    static_assert(sizeof(GmEnvState) % 16 == 0 && sizeof(GmEnvHot) % 16 == 0, "records move in 16-byte words");
    uint4* hw = reinterpret_cast<uint4*>(&s);
    for (int i = lane; i < GM_HOT_WORDS / 4; i += 64) hw[i] = make_uint4(0u, 0u, 0u, 0u);
    uint4* w = reinterpret_cast<uint4*>(&rec);
    for (int i = GM_HOT_WORDS / 4 + lane; i < GM_STATE_WORDS / 4; i += 64) w[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  GM_ENV_SYNC();
  if (lane == 0) {   // the reference's serial reset on lane 0
    const int32_t episode = keep.episode;
    s.rng = keep.rng; s.old_x = keep.ox; s.old_y = keep.oy; s.old_z = keep.oz;
    s.episode = episode;
    s.newton_caps = keep.newton_caps;
    g_reset(s.end); g_reset(s.next);
    for (int k = 0; k < GM_MAX_QPOS; k++) s.qpos[k] = m->qpos0[k];
    s.time = 0; s.last_step_time = 0;
    s.dt = m->timestep;
    for (int d = 0; d < T->nv; d++) {
      bool motor = (d == m->dof_base || d == m->dof_palm);
      for (int f = 0; f < 3; f++) motor = motor || d == m->dof_pris[f] || d == m->dof_rev[f];
      if (motor) s.qpos[d] = eq_qpos[d];
    }
    for (int k = 0; k < T->nlock; k++) { s.lock_active[k] = 1; s.lock_q[k] = m->qpos0[m->lock_dof[k]]; }
    for (int st = 0; st < GM_NSTREAM; st++) s.ring_i[st] = -1;
    // apply_noise_params: mean draws, SS order then the state sensors again
    {
      const gm_settings& st = C->s;
      const gm_sensor* ss[SL_N] = {&st.motor_state_sensor, &st.base_state_sensor_Z, &st.base_state_sensor_XY,
                                   &st.base_state_sensor_yaw, &st.bending_gauge, &st.axial_gauge, &st.palm_sensor,
                                   &st.wrist_sensor_XY, &st.wrist_sensor_Z, &st.cartesian_contacts_XYZ};
      uint32_t g = s.rng;   // the draws below run on a register copy of the stream
      for (int k = 0; k < SL_N; k++)
        for (int i = 0; i < 3; i++) {
          s.rand_mu[k][i] = ss[k]->noise_mu * (2 * unif01(g) - 1);
        }
      int order[5] = {SL_MOTOR, SL_BASEXY, SL_BASEZ, SL_YAW, SL_CART};
      for (int k = 0; k < 5; k++)
        for (int i = 0; i < 3; i++) {
          s.rand_mu[order[k]][i] = ss[order[k]]->noise_mu * (2 * unif01(g) - 1);
        }
      s.rng = g;
    }
    {
      double size = C->s.base_position_noise;
      uint32_t g = s.rng;
      double u = canon_d(g);
      s.rng = g;
      double z = u * (size - (-size)) + (-size);
      s.base[2] = z;
      if (s.base[2] > C->base_max[2]) s.base[2] = C->base_max[2];
      if (s.base[2] < C->base_min[2]) s.base[2] = C->base_min[2];
      s.qpos[m->dof_base] = s.base[2] + eq_qpos[m->dof_base];
    }
    gm_spawn sp = spawn ? spawn[env] : gm_spawn{0, 0.0, 0.0, 0.0};
    if (sr.enable && !spawn) {
      // MjEnv._spawn_object's generator draws: object index, then the "old method" pose
      // (integer mm offsets, one of {0, 60, 120} deg plus integer-degree noise)
      const int64_t gid = sr.env_offset + env;
      const int nm = sr.position_noise_mm, nd = sr.rotation_noise_deg;
      sp.object_index = gm_spawn_int(sr.seed, gid, episode, 0, 0, n_objects - 1);
      sp.x = gm_spawn_int(sr.seed, gid, episode, 1, -nm, nm) * 1e-3;
      sp.y = gm_spawn_int(sr.seed, gid, episode, 2, -nm, nm) * 1e-3;
      const int noise_deg = gm_spawn_int(sr.seed, gid, episode, 3, -nd, nd);
      const int opt = gm_spawn_int(sr.seed, gid, episode, 4, 0, 2);
      sp.zrot = (60 * opt + noise_deg) * (M_PI / 180.0);
    }
    bool placed = false;
    if (scene) {
      // MjEnv._spawn_object (MjEnv.py:1177-1267): spawn_into_scene up to scene_tries times,
      // then the "old method" pose from the spawn table
      for (int t = 0; t < scene_tries && !placed; t++)
        placed = spawn_into_scene_dev(s, m, T, objs, n_objects, *scene, sp.object_index, sh_pxy, sh_prot);
    }
    if (!placed) spawn_object(s, T, objs, n_objects, sp);
    s.done = 0;
    s.reward = 0;
  }
  GM_ENV_SYNC();
}
