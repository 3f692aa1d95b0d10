// gm_sensors.h -- lane-0 reference logic, part 2: the per-env RNG, the sensor windows (rings),
// the simulated sensors, gauge_reading, extract_forces, monitor_sensors (mjclass.cpp:741-898).
// SharedT: reads s, con, cgeom, ncon, xpos, gs (the record's rings); writes the rings and
// their indices in s, s.rng, forces, have_forces, gauge_tmp, bend_ready.
#pragma once
#include "gm_real.h"

// ---- RNG: minstd_rand0 + generate_canonical (libstdc++), per-env stream ----
__device__ __forceinline__ uint32_t lcg_next(uint32_t& s) {
  s = (uint32_t)(((uint64_t)s * 16807ull) % 2147483647ull);
  return s;
}
__device__ float unif01(uint32_t& s) {
  const float r = 2147483646.0f;
  float sum = (float)(lcg_next(s) - 1u) * 1.0f;
  float ret = sum / r;
  if (ret >= 1.0f) ret = __int_as_float(0x3F7FFFFF);  // nextafterf(1, 0)
  return ret * (1.0f - 0.0f) + 0.0f;
}
__device__ double canon_d(uint32_t& s) {
  const double r = 2147483646.0;
  double sum = 0.0, tmp = 1.0;
  for (int k = 0; k < 2; k++) { sum += (double)(lcg_next(s) - 1u) * tmp; tmp *= r; }
  double ret = sum / tmp;
  if (ret >= 1.0) ret = __longlong_as_double(0x3FEFFFFFFFFFFFFFLL);  // nextafter(1, 0)
  return ret;
}

// ---- sensors (mjclass.h:155-241) ----
// SlidingWindow::add / read_element on a ring of GM_RING readings (the window itself
// lives in the env's HBM record, GmEnvState::ring; its write index in the hot state)
typedef float (*RingRef)[GM_RING];
__device__ __forceinline__ void ring_add(GmEnvHot& s, RingRef R, int st, float x) {
  int i = s.ring_i[st] + 1;
  if (i > GM_RING - 1) i = 0;
  s.ring_i[st] = i;
  R[st][i] = x;
}
__device__ __forceinline__ float ring_read(const GmEnvHot& s, RingRef R, int st, int n) {
  int idx = s.ring_i[st] - n;
  while (idx < 0) idx += GM_RING;
  return R[st][idx];
}
__device__ __forceinline__ float ring_latest(const GmEnvHot& s, RingRef R, int st) {
  return s.ring_i[st] == -1 ? R[st][0] : R[st][s.ring_i[st]];
}
__device__ float s_normalise(const gm_sensor& ss, float v) {
  if (!ss.use_normalisation) return v;
  if (ss.normalise <= 0) return v < 0 ? -1.0f : 1.0f;
  else if (v > ss.normalise) return 1.0f;
  if (v < -ss.normalise) return -1.0f;
  return v / ss.normalise;
}
// Box-Muller's z0 = mag * cos(2 pi u2) + mu (mjclass.h:211-212).  log and cos of the float
// argument are taken in fp64 and rounded to float: the float function's correctly rounded value,
// whichever math library is underneath (ocml's logf / cosf are within an ulp of it, which the
// smallest accepted u1, log = -15.9, turns into two ulps of the noise value).  One outlined
// copy: s_noise is inlined at fifteen call sites.
__device__ __noinline__ float gauss_z0(float noise_std, float u1, float u2, float mu) {
  const float two_pi = (float)(2.0 * 3.14159265358979323846);
  const float lg = (float)log((double)u1);
  const float cs = (float)gm_cos((double)(two_pi * u2));
  const float mag = (float)(noise_std * sqrt(-2.0 * (double)lg));
  return mag * cs + mu;
}
__device__ float s_noise(GmEnvHot& s, const gm_sensor& ss, int slot, float value, int i) {
  if (!ss.use_noise) return value;
  const float eps = 1.1920928955078125e-07f;
  float mu = s.rand_mu[slot][i - 1];
  if (ss.noise_std < eps) {
    float noise = mu + ss.noise_mag * (2 * unif01(s.rng) - 1);
    value += noise;
  } else {
    float u1, u2;
    do { u1 = unif01(s.rng); } while (u1 <= eps);
    u2 = unif01(s.rng);
    float z0 = gauss_z0(ss.noise_std, u1, u2, mu);
    value += z0;
  }
  if (value > 1) value = 1;
  else if (value < -1) value = -1;
  return value;
}
__device__ int s_ready(GmEnvHot& s, const gm_sensor& ss, int slot) {
  double tbr = (double)(1 / ss.read_rate);
  if (s.time > s.last_read[slot] + tbr) { s.last_read[slot] = s.time; return 1; }
  return 0;
}

// The earliest sim time at which one of monitor_sensors' four sensors becomes ready:
// s_ready's test is time > last_read + tbr, so time <= min over the sensors of
// (last_read + tbr) means none is, with the same operands and the same rounding.
__device__ __forceinline__ double next_sensor_read(const GmEnvHot& s, const gm_settings& st) {
  const gm_sensor* ss[4] = {&st.bending_gauge, &st.axial_gauge, &st.palm_sensor, &st.wrist_sensor_Z};
  const int slot[4] = {SL_BEND, SL_AXIAL, SL_PALM, SL_WRISTZ};
  double t = __builtin_inf();
  for (int k = 0; k < 4; k++) {
    const double tk = s.last_read[slot[k]] + (double)(1 / ss[k]->read_rate);
    t = tk < t ? tk : t;
  }
  return t;
}

// bending gauge: cubic least squares through the N+1 joint points, evaluated at
// gauge.xpos (read_armadillo_gauge, myfunctions.cpp:2699-2795).  Evaluated in fp64
// (two reads per env-step at 10 Hz: negligible cost): the fitted value at 50 mm is
// ~16x smaller than the tip deflection, so an fp32 fit would cost ~3e-5 relative.
// Householder QR on a centred/scaled abscissa -- the same least-squares solution as
// the reference's arma::polyfit on the raw Vandermonde.
template <int NS>
__device__ float gauge_reading(const gm_model* __restrict__ m, const real* q) {
  constexpr int P = NS + 1;
  const double Ls = m->segment_length;
  double X[P], Yv[P];
  X[0] = m->fixed_first_segment ? Ls : 0.0;
  Yv[0] = 0;
  double cum = 0;
#pragma unroll
  for (int i = 0; i < NS; i++) {
    cum = (i == 0) ? (double)q[0] : cum + (double)q[i];
    double sn, cs;
    gm_sincos(cum, &sn, &cs);
    X[i + 1] = X[i] + Ls * cs;
    Yv[i + 1] = Yv[i] + Ls * sn;
  }
  const double half = 0.5 * m->finger_length;
  const double ihalf = 1.0 / half;
  double A[P][4], b[P];
#pragma unroll
  for (int i = 0; i < P; i++) {
    const double t = (X[i] - half) * ihalf;
    A[i][0] = t * t * t; A[i][1] = t * t; A[i][2] = t; A[i][3] = 1.0;
    b[i] = Yv[i];
  }
  // Householder QR of the (centred) Vandermonde system, as LAPACK's dgels under arma::polyfit
#pragma unroll
  for (int k = 0; k < 4; k++) {
    double nrm = 0;
#pragma unroll
    for (int i = k; i < P; i++) nrm += A[i][k] * A[i][k];
    nrm = sqrt(nrm);
    const double alpha = A[k][k] > 0 ? -nrm : nrm;
    double v[P];
#pragma unroll
    for (int i = 0; i < P; i++) v[i] = (i >= k) ? A[i][k] : 0.0;
    v[k] -= alpha;
    double vv = 0;
#pragma unroll
    for (int i = k; i < P; i++) vv += v[i] * v[i];
    if (vv < 1e-300) continue;
    const double ivv = 2.0 / vv;
#pragma unroll
    for (int j = k; j < 4; j++) {
      double sacc = 0;
#pragma unroll
      for (int i = k; i < P; i++) sacc += v[i] * A[i][j];
      sacc *= ivv;
#pragma unroll
      for (int i = k; i < P; i++) A[i][j] -= sacc * v[i];
    }
    double sacc = 0;
#pragma unroll
    for (int i = k; i < P; i++) sacc += v[i] * b[i];
    sacc *= ivv;
#pragma unroll
    for (int i = k; i < P; i++) b[i] -= sacc * v[i];
  }
  double coeff[4];
#pragma unroll
  for (int k = 3; k >= 0; k--) {
    double sacc = b[k];
#pragma unroll
    for (int j = k + 1; j < 4; j++) sacc -= A[k][j] * coeff[j];
    coeff[k] = sacc / A[k][k];
  }
  const double tg = (m->gauge_xpos - half) * ihalf;
  const double y = ((coeff[0] * tg + coeff[1]) * tg + coeff[2]) * tg + coeff[3];
  return (float)y * 1000;
}

// extract_forces_faster (objecthandler.cpp:737-992) over the last substep's contacts.
// forces[]: obj_loc f1,f2,f3,palm (12) | obj ground global (3) | all_loc f1,f2,f3 x (3),
//           all_loc palm x (1) | gnd_loc f1,f2,f3 x (3)
template <int CL>
__device__ void extract_forces(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T) {
  real og[5][3], ag[4][3], gg[3][3];
  for (int a = 0; a < 5; a++) for (int k = 0; k < 3; k++) og[a][k] = 0;
  for (int a = 0; a < 4; a++) for (int k = 0; k < 3; k++) ag[a][k] = 0;
  for (int a = 0; a < 3; a++) for (int k = 0; k < 3; k++) gg[a][k] = 0;
  for (int i = 0; i < S.ncon; i++) {
    const real* C = S.con[i];
    int c1 = m->geom_class[S.cgeom[i][0]], c2 = m->geom_class[S.cgeom[i][1]];
    int w_obj = (c1 == GM_CLS_OBJECT || c2 == GM_CLS_OBJECT);
    int w_f0 = (c1 == GM_CLS_FINGER1 || c2 == GM_CLS_FINGER1);
    int w_f1 = (c1 == GM_CLS_FINGER2 || c2 == GM_CLS_FINGER2);
    int w_f2 = (c1 == GM_CLS_FINGER3 || c2 == GM_CLS_FINGER3);
    int w_palm = (c1 == GM_CLS_PALM || c2 == GM_CLS_PALM);
    int w_gnd = (c1 == GM_CLS_GROUND || c2 == GM_CLS_GROUND);
    real g[3];
    real Fr[9];
    Fr[0] = C[4]; Fr[1] = C[5]; Fr[2] = C[6]; Fr[3] = C[7]; Fr[4] = C[8]; Fr[5] = C[9];
    cross3(Fr + 6, Fr, Fr + 3);
    for (int k = 0; k < 3; k++) g[k] = Fr[k] * C[11] + Fr[3 + k] * C[12] + Fr[6 + k] * C[13];
    int wf[3] = {w_f0, w_f1, w_f2};
    if (w_obj) {
      for (int f = 0; f < 3; f++) if (wf[f]) for (int k = 0; k < 3; k++) og[f][k] += g[k];
      if (w_palm) for (int k = 0; k < 3; k++) og[3][k] += g[k];
      if (w_gnd) for (int k = 0; k < 3; k++) og[4][k] += g[k];
    }
    for (int f = 0; f < 3; f++)
      if (wf[f]) {
        for (int k = 0; k < 3; k++) ag[f][k] += g[k];
        if (w_gnd) for (int k = 0; k < 3; k++) gg[f][k] += g[k];
      }
    if (w_palm) for (int k = 0; k < 3; k++) ag[3][k] += g[k];
  }
  float* F = S.forces;
  for (int f = 0; f < 4; f++) {
    int b = f < 3 ? T->body_finger[f] : T->body_palm;
    real Rb[9];
    body_R(S, b, Rb);
    real loc[3];
    mulmtv3(loc, Rb, og[f]);
    F[3 * f] = (float)loc[0]; F[3 * f + 1] = (float)loc[1]; F[3 * f + 2] = (float)loc[2];
    real al[3];
    mulmtv3(al, Rb, ag[f]);
    if (f < 3) F[15 + f] = (float)al[0]; else F[18] = (float)al[0];
    if (f < 3) { real gl[3]; mulmtv3(gl, Rb, gg[f]); F[19 + f] = (float)gl[0]; }
  }
  F[12] = (float)og[4][0]; F[13] = (float)og[4][1]; F[14] = (float)og[4][2];
}

// mj_rnePostConstraint's cfrc_ext for the live object (myfunctions.cpp:1905), as
// ObjectHandler::get_object_net_force_faster reads it (objecthandler.cpp:543-565): each
// contact's world force (frame^T * contact-frame force) acts on geom2, its reaction on
// geom1; torques about the object's centre of mass.  out = [force; torque] (the
// reference's swapped order).  Lane-parallel over contacts, wave-reduced.
template <int CL>
__device__ void object_net_wrench(SharedT<CL>& S, const GmTopo* __restrict__ T, int lane, real* out) {
  real w[6] = {0, 0, 0, 0, 0, 0};
  if (lane < S.ncon) {
    const real* C = S.con[lane];
    const int g1 = S.cgeom[lane][0], g2 = S.cgeom[lane][1];
    const real sgn = (g2 == T->geom_obj) ? 1.0 : (g1 == T->geom_obj) ? -1.0 : 0.0;
    real Fr[9], g[3], r[3], t[3];
    Fr[0] = C[4]; Fr[1] = C[5]; Fr[2] = C[6]; Fr[3] = C[7]; Fr[4] = C[8]; Fr[5] = C[9];
    cross3(Fr + 6, Fr, Fr + 3);
    for (int k = 0; k < 3; k++) g[k] = Fr[k] * C[11] + Fr[3 + k] * C[12] + Fr[6 + k] * C[13];
    const int bo = T->body_obj;
    for (int k = 0; k < 3; k++) r[k] = C[1 + k] - S.xpos[bo][k];
    cross3(t, r, g);
    for (int k = 0; k < 3; k++) { w[k] = sgn * g[k]; w[3 + k] = sgn * t[k]; }
  }
  // contact order sum (lane 0 accumulates in index order, as the oracle does)
  for (int k = 0; k < 6; k++) {
    real acc = 0;
    for (int i = 0; i < GM_MAX_CON; i++) acc += readlane_real(w[k], i);
    out[k] = acc;
  }
}

// MjClass::monitor_sensors (mjclass.cpp:741-898)
template <int CL>
GM_EPI_ATTR void monitor_sensors(SharedT<CL>& S, const gm_model* __restrict__ m, const gm_config* __restrict__ C,
                                const GmTopo* __restrict__ T, int lane) {
  // (per-env LDS fields, no function-scope __shared__: substep_loop and monitor_sensors are
  // reached from two kernels, and such variables would cost a per-kernel offset lookup)
  if (lane == 0) S.bend_ready = s_ready(S.s, C->s.bending_gauge, SL_BEND);
  GM_WAVE_SYNC();
  const int bend_ready = S.bend_ready;
  if (bend_ready && lane < 3) S.gauge_tmp[lane] = gauge_reading<CL - 2>(m, &S.s.qpos[T->dof_f0[lane] + 2]);
  GM_WAVE_SYNC();
  if (lane == 0) {
    GmEnvHot& s = S.s;
  RingRef R = S.gs->ring;
    const gm_settings& st = C->s;
    int have = 0;
    if (bend_ready) {
      float g[3] = {S.gauge_tmp[0], S.gauge_tmp[1], S.gauge_tmp[2]};
      for (int f = 0; f < 3; f++) ring_add(s, R, ST_SI_GAUGE + f, (float)(g[f] * C->sim_gauge_raw_to_N_factor));
      for (int f = 0; f < 3; f++) g[f] = s_normalise(st.bending_gauge, g[f]);
      for (int f = 0; f < 3; f++) g[f] = s_noise(s, st.bending_gauge, SL_BEND, g[f], f + 1);
      for (int f = 0; f < 3; f++) ring_add(s, R, ST_GAUGE + f, g[f]);
    }
    if (s_ready(s, st.axial_gauge, SL_AXIAL)) {
      if (!have) { extract_forces(S, m, T); have = 1; }
      float a[3] = {S.forces[15], S.forces[16], S.forces[17]};
      for (int f = 0; f < 3; f++) ring_add(s, R, ST_SI_AXIAL + f, a[f]);
      for (int f = 0; f < 3; f++) a[f] = s_normalise(st.axial_gauge, a[f]);
      for (int f = 0; f < 3; f++) a[f] = s_noise(s, st.axial_gauge, SL_AXIAL, a[f], f + 1);
      for (int f = 0; f < 3; f++) ring_add(s, R, ST_AXIAL + f, a[f]);
    }
    if (s_ready(s, st.palm_sensor, SL_PALM)) {
      if (!have) { extract_forces(S, m, T); have = 1; }
      float p = S.forces[18];
      p *= st.palm_scale_factor;
      ring_add(s, R, ST_SI_PALM, p);
      p = s_normalise(st.palm_sensor, p);
      p = s_noise(s, st.palm_sensor, SL_PALM, p, 1);
      ring_add(s, R, ST_PALM, p);
    }
    if (s_ready(s, st.wrist_sensor_Z, SL_WRISTZ)) {
      float z = 0.0f;
      z -= st.wrist_sensor_Z.raw_value_offset;
      ring_add(s, R, ST_SI_WZ, z);
      z = s_normalise(st.wrist_sensor_Z, z);
      z = s_noise(s, st.wrist_sensor_Z, SL_WRISTZ, z, 1);
      ring_add(s, R, ST_WZ, z);
    }
  }
  GM_WAVE_SYNC();
}
