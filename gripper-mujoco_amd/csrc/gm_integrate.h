// gm_integrate.h -- physics stage 4, mj_Euler: implicit joint damping (gm_euler.h's
// euler_solve / euler_damping), the free object's quaternion step, and the calibration unit's
// mj_checkAcc.  SharedT: reads qacc, xs; writes s.qvel, s.qpos, s.time (s.badqacc).
#pragma once
#include "gm_euler.h"

GM_PHYSICS_BEGIN
// DUO workgroups: the helper wave's euler_factor results, lane-major ([j][64]: L[1..CL], lb,
// 1 / d), then the base pivot's Schur sum
template <int CL>
__device__ __forceinline__ real* duo_ef() {
  __shared__ real ef[64 * (CL + 2) + 1];
  return ef;
}

// ============================================================ integrate
template <int CL, bool CAL, bool DUO = false>
__device__ __forceinline__ void integrate(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T, int lane,
                                          bool prof = false) {
  const real h = CAL ? S.s.dt : m->timestep;
  if constexpr (CAL) {
    // mj_checkAcc's mjWARN_BADQACC (is_sim_unstable, myfunctions.cpp:4233-4242): a
    // non-finite or |qacc| > mjMAXVAL acceleration; sticky until the next reset
    const bool bad = lane < T->nv && !(fabs(S.qacc[lane]) <= 1e10);
    if (__ballot(bad) != 0ull && lane == 0) S.s.badqacc = 1;
  }
  // mj_Euler: under MuJoCo's actuator order the joint damping is implicit here
  // (euler_damping: qacc_e = (M + h D)^-1 (qfrc_smooth + qfrc_constraint) into S.xs)
  const bool mj = m->mujoco_actuators != 0;
  if constexpr (DUO) {
    // the helper factored M + h D during the constraint solve (duo_helper); third barrier
    __syncthreads();
    if (mj) {
      const int ln = fresh_lane();
      const real* ef = duo_ef<CL>();
      real L[CL + 1];
      L[0] = 0.0;
#pragma unroll
      for (int j = 1; j <= CL; j++) L[j] = ef[(j - 1) * 64 + ln];
      euler_solve<CL>(S, T, h, ln, L, ef[CL * 64 + ln], ef[(CL + 1) * 64 + ln], ef[64 * (CL + 2)]);
    }
  } else {
    if (mj) {
      // euler_damping, with the profiled instance's marks between its halves: the Euler
      // factor's and the Euler solve's clocks go to the upper halves of two counter columns
      // (gmx.env integrate_split); the rest of the stage is PH(8) minus the two
      unsigned long long t0 = prof ? clock64() : 0;
#define GM_PH_HI(k) do { if (__builtin_expect(prof, 0)) { unsigned long long t_ = clock64(); \
                         if (lane == 0) S.tph[k] += (t_ - t0) << 32; t0 = t_; } } while (0)
      const int ln = fresh_lane();
      real L[CL + 1], lb, invd;
      const real sch = euler_factor<CL>(S, T, h, ln, L, lb, invd);
      GM_PH_HI(28);
      euler_solve<CL>(S, T, h, ln, L, lb, invd, sch);
      GM_PH_HI(31);
#undef GM_PH_HI
    }
  }
  if (lane < T->nv) S.s.qvel[lane] += h * (mj ? S.xs[lane] : S.qacc[lane]);
  GM_WAVE_SYNC();
  if (lane < T->nv && lane < T->dof_obj) {
    S.s.qpos[lane] += h * S.s.qvel[lane];   // slides/hinges: qposadr == dofadr before the object
  }
  if (lane == 0) {
    int qa = T->qadr_obj, da = T->dof_obj;
    for (int k = 0; k < 3; k++) S.s.qpos[qa + k] += h * S.s.qvel[da + k];
    real* q = &S.s.qpos[qa + 3];
    real w[3] = {S.s.qvel[da + 3], S.s.qvel[da + 4], S.s.qvel[da + 5]};
    // (sqrt_n / div_n: the library operations' results wherever their range scaling is
    // inactive -- a |w| below 2^-383 takes the branch either way)
    real wn = sqrt_n(dot3(w, w));
    if (wn > 1e-15) {
      real ang = wn * h;
      real sn, cs;
      gm_sincos(0.5 * ang, &sn, &cs);
      sn = div_n(sn, wn);
      real dq[4] = {cs, w[0] * sn, w[1] * sn, w[2] * sn};
      quatmul(q, q, dq);
    }
    quatnorm(q);
    S.s.time += h;
  }
  GM_WAVE_SYNC();
}
GM_PHYSICS_END
using gmf::integrate, gmf::duo_ef;
