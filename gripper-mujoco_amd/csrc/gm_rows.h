// gm_rows.h -- the constraint rows of physics stage 3 (the constraint solve): MuJoCo's
// mj_makeConstraint / mj_makeImpedance with the mj_diagApprox regulariser, pyramidal cones.
// Row data lives with its lane: contact c's 4 pyramid edges on lane c, motor-lock row r on
// lane r.  gm_dynamics.h includes this file (crb_rne issues lock_rows in its first block), the
// Newton solve (gm_newton.hip) reads the rows; oracle/physics.c constraint_setup restates them.

// SharedT: reads con, cbody, ncon, cdof, s.qpos, s.qvel, s.qacc_warm, s.lock_*, s.obj_invw, s.dt;
// writes lrow_*, nl, nefc and the union's nw.V, nw2.V / V2.
#pragma once
#include "gm_real.h"

GM_PHYSICS_BEGIN
// ------------------------------------------------------------ constraint rows
// the solimp sigmoid's general power (cold on the canonical model): one pow pair serves
// both halves; outlined so the inlined fast path stays small
__device__ __noinline__ real impedance_pow(real x, real mid, real pw) {
  const bool lo = x <= mid;
  const real t = pow(lo ? x : 1 - x, pw) / pow(lo ? mid : 1 - mid, pw - 1);
  return lo ? t : 1 - t;
}
// mj_makeImpedance's sigmoid, branch-free in the data (the branches left test model
// constants, wave-uniform): the same values as the early-return form, so several calls can
// interleave their dependency chains
__device__ __forceinline__ real impedance(const gm_model* __restrict__ m, real r) {
  const real dmin = m->solimp[0], dmax = m->solimp[1], width = m->solimp[2];
  const real mid = m->solimp[3], pw = m->solimp[4];
  // a flat sigmoid (MuJoCo getimpedance: equal ends or a width under mjMINVAL): the mean of the ends
  if (dmin == dmax || width <= 1e-15) return 0.5 * (dmin + dmax);
  const real x = div_n(fabs(r), width);
  real y;
  if (pw == 2) {   // MuJoCo's default power
    const bool lo = x <= mid;
    const real q = div_n(lo ? x * x : (1 - x) * (1 - x), lo ? mid : 1 - mid);
    y = lo ? q : 1 - q;
  } else if (pw == 1) {
    y = x;
  } else {
    y = impedance_pow(x, mid, pw);
  }
  real imp = dmin + y * (dmax - dmin);
  imp = (x >= 1) ? dmax : imp;
  imp = (x <= 0) ? dmin : imp;
  return imp;
}

// spatial velocity [angular; linear at the world origin] of every body for NVEC dof
// vectors v[0..NVEC) (LDS) into V[0..NVEC): chain prefix scans on the scan lanes plus the
// base, the object's free joint (two vectors scan interleaved: one pass of latency)
template <int CL, int NVEC>
__device__ void body_vel(SharedT<CL>& S, const real* const* v, real (*const* V)[6], const gm_model* __restrict__ m,
                         const GmTopo* __restrict__ T, int lane, bool obj_only = false) {
  // obj_only (wave-uniform): every contact is the object on the ground, so only the
  // object's velocity (and the world's zero) is read: the chain scans are skipped
  const int db = T->dof_base;
  const int grp = T->kl_grp[lane];
  const bool chain = grp >= 0 && grp <= 3;
  const int p = T->kl_cpos[lane];
  const int d = chain ? (grp < 3 ? T->dof_f0[grp] + p - 1 : T->dof_palm) : db;
  real cvb[NVEC][6], s[NVEC][6];
#pragma unroll
  for (int n = 0; n < NVEC; n++) {
    const real vb = v[n][db];
    const real vd = chain ? v[n][d] : 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      cvb[n][k] = S.cdof[db][k] * vb;
      const real c = S.cdof[d][k];   // (d: the base dof off the chains; loaded, then selected)
      s[n][k] = (chain ? c : 0.0) * vd;
    }
  }
  if (!obj_only) {
#pragma unroll
    for (int off = 1; off < CL; off <<= 1)
#pragma unroll
      for (int n = 0; n < NVEC; n++)
#pragma unroll
        for (int k = 0; k < 6; k++) s[n][k] += row_shr(s[n][k], off);
  }
  const int b = T->lane_body[lane];
  if (chain && !obj_only) {
#pragma unroll
    for (int n = 0; n < NVEC; n++)
#pragma unroll
      for (int k = 0; k < 6; k++) V[n][b][k] = s[n][k] + cvb[n][k];
  } else if (lane == T->lane_base && !obj_only) {
#pragma unroll
    for (int n = 0; n < NVEC; n++)
#pragma unroll
      for (int k = 0; k < 6; k++) V[n][T->body_base][k] = cvb[n][k];
#ifndef GM_NO_OBJECT_LANES
  } else if (lane >= GM_OBJ_LANE0 && lane < GM_OBJ_LANE0 + 6) {
    // the object's free joint, one component per lane (the lanes euler_solve gives the
    // object dofs; gm_shared.h asserts that they hold no chain link, base, palm or object,
    // so the branches above never take them): component t sums its six products from +0
    // in dof order, the one-lane loop's additions for that component, operand for operand
    const int d0 = T->dof_obj, t = lane - GM_OBJ_LANE0;
    real co[6], vk[NVEC][6], acc[NVEC];
#pragma unroll
    for (int k = 0; k < 6; k++) {
      co[k] = S.cdof[d0 + k][t];
#pragma unroll
      for (int n = 0; n < NVEC; n++) vk[n][k] = v[n][d0 + k];
    }
    keep_n<6>(co);
#pragma unroll
    for (int n = 0; n < NVEC; n++) acc[n] = 0;
#pragma unroll
    for (int k = 0; k < 6; k++)
#pragma unroll
      for (int n = 0; n < NVEC; n++) acc[n] += co[k] * vk[n][k];
#pragma unroll
    for (int n = 0; n < NVEC; n++) V[n][T->body_obj][t] = acc[n];
#else
  } else if (b == T->body_obj) {
    const int d0 = T->dof_obj;
    real acc[NVEC][6];
#pragma unroll
    for (int n = 0; n < NVEC; n++)
#pragma unroll
      for (int t = 0; t < 6; t++) acc[n][t] = 0;
#pragma unroll
    for (int k0 = 0; k0 < 6; k0 += 3) {
      real co[18], vk[NVEC][3];   // three object dofs' subspaces and velocities, one batch
#pragma unroll
      for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int t = 0; t < 6; t++) co[6 * k + t] = S.cdof[d0 + k0 + k][t];
#pragma unroll
        for (int n = 0; n < NVEC; n++) vk[n][k] = v[n][d0 + k0 + k];
      }
      keep_n<18>(co);
#pragma unroll
      for (int k = 0; k < 3; k++)
#pragma unroll
        for (int n = 0; n < NVEC; n++)
#pragma unroll
          for (int t = 0; t < 6; t++) acc[n][t] += co[6 * k + t] * vk[n][k];
    }
#pragma unroll
    for (int n = 0; n < NVEC; n++)
#pragma unroll
      for (int t = 0; t < 6; t++) V[n][b][t] = acc[n][t];
#endif
  } else if (lane == 0) {
#pragma unroll
    for (int n = 0; n < NVEC; n++)
#pragma unroll
      for (int k = 0; k < 6; k++) V[n][0][k] = 0.0;
  }
  GM_WAVE_SYNC();
}

// J v of contact c's 4 pyramid edges from the body velocities V (n + mu t1, n - mu t1,
// n + mu t2, n - mu t2)
template <int CL>
__device__ __forceinline__ void contact_jv(const SharedT<CL>& S, const real (*V)[6], const gm_model* __restrict__ m,
                                           int c, real* jv) {
  const real* C = S.con[c];
  const int b1 = S.cbody[c][0], b2 = S.cbody[c][1];
  const real pos[3] = {C[1], C[2], C[3]};
  real t1v[3], t2v[3];
  cross3(t1v, V[b1], pos);
  cross3(t2v, V[b2], pos);
  const real v1[3] = {V[b1][3] + t1v[0], V[b1][4] + t1v[1], V[b1][5] + t1v[2]};
  const real v2[3] = {V[b2][3] + t2v[0], V[b2][4] + t2v[1], V[b2][5] + t2v[2]};
  const real dv[3] = {v2[0] - v1[0], v2[1] - v1[1], v2[2] - v1[2]};
  const real n[3] = {C[4], C[5], C[6]}, t1[3] = {C[7], C[8], C[9]};
  real t2[3];
  cross3(t2, n, t1);
  const real mu = C[10];
  const real cn = dot3(n, dv), c1 = dot3(t1, dv), c2 = dot3(t2, dv);
  const real m1 = mu * c1, m2 = mu * c2;
  jv[0] = cn + m1; jv[1] = cn - m1; jv[2] = cn + m2; jv[3] = cn - m2;
}
// pyramid edge direction u_e of contact record C
__device__ __forceinline__ void edge_dir(const real* C, const real* t2, int ed, real* u) {
  const real* t = (ed >> 1) ? t2 : C + 7;
  const real mt[3] = {C[10] * t[0], C[10] * t[1], C[10] * t[2]};
  if (ed & 1) { u[0] = C[4] - mt[0]; u[1] = C[5] - mt[1]; u[2] = C[6] - mt[2]; }
  else { u[0] = C[4] + mt[0]; u[1] = C[5] + mt[1]; u[2] = C[6] + mt[2]; }
}

// xor butterfly over the wave: every lane ends with the same sum (oracle butterfly64)
__device__ __forceinline__ real wave_sum(real v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s);
  return v;
}

// Row data lives with its lane: contact c's 4 edges on lane c (D, aref, jar at the
// iterate q, at the Newton point x), motor-lock row r on lane r (its own registers).
struct RowsT {
  real cD, caref[4], cjq[4], cjx[4];   // contact lane
  real lD, laref, ljq, ljx;            // lock lane
  int ldof;
};

// The motor-lock rows (1-dof joint equalities) of the constraint problem: impedance, the
// regulariser R = (1 - d) / d dof_invweight0 and the reference acceleration of each active
// lock, row r on lane r, into S.lrow_* and S.nl.  They need only qpos, qvel and the motion
// subspaces, so crb_rne issues them in its first basic block: their division chains fill
// the scans' latency instead of running as a phase of their own.
template <int CL, bool CAL>
__device__ __forceinline__ void lock_rows(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T, int lane) {
  const real h = CAL ? S.s.dt : m->timestep;
  real tc = m->solref[0];
  if (tc < 2 * h) tc = 2 * h;
  const real dr = m->solref[1], dmax = m->solimp[1];
  const real K = rcp_n(dmax * dmax * tc * tc * dr * dr);
  const real Bd = div_n(2.0, dmax * tc);
  // lock rows: row r (lane r) is the r-th active lock.  The lock behind each row is picked
  // branch-free from the (wave-uniform) active flags and its constants from uniform scalar
  // loads, and the weld's per-axis rows are evaluated side by side: no divergent search
  // loop, no per-lane global loads, three independent dependency chains instead of one.
  int nl = 0, k = 0, d = 0;
  real tran = 0.0;
#pragma unroll
  for (int kk = 0; kk < GM_MAX_LOCK; kk++) {
    const bool act = kk < T->nlock && S.s.lock_active[kk];
    const bool mine = act && nl == lane;
    k = mine ? kk : k;
    d = mine ? m->lock_dof[kk] : d;
    tran = mine ? T->lock_tran[kk] : tran;
    nl += act ? 1 : 0;
  }
  {
    const real pos = S.s.qpos[d] - S.s.lock_q[k];
    const real vel = S.s.qvel[d];
    // the reference's weld on a slide as one row on the dof (oracle constraint_setup):
    // per world axis r the weld row a_r qdot with its own impedance and the weld's
    // regulariser, summed in axis order: D = sum D_r a_r^2, D aref = sum D_r a_r aref_r
    real Da[3], ar[3], av[3];
    bool on[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const real a = S.cdof[d][3 + r];
      av[r] = a;
      on[r] = a != 0.0;
      const real pr = a * pos, vr = a * vel;
      const real imp = impedance(m, pr);
      real Rr = div_n(1 - imp, imp) * tran;
      if (Rr < 1e-15) Rr = 1e-15;
      Da[r] = rcp_n(Rr) * a;
      ar[r] = -Bd * vr - K * imp * pr;
    }
    real De = 0.0, Dar = 0.0;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      De = on[r] ? De + Da[r] * av[r] : De;
      Dar = on[r] ? Dar + Da[r] * ar[r] : Dar;
    }
    // every lane stores (lanes past the active rows into the spare slot GM_MAX_LOCK): no
    // branch, so the whole computation stays in one basic block with the caller's
    const int slot = lane < nl ? lane : GM_MAX_LOCK;
    S.lrow_D[slot] = De;
    S.lrow_aref[slot] = div_n(Dar, De);
    S.lrow_dof[slot] = d;
  }
  S.nl = nl;   // (wave-uniform: every lane stores the same value)
}

// The contact rows of the constraint setup (mj_makeConstraint / mj_makeImpedance for the
// pyramid edges): body velocities at qvel (reference accelerations) and at the warm start
// (the first iterate's J q - aref) into V / V2, one fused pass; then per contact lane the
// edges' D = 1 / R (R = (1 - d) / d diagApprox, diagApprox = tran + mu^2 tran, tran = the two
// bodies' invweight0), their aref and the warm start's J q - aref.  The owner wave runs it
// inside constraint_setup; in a DUO workgroup the helper runs it right after its collider
// (duo_helper: it needs only the contacts, the motion subspaces and qvel / qacc_warm) and
// hands the rows over in LDS (duo_rows) -- the same code on the same operands.
template <int CL, bool CAL>
__device__ __forceinline__ void contact_rows(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T,
                                             int lane, real (*V)[6], real (*V2)[6], real& cD, real* caref, real* jq,
                                             bool& obj_only) {
  const real h = CAL ? S.s.dt : m->timestep;
  real tc = m->solref[0];
  if (tc < 2 * h) tc = 2 * h;
  const real dr = m->solref[1], dmax = m->solimp[1];
  const real K = rcp_n(dmax * dmax * tc * tc * dr * dr);
  const real Bd = div_n(2.0, dmax * tc);
  {
    const real* vv[2] = {S.s.qvel, S.s.qacc_warm};
    real (*VV[2])[6] = {V, V2};
    bool og = true;
    if (lane < S.ncon) {
      const int b1 = S.cbody[lane][0], b2 = S.cbody[lane][1];
      og = (b1 == 0 && b2 == T->body_obj) || (b2 == 0 && b1 == T->body_obj);
    }
    obj_only = __ballot(!og) == 0ull;
    body_vel<CL, 2>(S, vv, VV, m, T, lane, obj_only);
  }
#pragma unroll
  for (int e = 0; e < 4; e++) jq[e] = 0.0;
  cD = 0;
#pragma unroll
  for (int e = 0; e < 4; e++) caref[e] = 0;
  if (lane < S.ncon) {
    const real* C = S.con[lane];
    const int b1 = S.cbody[lane][0], b2 = S.cbody[lane][1];
    const real oiw = S.s.obj_invw[0], biw1 = m->body_invweight0[b1][0], biw2 = m->body_invweight0[b2][0];
    const real iw1 = (b1 == T->body_obj) ? oiw : biw1;
    const real iw2 = (b2 == T->body_obj) ? oiw : biw2;
    const real tran = iw1 + iw2;
    const real mu = C[10];
    const real diag = tran + (mu * mu) * tran;
    const real imp = impedance(m, C[0]);
    real Rr = div_n(1 - imp, imp) * diag;
    if (Rr < 1e-15) Rr = 1e-15;
    cD = rcp_n(Rr);
    real vel[4], jv[4];
    contact_jv<CL>(S, V, m, lane, vel);
    contact_jv<CL>(S, V2, m, lane, jv);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      caref[e] = -Bd * vel[e] - K * imp * C[0];
      jq[e] = jv[e] - caref[e];
    }
  }
}

// DUO workgroups: the contact rows the helper formed (contact_rows), contact-lane-major
template <int CL>
struct DuoRows {
  real cD[GM_MAX_CON], caref[4][GM_MAX_CON], jq[4][GM_MAX_CON];
  int32_t obj_only;
};
template <int CL>
__device__ __forceinline__ DuoRows<CL>* duo_rows() {
  __shared__ DuoRows<CL> r;
  return &r;
}

// constraint setup (mj_makeConstraint / mj_makeImpedance): impedance, the regulariser
// R = (1 - d) / d diagApprox (lock rows: dof_invweight0; pyramid edges:
// tran + mu^2 tran, tran = the two bodies' invweight0), reference accelerations
template <int CL, bool CAL, bool DUO = false>
__device__ void constraint_setup(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T,
                                 int lane, RowsT& R, real* jq, real& jql, bool& obj_only, bool prof = false) {
  unsigned long long t0 = prof ? clock64() : 0;
  (void)t0;
  // lock rows: formed in crb_rne's first block (lock_rows above) and read back here
  const int nl = S.nl;
  R.lD = 0; R.laref = 0; R.ldof = 0;
  if (lane < GM_MAX_LOCK) { R.lD = S.lrow_D[lane]; R.laref = S.lrow_aref[lane]; R.ldof = S.lrow_dof[lane]; }
  if (lane >= nl) { R.lD = 0; R.laref = 0; R.ldof = 0; }
  if (lane == 0) S.nefc = nl + 4 * S.ncon;
  if constexpr (DUO) {
    // formed by the helper wave after its collider (duo_helper), read after the barrier
    const DuoRows<CL>* dr = duo_rows<CL>();
    obj_only = dr->obj_only != 0;
    R.cD = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) { R.caref[e] = 0; jq[e] = 0.0; }
    if (lane < S.ncon) {
      R.cD = dr->cD[lane];
#pragma unroll
      for (int e = 0; e < 4; e++) { R.caref[e] = dr->caref[e][lane]; jq[e] = dr->jq[e][lane]; }
    }
  } else {
    contact_rows<CL, CAL>(S, m, T, lane, S.nw2.V, S.nw2.V2, R.cD, R.caref, jq, obj_only);
  }
  {
    const real qw = S.s.qacc_warm[R.ldof];   // (ldof = 0 off the lock lanes)
    jql = (lane < nl) ? qw - R.laref : 0.0;
  }
  GM_WAVE_SYNC();
}

// J v - aref for every row at the dof vector v (LDS); into jr (contact) / jl (lock)
template <int CL>
__device__ __forceinline__ void rows_jar(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T, bool obj_only,
                                         const real* v, int lane, const RowsT& R, real* jr, real& jl) {
  {
    const real* vv[1] = {v};
    real (*VV[1])[6] = {S.nw.V};
    body_vel<CL, 1>(S, vv, VV, m, T, lane, obj_only);
  }
  jl = (lane < S.nl) ? v[R.ldof] - R.laref : 0.0;
  if (lane < S.ncon) {
    real jv[4];
    contact_jv<CL>(S, S.nw.V, m, lane, jv);
#pragma unroll
    for (int e = 0; e < 4; e++) jr[e] = jv[e] - R.caref[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++) jr[e] = 0.0;
  }
}

// per-lane partial of a row sum (contact edges in order, then the lane's lock row) and the
// wave butterfly (oracle row_reduce)
__device__ __forceinline__ real row_sum(int lane, int ncon, int nl, const real* tc, real tl) {
  real a = 0.0;
  if (lane < ncon) a = ((tc[0] + tc[1]) + tc[2]) + tc[3];
  if (lane < nl) a = a + tl;
  return wave_sum(a);
}
GM_PHYSICS_END
using gmf::contact_rows, gmf::duo_rows, gmf::DuoRows;
