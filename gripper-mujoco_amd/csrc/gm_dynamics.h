// gm_dynamics.h -- physics stage 1, the smooth dynamics: mj_kinematics (oracle.c fk), mj_rne /
// mj_crb, the H~ rows and the smooth force per dof (with the calibration tip load,
// myfunctions.cpp:1642-1727).  SharedT: reads s.qpos, s.qvel, s.next, s.base; writes xpos, xquat,
// cdof, cinert / Ic, cfrc, chain_f, chain_I, Hf, Hp, Ho, Hbb, frc (and lock_rows' lrow_*, nl;
// crb_rne hands the object's three cross products over in go, dead until the Newton point).
#pragma once
#include "gm_real.h"
#include "gm_rows.h"

// ============================================================ kinematics
// mj_kinematics restated (oracle.c fk): phase A, one lane per body, the hinge joint
// rotations (the only transcendental work) ; phase B, one lane per chain, the pose
// recursion root -> leaf entirely in registers (chain length compile-time, unrolled,
// every model constant load independent of the recursion) ; phase C, one lane per
// body / dof / geom: rotation matrices, world-origin spatial inertias, motion
// subspaces, geom poses.
struct Pose { real p[3], q[4], R[9]; };

GM_PHYSICS_BEGIN
template <int CL>
__device__ __forceinline__ void kinematics(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T, int lane,
                           bool prof = false) {
  unsigned long long t0 = prof ? clock64() : 0;
  // A: local transform of every body (model constants + its joint), lane = body:
  //    slide  p = bpos + R(bquat) axis q,  quat = bquat
  //    hinge  p = bpos,                    quat = bquat (x) (cos q/2, axis sin q/2)
  // every constant below is one load from the lane's flattened GmTopo entry (identity
  // transform and no joint on lanes without a body)
  real lp[3], lq[4], ax[3] = {0, 0, 0};
  const int b = T->lane_body[lane];   // scan-lane layout (GmTopo::lane_body)
  const int type = T->kl_type[lane];
  ld3(lp, T->kl_pos[lane]);
  ld4(lq, T->kl_quat[lane]);
  if (type >= 0) {
    const real qv = S.s.qpos[T->kl_qadr[lane]];
    ld3(ax, T->kl_axis[lane]);
    if (type == GM_JNT_SLIDE) {
      real R[9], wa[3];
      quat2mat(R, lq);
      mulmv3(wa, R, ax);
      lp[0] += wa[0] * qv; lp[1] += wa[1] * qv; lp[2] += wa[2] * qv;
    } else if (type == GM_JNT_HINGE) {
      real sn, cs;
      gm_sincos(0.5 * qv, &sn, &cs);   // shared with the oracle (gm_math.h)
      const real ql[4] = {cs, ax[0] * sn, ax[1] * sn, ax[2] * sn};
      quatmul(lq, lq, ql);
    }
  }
  PH(15);
  // B: poses.  The base is the world's child; along each finger / palm chain the
  // local transforms are composed by a segmented inclusive scan (root-side operand on
  // the left: (p_a, q_a) o (p_b, q_b) = (p_a + R(q_a) p_b, q_a (x) q_b)), then the base
  // pose is applied and the orientation renormalised.  Every body other than the world has
  // a scan lane (chain links, palm, base, object), which keeps its pose in registers for C.
  const int bb = T->body_base;
  const int grp = T->kl_grp[lane];
  const bool chain = grp >= 0 && grp <= 3;
  const bool is_obj = b == T->body_obj;
  real xp[3], xq[4];
  {
    const int lb = T->lane_base;
    real bpos[3], bq[4];
#pragma unroll
    for (int k = 0; k < 3; k++) bpos[k] = readlane_real(lp[k], lb);
#pragma unroll
    for (int k = 0; k < 4; k++) bq[k] = readlane_real(lq[k], lb);
    quatnorm(bq);
    real bR[9];
    quat2mat(bR, bq);
    const int p = T->kl_cpos[lane];
#pragma unroll
    for (int off = 1; off < CL; off <<= 1) {
      real np[3], nq[4];
#pragma unroll
      for (int k = 0; k < 3; k++) np[k] = row_shr(lp[k], off);
#pragma unroll
      for (int k = 0; k < 4; k++) nq[k] = row_shr(lq[k], off);
      if (p > off) {
        real R[9], t[3], q[4];
        quat2mat(R, nq);
        mulmv3(t, R, lp);
        quatmul(q, nq, lq);
        lp[0] = np[0] + t[0]; lp[1] = np[1] + t[1]; lp[2] = np[2] + t[2];
        lq[0] = q[0]; lq[1] = q[1]; lq[2] = q[2]; lq[3] = q[3];
      }
    }
    if (chain) {
      real t[3];
      mulmv3(t, bR, lp);
      quatmul(xq, bq, lq);
      quatnorm(xq);
      xp[0] = bpos[0] + t[0]; xp[1] = bpos[1] + t[1]; xp[2] = bpos[2] + t[2];
    } else if (is_obj) {
      // object: free joint, pose straight from qpos
      const int qa = T->qadr_obj;
      xq[0] = S.s.qpos[qa + 3]; xq[1] = S.s.qpos[qa + 4]; xq[2] = S.s.qpos[qa + 5]; xq[3] = S.s.qpos[qa + 6];
      quatnorm(xq);
      xp[0] = S.s.qpos[qa]; xp[1] = S.s.qpos[qa + 1]; xp[2] = S.s.qpos[qa + 2];
    } else {   // the base lane (the rest hold no body and store nothing)
      xp[0] = bpos[0]; xp[1] = bpos[1]; xp[2] = bpos[2];
      xq[0] = bq[0]; xq[1] = bq[1]; xq[2] = bq[2]; xq[3] = bq[3];
    }
  }
  PH(16);
  // C, on the body's scan lane from the pose in registers: the pose itself, the
  // world-origin spatial inertia and the motion subspace of the body's dof(s) (the
  // object's six)
  if (b > 0) {
    real R[9];
    quat2mat(R, xq);
    S.xpos[b][0] = xp[0]; S.xpos[b][1] = xp[1]; S.xpos[b][2] = xp[2];
#pragma unroll
    for (int k = 0; k < 4; k++) S.xquat[b][k] = xq[k];
    real ip[3], c[3];
    ld3(ip, m->body_ipos[b]);
    mulmv3(c, R, ip);
    c[0] += xp[0]; c[1] += xp[1]; c[2] += xp[2];
    real I[3] = {(real)m->body_inertia[b][0], (real)m->body_inertia[b][1], (real)m->body_inertia[b][2]};
    real mass = (real)m->body_mass[b];
    if (is_obj) {
      mass = S.s.obj_mass;
      I[0] = S.s.obj_inertia[0]; I[1] = S.s.obj_inertia[1]; I[2] = S.s.obj_inertia[2];
    }
    real Iw[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int k = 0; k < 3; k++)
        Iw[3 * i + k] = R[3 * i] * I[0] * R[3 * k] + R[3 * i + 1] * I[1] * R[3 * k + 1] + R[3 * i + 2] * I[2] * R[3 * k + 2];
    const real cc = dot3(c, c);
    real* ci = S.cinert[b];
    ci[0] = Iw[0] + mass * (cc - c[0] * c[0]);
    ci[1] = Iw[4] + mass * (cc - c[1] * c[1]);
    ci[2] = Iw[8] + mass * (cc - c[2] * c[2]);
    ci[3] = Iw[1] - mass * c[0] * c[1];
    ci[4] = Iw[2] - mass * c[0] * c[2];
    ci[5] = Iw[5] - mass * c[1] * c[2];
    ci[6] = mass * c[0]; ci[7] = mass * c[1]; ci[8] = mass * c[2];
    ci[9] = mass;
    if (is_obj) {
      // free joint: translations along the world axes, rotations about the body axes
      // through the body origin
      const int d0 = T->dof_obj;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        real* cd = S.cdof[d0 + k];
        cd[0] = cd[1] = cd[2] = 0; cd[3] = cd[4] = cd[5] = 0; cd[3 + k] = 1;
      }
#pragma unroll
      for (int k = 0; k < 3; k++) {
        real* cd = S.cdof[d0 + 3 + k];
        const real w[3] = {R[k], R[3 + k], R[6 + k]};
        cd[0] = w[0]; cd[1] = w[1]; cd[2] = w[2];
        cross3(cd + 3, xp, w);
      }
    } else {
      // the body's one joint (slide / hinge; kl_axis = the joint's dof axis)
      const int d = chain ? (grp < 3 ? T->dof_f0[grp] + T->kl_cpos[lane] - 1 : T->dof_palm) : T->dof_base;
      real* cd = S.cdof[d];
      real wa[3];
      mulmv3(wa, R, ax);
      if (type == GM_JNT_SLIDE) {
        cd[0] = cd[1] = cd[2] = 0; cd[3] = wa[0]; cd[4] = wa[1]; cd[5] = wa[2];
      } else {
        cd[0] = wa[0]; cd[1] = wa[1]; cd[2] = wa[2];
        cross3(cd + 3, xp, wa);   // anchor at the body origin in this model
      }
    }
  }
  GM_WAVE_SYNC();
}

// ============================================================ CRB + RNE
// mj_rne (bias forces, world-origin spatial algebra) and mj_crb (composite inertias):
// forward velocity / bias-acceleration recursion and body forces per chain, then
// leaf -> root running sums in registers; chain-root totals meet at the base body.
template <int CL>
__device__ __forceinline__ void body_force(SharedT<CL>& S, int b, const real* cvel, const real* cacc) {
  real ci[10], t1[6], t2[6], f[6];
#pragma unroll
  for (int k = 0; k < 10; k++) ci[k] = S.cinert[b][k];
  inert_mul(f, ci, cacc);
  inert_mul(t1, ci, cvel);
  cross_force(t2, cvel, t1);
#pragma unroll
  for (int k = 0; k < 6; k++) S.cfrc[b][k] = f[k] + t2[k];
}
template <int CL>
__device__ __forceinline__ void rne_fwd(SharedT<CL>& S, int b, int d, real* cvel, real* cacc) {
  real cd[6], cdd[6];
#pragma unroll
  for (int k = 0; k < 6; k++) cd[k] = S.cdof[d][k];
  cross_motion(cdd, cvel, cd);
  const real qv = S.s.qvel[d];
#pragma unroll
  for (int k = 0; k < 6; k++) { cvel[k] += cd[k] * qv; cacc[k] += cdd[k] * qv; }
  body_force(S, b, cvel, cacc);
}
// backward running sums over bodies b0 .. b0+L-1 (leaf = last); writes cfrc / Ic
template <int L, int CL>
__device__ __forceinline__ void chain_sums(SharedT<CL>& S, int b0, real* fs, real* Is) {
#pragma unroll
  for (int k = 0; k < 6; k++) fs[k] = 0;
#pragma unroll
  for (int k = 0; k < 10; k++) Is[k] = 0;
#pragma unroll
  for (int p = L; p >= 1; p--) {
    const int b = b0 + p - 1;
#pragma unroll
    for (int k = 0; k < 6; k++) { fs[k] += S.cfrc[b][k]; S.cfrc[b][k] = fs[k]; }
#pragma unroll
    for (int k = 0; k < 10; k++) { Is[k] = S.cinert[b][k] + (p < L ? Is[k] : 0.0); S.Ic[b][k] = Is[k]; }
  }
}

template <int CL, bool CAL>
__device__ __forceinline__ void crb_rne(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T, int lane,
                        bool prof = false) {
  unsigned long long t0 = prof ? clock64() : 0;
  // the constraint problem's lock rows ride in this phase's first block (see lock_rows)
  lock_rows<CL, CAL>(S, m, T, lane);
  // Lanes = bodies.  Along each finger / palm chain the velocities and bias accelerations
  // are segmented prefix sums and the composite forces / inertias segmented suffix sums
  // (Hillis-Steele over the chain position, shuffles within the wave); the base body is
  // the common root and the free object is handled by its own lane.
  const int db = T->dof_base;
  const real qdb = S.s.qvel[db];
  real cvb[6], cab[6];
#pragma unroll
  for (int k = 0; k < 6; k++) { cvb[k] = S.cdof[db][k] * qdb; cab[k] = 0; }
  cab[3] = -(real)m->gravity[0]; cab[4] = -(real)m->gravity[1]; cab[5] = -(real)m->gravity[2];

  const int b = T->lane_body[lane];   // scan-lane layout (GmTopo::lane_body)
  const int grp = T->kl_grp[lane];
  const bool chain = grp >= 0 && grp <= 3;
  const int p = T->kl_cpos[lane];
  const int d = chain ? (grp < 3 ? T->dof_f0[grp] + p - 1 : T->dof_palm) : db;
  real cd[6], v[6];
  // (operands loaded on every lane -- d is the base dof off the chains -- and selected: a
  // select instead of a divergent branch around each load)
  const real qvd = S.s.qvel[d];
  const real qd = chain ? qvd : 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) { const real c = S.cdof[d][k]; cd[k] = chain ? c : 0.0; v[k] = cd[k] * qd; }
  // The scans add their shifted operand unconditionally: every source outside a lane's
  // chain segment holds an exact zero (the empty position 0 of each finger row, the base
  // lane before the palm, the no-body lanes past the chain end, the zero-inertia object
  // lane, and DPP's bound_ctrl zero past the row edge), so the old p > off / p + off <= Lc
  // selects only cost two v_cndmask per double per step.  The sums of nonzero terms keep
  // the scan's association; only the sign of an exactly-zero entry can differ.
  // velocities: inclusive prefix along the chain, then the base contribution
  real cv[6];
#pragma unroll
  for (int k = 0; k < 6; k++) cv[k] = v[k];
#pragma unroll
  for (int off = 1; off < CL; off <<= 1) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const real nb = row_shr(cv[k], off);
      cv[k] += nb;
    }
  }
  real cvp[6];
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const real nb = row_shr(cv[k], 1);
    cvp[k] = cvb[k] + (p > 1 ? nb : 0.0);
    cv[k] += cvb[k];
  }
  // bias accelerations: prefix of (cvel_parent x cdof) qd
  real ca[6];
  cross_motion(ca, cvp, cd);
#pragma unroll
  for (int k = 0; k < 6; k++) ca[k] *= qd;
#pragma unroll
  for (int off = 1; off < CL; off <<= 1) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const real nb = row_shr(ca[k], off);
      ca[k] += nb;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; k++) ca[k] += cab[k];
  // body forces I a + v x* (I v), then suffix sums of forces and inertias
  real ci[10], f[6];
#pragma unroll
  for (int k = 0; k < 10; k++) { const real c = S.cinert[b < 0 ? 0 : b][k]; ci[k] = chain ? c : 0.0; }
  {
    real t1[6], t2[6];
    inert_mul(f, ci, ca);
    inert_mul(t1, ci, cv);
    cross_force(t2, cv, t1);
#pragma unroll
    for (int k = 0; k < 6; k++) f[k] += t2[k];
  }
#pragma unroll
  for (int off = 1; off < CL; off <<= 1) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const real nb = row_shl(f[k], off);
      f[k] += nb;
    }
#pragma unroll
    for (int k = 0; k < 10; k++) {
      const real nb = row_shl(ci[k], off);
      ci[k] += nb;
    }
  }
  if (chain) {
#pragma unroll
    for (int k = 0; k < 6; k++) S.cfrc[b][k] = f[k];
#pragma unroll
    for (int k = 0; k < 10; k++) S.Ic[b][k] = ci[k];
    if (p == 1) {
#pragma unroll
      for (int k = 0; k < 6; k++) S.chain_f[grp][k] = f[k];
#pragma unroll
      for (int k = 0; k < 10; k++) S.chain_I[grp][k] = ci[k];
    }
  }
#ifndef GM_NO_OBJECT_LANES
  {
    // object: free joint on one body.  Its velocity and bias-acceleration sums run one
    // component t per lane on lanes GM_OBJ_LANE0 + t and the three cross_motion one rotation
    // dof k per lane on lanes GM_OBJ_LANE0 + k, each sum in the one-lane loop's order (from
    // +0 / the gravity term, k = 0 .. 2); every lane issues them on a clamped index, so there
    // is no divergent branch, and only those six lanes are read.  cvel after the translations
    // reaches the cross products by readlane, their 18 results change lanes through S.go
    // (dead between two Newton points), and the finished cvel / cacc reach body_force as
    // wave-uniform operands.
    const int d0 = T->dof_obj;
    const int ol = lane - GM_OBJ_LANE0;
    const int t = ol < 0 ? 0 : (ol > 5 ? 5 : ol);
    const int kr = t < 3 ? t : 2;
    real qv[6], cdt[6], cdk[6];
#pragma unroll
    for (int k = 0; k < 6; k++) { qv[k] = S.s.qvel[d0 + k]; cdt[k] = S.cdof[d0 + k][t]; cdk[k] = S.cdof[d0 + 3 + kr][k]; }
    real cvt = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) cvt += cdt[k] * qv[k];
    real cw[6], cdd[6];
#pragma unroll
    for (int k = 0; k < 6; k++) cw[k] = readlane_real(cvt, GM_OBJ_LANE0 + k);
    cross_motion(cdd, cw, cdk);
    if (ol >= 0 && ol < 3) {
#pragma unroll
      for (int k = 0; k < 6; k++) S.go[6 * ol + k] = cdd[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) cvt += cdt[3 + k] * qv[3 + k];
    GM_WAVE_SYNC();
    real cat = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) cat = (t == 3 + k) ? -(real)m->gravity[k] : cat;
#pragma unroll
    for (int k = 0; k < 3; k++) cat += S.go[6 * k + t] * qv[3 + k];
    real cvel[6], cacc[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
      cvel[k] = readlane_real(cvt, GM_OBJ_LANE0 + k);
      cacc[k] = readlane_real(cat, GM_OBJ_LANE0 + k);
    }
    if (b == T->body_obj) body_force(S, b, cvel, cacc);
  }
#else
  if (b == T->body_obj) {
    // object: free joint on one body
    const int d0 = T->dof_obj;
    real cvel[6], cacc[6];
#pragma unroll
    for (int k = 0; k < 6; k++) { cvel[k] = 0; cacc[k] = 0; }
    cacc[3] = -(real)m->gravity[0]; cacc[4] = -(real)m->gravity[1]; cacc[5] = -(real)m->gravity[2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const real qv = S.s.qvel[d0 + k];
#pragma unroll
      for (int t = 0; t < 6; t++) cvel[t] += S.cdof[d0 + k][t] * qv;
    }
    real cdd[3][6];
#pragma unroll
    for (int k = 0; k < 3; k++) cross_motion(cdd[k], cvel, S.cdof[d0 + 3 + k]);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const real qv = S.s.qvel[d0 + 3 + k];
#pragma unroll
      for (int t = 0; t < 6; t++) cvel[t] += S.cdof[d0 + 3 + k][t] * qv;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const real qv = S.s.qvel[d0 + 3 + k];
#pragma unroll
      for (int t = 0; t < 6; t++) cacc[t] += cdd[k][t] * qv;
    }
    body_force(S, b, cvel, cacc);
  }
#endif
  GM_WAVE_SYNC();
  PH(17);
  // base body: its own inertia / force plus the four chain roots, one lane per value
  // (lanes 0..9 the composite inertia, 10..15 the force; the base's own body force is
  // formed on every lane from its uniform operands, the same operations as body_force)
  {
    const int bb = T->body_base;
    real ci[10], t1[6], t2[6], fo[6];
#pragma unroll
    for (int k = 0; k < 10; k++) ci[k] = S.cinert[bb][k];
    inert_mul(fo, ci, cab);
    inert_mul(t1, ci, cvb);
    cross_force(t2, cvb, t1);
#pragma unroll
    for (int k = 0; k < 6; k++) fo[k] = fo[k] + t2[k];
    const bool isI = lane < 10;
    const int k = isI ? lane : (lane < 16 ? lane - 10 : 0);
    real own = ci[0];
#pragma unroll
    for (int t = 1; t < 10; t++) own = (lane == t) ? ci[t] : own;
#pragma unroll
    for (int t = 0; t < 6; t++) own = (lane == 10 + t) ? fo[t] : own;
    real acc = own;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const real vI = S.chain_I[c][k], vf = S.chain_f[c][k];
      acc += isI ? vI : vf;
    }
    if (lane < 16) {
      real* dst = isI ? &S.Ic[bb][k] : &S.cfrc[bb][k];
      *dst = acc;
    }
  }
  GM_WAVE_SYNC();
}

// ============================================================ mass matrix rows + forces
__device__ __forceinline__ void ctrl_gains(const gm_model* __restrict__ m, const GmTopo* __restrict__ T, int d,
                                           real* kp, real* kd) {
  *kp = 0; *kd = 0;
  for (int f = 0; f < 3; f++) {
    if (d == m->dof_pris[f]) { *kp = (real)m->kp_gripper[0]; *kd = (real)m->kd_gripper[0]; }
    if (d == m->dof_rev[f]) { *kp = (real)m->kp_gripper[1]; *kd = (real)m->kd_gripper[1]; }
  }
  if (d == m->dof_palm) { *kp = (real)m->kp_gripper[2]; *kd = (real)m->kd_gripper[2]; }
  if (d == m->dof_base) { *kp = (real)m->kp_base[2]; *kd = (real)m->kd_base[2]; }
}

// lane per dof: H row entries (compact), bias/passive/actuator force
// CAL: the calibration variant (per-env timestep, tip load); the env-step kernel is CAL = false
template <int CL, bool CAL>
__device__ __forceinline__ void mass_and_forces(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T, int lane) {
  if (lane < T->nv) {
    const int d = lane;
    const int b = T->dof_body[d];
    const int c = T->dof_grp[d];
    const int p = T->dof_p[d];
    real add;
    if constexpr (CAL) {   // H~ diagonal for this env's timestep (same operations as the host fold)
      const real h = S.s.dt;
      add = T->dof_arm[d] + h * T->dof_dsum[d];
      add += h * h * T->dof_ksum[d];
    } else {
      add = T->dof_add[d];
    }
    real cd[6], F[6];
#pragma unroll
    for (int k = 0; k < 6; k++) cd[k] = S.cdof[d][k];
    inert_mul(F, S.Ic[b], cd);
    if (c == GM_GRP_BASE) {
      S.Hbb = dot6(cd, F) + add;
    } else {
      // object and chain rows share one loop (one pass of the wave instead of two
      // divergent ones): row p of the object block or of the chain's block
      const bool objd = c == GM_GRP_OBJECT;
      const int d0 = objd ? T->dof_obj : (c < 3) ? T->dof_f0[c] : T->dof_palm;
      real* Hrow = objd ? &S.Ho[TRI(p, 0)] : (c < 3) ? &S.Hf[c][TRI(p, 0)] : &S.Hp[TRI(p, 0)];
#pragma unroll
      for (int q = 0; q <= CL; q++) {
        int dq = objd ? d0 + q : (q == 0) ? T->dof_base : d0 + q - 1;
        dq = dq < SharedT<CL>::NV ? dq : SharedT<CL>::NV - 1;
        real v = dot6(S.cdof[dq], F);
        if (q == p) v += add;
        keep(v);
        if (q <= p) Hrow[q] = v;
      }
    }
    // forces: passive springs/damping, PD control (target_.next, base target), RNE bias
    const real bias = dot6(cd, S.cfrc[b]);
    const real qp = S.s.qpos[d], qv = S.s.qvel[d];
    real pas = 0;
    pas -= T->dof_stiff[d] * qp;
    pas -= T->dof_damp[d] * qv;
    const int tgt = T->dof_target[d];
    real act = 0;
    if (tgt != 0) {
      const real target = tgt == 1 ? S.s.next.x : tgt == 2 ? S.s.next.th : tgt == 3 ? S.s.next.z : S.s.base[2];
      act = -((qp - target) * T->dof_kp[d] + qv * T->dof_kd[d]);
    }
    real frc = pas + act - bias;
    if (CAL && S.s.tip_force != 0.0 && (c < 3 || c == GM_GRP_BASE)) {
      // calibration tip load: resolve_segment_forces -> apply_segment_force
      // (myfunctions.cpp:1642-1727) pulls each finger's tip link at its centre of mass
      // along the finger's rest bending direction; J^T F for the dofs above that link
#pragma unroll
      for (int f = 0; f < 3; f++) {
        if (c < 3 && f != c) continue;
        const int bt = m->body_tip[f];
        real R[9], ip[3], pc[3], wxp[3];
        body_R(S, bt, R);
        ld3(ip, m->body_ipos[bt]);
        mulmv3(pc, R, ip);
        pc[0] += S.xpos[bt][0]; pc[1] += S.xpos[bt][1]; pc[2] += S.xpos[bt][2];
        const real F[3] = {S.s.tip_force * m->tip_dir[f][0], S.s.tip_force * m->tip_dir[f][1],
                           S.s.tip_force * m->tip_dir[f][2]};
        cross3(wxp, cd, pc);
        const real col[3] = {cd[3] + wxp[0], cd[4] + wxp[1], cd[5] + wxp[2]};
        frc += dot3(col, F);
      }
    }
    S.frc[d] = frc;
  }
  GM_WAVE_SYNC();
}
GM_PHYSICS_END
using gmf::kinematics, gmf::crb_rne, gmf::mass_and_forces;
