// gm_euler.h -- mj_Euler's implicit joint damping, the arrow solve of physics stage 4
// (gm_integrate.h calls euler_damping, or euler_solve on the factor a DUO workgroup's helper
// wave formed with euler_factor, gm_kernels.hip duo_helper).
//
// MuJoCo 2.1.5's actuator order (gm_model::mujoco_actuators): the PD forces are explicit
// (mass_and_forces), the constraint solve runs on M + armature, and mj_Euler integrates
// qacc_e = (M + h D)^-1 (qfrc_smooth + qfrc_constraint) = qacc - (M + h D)^-1 (h D qacc)
// (M qacc = qfrc_smooth + qfrc_constraint at the solve's optimum).  The gripper's M + h D on
// the factor lanes (gm_arrow.h): each finger chain block leaf-first on its DPP row with the
// base as the single border column (row_newbcast pivots, as the Newton point with a one-wide
// border), the palm one pivot; the base pivot's two sums (Schur complement sum lb ub, forward
// sum lb y) are one segmented scan per DPP row plus the three row totals and the palm read
// back as scalars (row_totals), so the base solve is computed wave-uniformly.  The object has
// no damping and no coupling to the gripper in M: its rows take no correction.  qacc_e goes to
// S.xs (free after the solve); oracle/physics.c euler_damping restates it lane for lane.

// SharedT: reads Hf, Hp, Hbb, qacc, Mv, res_valid; writes xs.
#pragma once
#include "gm_arrow.h"

GM_PHYSICS_BEGIN
// The factor half: L (chain rows, scaled), lb (the base column, scaled), 1 / d on the pivot
// lanes, and the base pivot's Schur sum (returned, wave-uniform).  It reads only M's blocks
// (mass_and_forces) and the damping, so a DUO workgroup's helper wave runs it during the
// constraint solve (duo_helper) and hands it over in LDS; the one-wave kernel keeps it in
// registers.  The same operations either way.
template <int CL>
__device__ __forceinline__ real euler_factor(const SharedT<CL>& S, const GmTopo* __restrict__ T, real h, int lane,
                                             real (&L)[CL + 1], real& lb, real& invd) {
  const FactorLane fl = factor_lane<CL>(lane);
  const int rowf = fl.rowf, p = fl.p;
  const bool chainrow = fl.chainrow, palm = fl.palm;
  lb = 0.0;
#pragma unroll
  for (int j = 0; j <= CL; j++) L[j] = 0.0;
  if (chainrow) {
    const real* H = S.Hf[rowf];
    const int d = T->dof_f0[rowf] + p - 1;
    const real hd = h * T->dof_damp[d];
    {
      // the full symmetric row (M's upper part read from its lower triangle): the factor
      // then takes each pivot's column entry from the lane's own row
      real Hr[CL + 1];
#pragma unroll
      for (int j = 1; j <= CL; j++) Hr[j] = H[j <= p ? TRI(p, j) : TRI(j, p)];
      Hr[0] = Hr[1];
      keep_n<CL + 1>(Hr);
#pragma unroll
      for (int j = 1; j <= CL; j++) L[j] = Hr[j];
    }
#pragma unroll
    for (int j = 1; j <= CL; j++) L[j] = (j == p) ? L[j] + hd : L[j];
    lb = H[TRI(p, 0)];
  } else if (palm) {
    const int d = T->dof_palm;
    const real hd = h * T->dof_damp[d];
    L[1] = S.Hp[TRI(1, 1)] + hd;
    lb = S.Hp[TRI(1, 0)];
  }
  invd = 1.0;
  real ub = 0.0;
  if (lane < 48) {
#pragma unroll
    for (int k = CL; k >= 1; k--) {
      const real ihk = rcp_piv(row_bcast(L[k], k));
      real hk[CL + 1];
#pragma unroll
      for (int j = 1; j < k; j++) hk[j] = row_bcast(L[j], k);
      const real hkb = row_bcast(lb, k);
      const bool upd = p >= 1 && p < k, piv = p == k;
      const real a = L[k] * ihk;   // (the lane's own row holds the pivot column: full symmetric rows)
      const real aa = upd ? a : 0.0;
      ub = piv ? lb : ub;
#pragma unroll
      for (int j = 1; j < k; j++) L[j] = L[j] - hk[j] * aa;   // (pivot row scaled after the loop)
      lb = lb - hkb * aa;
      L[k] = upd ? a : L[k];
      invd = piv ? ihk : invd;
    }
#pragma unroll
    for (int j = 1; j < CL; j++) L[j] = (j < p) ? L[j] * invd : L[j];
    lb = lb * invd;
  } else if (palm) {
    const real ih = rcp_piv(L[1]);
    ub = lb;
    lb = lb * ih;
    invd = ih;
  }
  // the base pivot's Schur sum of lb ub over the chain rows and the palm
  const bool part = chainrow || palm;
  return row_totals(part ? lb * ub : 0.0);
}

// The solve half: qacc_e = qacc - (M + h D)^-1 (h D qacc [- r on a capped solve]) into S.xs.
template <int CL>
__device__ __forceinline__ void euler_solve(SharedT<CL>& S, const GmTopo* __restrict__ T, real h, int lane,
                                            const real (&L)[CL + 1], real lb, real invd, real sch) {
  const FactorLane fl = factor_lane<CL>(lane);
  const int rowf = fl.rowf, p = fl.p;
  const bool chainrow = fl.chainrow, palm = fl.palm;
  const bool res = S.res_valid != 0;   // a capped solve's residual in S.Mv (newton_solve)
  real y = 0.0;
  if (chainrow) {
    const int d = T->dof_f0[rowf] + p - 1;
    const real hd = h * T->dof_damp[d];
    y = hd * S.qacc[d];
    if (res) y = y + S.Mv[d];
  } else if (palm) {
    const int d = T->dof_palm;
    const real hd = h * T->dof_damp[d];
    y = hd * S.qacc[d];
    if (res) y = y + S.Mv[d];
  }
  // the base row (wave-uniform: one scalar dof)
  const int db = T->dof_base;
  const real hdb = h * T->dof_damp[db];
  const real bb = S.Hbb + hdb;
  const real yb0 = res ? hdb * S.qacc[db] + S.Mv[db] : hdb * S.qacc[db];
  if (lane < 48) y = chain_forward<CL>(y, L, p);   // forward over the chains, leaf first
  // the base pivot's forward sum of lb y, as the Schur sum (euler_factor)
  const bool part = chainrow || palm;
  const real fs = row_totals(part ? lb * y : 0.0);
  const real xb = (yb0 - fs) * rcp_piv(bb - sch);
  // back substitution: D^-1, the border column, then the chains root -> leaf
  y = y * invd;
  y = y - lb * xb;
  if (lane < 48) y = chain_backward<CL>(y, L, p);
  if (chainrow) {
    const int d = T->dof_f0[rowf] + p - 1;
    S.xs[d] = S.qacc[d] - y;
  } else if (palm) {
    S.xs[T->dof_palm] = S.qacc[T->dof_palm] - y;
  } else if (lane == 48) {
    S.xs[db] = S.qacc[db] - xb;
  } else if (lane >= GM_OBJ_LANE0 && lane < GM_OBJ_LANE0 + 6) {
    const int d = T->dof_obj + lane - GM_OBJ_LANE0;
    S.xs[d] = res ? S.qacc[d] - S.Mv[d] : S.qacc[d];
  }
  GM_WAVE_SYNC();
}

template <int CL>
__device__ __forceinline__ void euler_damping(SharedT<CL>& S, const GmTopo* __restrict__ T, real h, int lane) {
  real L[CL + 1], lb, invd;
  const real sch = euler_factor<CL>(S, T, h, lane, L, lb, invd);
  euler_solve<CL>(S, T, h, lane, L, lb, invd, sch);
}
GM_PHYSICS_END
using gmf::euler_factor;
