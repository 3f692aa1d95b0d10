// gm_newton.hip -- physics stage 3, the constraint solve of the env-step kernel (after the
// smooth dynamics, gm_dynamics.h, and the collider, gm_collide.h).
//
// The constraint problem is MuJoCo's (mj_makeConstraint / mj_makeImpedance with the
// mj_diagApprox regulariser, pyramidal cones: the rows, gm_rows.h), solved to its unique optimum
// by MuJoCo's Newton method (mj_solNewton: primal, in qacc space, exact line search, warm start
// from the previous substep's qacc).  Each iteration's Newton point -- the Hessian
// H~ + J_a^T D_a J_a assembled in spatial form, factored and solved on the DPP-row layout -- is
// gm_newton_point.h; this file holds the iteration around it.
// oracle/physics.c restates every function here operation for operation (the oracle's
// lane emulation), so device and oracle agree bit for bit from the same state.
// (The capped-solve residual with its lane-0 6x6 LDL^T -- the oracle's ldl6_solve -- and the
// force write-back stay in newton_solve's body: as functions of their own they change the
// encoding of four compares and selects, profiles/newton_stages_code_identity.txt.)

// SharedT: reads Hf / Hp / Ho / Hbb, frc, s.qacc_warm; writes qacc, xs, Ma, Mv, res_valid, con's
// forces, s.qacc_warm, s.newton_caps, work_nefc / work_newton and the union's dbg (and what
// gm_rows.h and gm_newton_point.h list).
#pragma once
#include "gm_rows.h"
#include "gm_newton_point.h"

GM_PHYSICS_BEGIN
// H~ v on the tree blocks, lane = dof (oracle smooth_matvec); v, out in LDS
template <int CL>
__device__ void smooth_matvec(SharedT<CL>& S, const GmTopo* __restrict__ T, const real* v, real* out, int lane) {
  if (lane < T->nv) {
    const int d = lane, c = T->dof_grp[d], p = T->dof_p[d];
    real acc;
    if (c >= 0 && c < 3) {
      const real* H = S.Hf[c];
      const int f0 = T->dof_f0[c];
      acc = H[TRI(p, 0)] * v[T->dof_base];
#pragma unroll
      for (int j = 1; j <= CL; j++) {
        const real hv = H[(j <= p) ? TRI(p, j) : TRI(j, p)];
        acc = acc + hv * v[f0 + j - 1];
      }
    } else if (c == GM_GRP_BASE) {
      acc = S.Hbb * v[T->dof_base];
#pragma unroll
      for (int f = 0; f < 3; f++)
#pragma unroll
        for (int q = 1; q <= CL; q++) acc = acc + S.Hf[f][TRI(q, 0)] * v[T->dof_f0[f] + q - 1];
      acc = acc + S.Hp[TRI(1, 0)] * v[T->dof_palm];
    } else if (c == GM_GRP_PALM) {
      acc = S.Hp[TRI(1, 0)] * v[T->dof_base] + S.Hp[TRI(1, 1)] * v[T->dof_palm];
    } else {
      acc = 0;
#pragma unroll
      for (int l = 0; l < 6; l++) {
        const real hv = S.Ho[(l <= p) ? TRI(p, l) : TRI(l, p)];
        acc = acc + hv * v[T->dof_obj + l];
      }
    }
    out[d] = acc;
  }
  GM_WAVE_SYNC();
}

// The exact line search of one iteration along d = x - q from the rows' J q - aref (jq / jql)
// and J d (dj / djl) and the smooth part's slope g0 = d . (H~ q - f) and curvature h0 = d . H~ d:
// the step alpha and whether the search ran GM_NEWTON_MAXLS evaluations without settling
// (wave-uniform: every exit test is); nls counts the evaluations.
struct LineSearch { real alpha; bool capped; };
__device__ __forceinline__ LineSearch line_search(int lane, int ncon, int nl, const RowsT& R, const real* jq, real jql,
                                                  const real* dj, real djl, real g0, real h0, int& nls) {
  const bool clane = lane < ncon;
  real alpha = 1.0, lo = 0.0, hi = 0.0;
  bool hi_set = false, newton = false, have_prev = false;
  unsigned prev = 0;
  int ls = 0;
  for (; ls < GM_NEWTON_MAXLS; ls++) {
    nls++;
    unsigned pat = 0;
    real tg[4], th[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const real j = jq[e] + alpha * dj[e];
      const bool a = clane && j < 0;
      pat |= (unsigned)a << e;
      tg[e] = a ? (R.cD * j) * dj[e] : 0.0;
      th[e] = a ? (R.cD * dj[e]) * dj[e] : 0.0;
    }
    const real jl = jql + alpha * djl;
    const real tgl = (R.lD * jl) * djl, thl = (R.lD * djl) * djl;   // lock rows: always active
    const bool same_piece = have_prev && __ballot(pat != prev) == 0ull;
    if (newton && same_piece) break;
    const real g = (g0 + alpha * h0) + row_sum(lane, ncon, nl, tg, tgl);
    const real hh = h0 + row_sum(lane, ncon, nl, th, thl);
    if (g == 0.0) break;
    if (g < 0) lo = alpha; else { hi = alpha; hi_set = true; }
    if (!(hh > 0)) break;
    real an = alpha - div_n(g, hh);
    newton = true;
    if (!(an > lo) || (hi_set && !(an < hi))) { an = hi_set ? 0.5 * (lo + hi) : 2.0 * alpha; newton = false; }
    prev = pat;
    have_prev = true;
    alpha = an;
  }
  return {alpha, ls == GM_NEWTON_MAXLS};
}

// mj_solNewton restated (oracle newton_solve): warm start, Newton point on the active
// pattern, accept when the pattern at x is unchanged (x is then the exact optimum), else
// an exact line search along x - q; contact forces and the warm start at the end.
template <int CL, bool CAL, bool DUO = false>
__device__ __forceinline__ void newton_solve(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T, int lane,
                             bool prof) {
  unsigned long long t0 = prof ? clock64() : 0;
  RowsT R;
  real jq[4], jql;
  bool obj_only;
  constraint_setup<CL, CAL, DUO>(S, m, T, lane, R, jq, jql, obj_only, prof);
#ifndef GM_NO_DECOUPLED_POINT
  // obj_only: every contact slot below ncon is an object-ground contact, so no slot belongs to a
  // gripper-object or gripper-ground pair: newton_point's any_o and any_g are both false
  const bool decoupled = __builtin_amdgcn_readfirstlane((int)obj_only) != 0;
#endif
  PH(11);
  const int ncon = S.ncon, nl = S.nl, nv = T->nv;
  const bool clane = lane < ncon;
  if (lane < nv) S.qacc[lane] = S.s.qacc_warm[lane];
  GM_WAVE_SYNC();
  PH(12);
  int it = 0, nls = 0;
  bool capped = true;   // no Newton point accepted within GM_NEWTON_MAXIT iterations
  bool ls_cap = false;  // a line search ran GM_NEWTON_MAXLS evaluations without settling
  const int maxit = (m->newton_maxit > 0 && m->newton_maxit < GM_NEWTON_MAXIT) ? m->newton_maxit : GM_NEWTON_MAXIT;
  for (it = 0; it < maxit; it++) {
    bool act[4];
#pragma unroll
    for (int e = 0; e < 4; e++) act[e] = clane && jq[e] < 0;
    PH(13);
#ifndef GM_NO_DECOUPLED_POINT
    // the first point of a solve whose contacts are all the object's with the ground
    // (wave-uniform; the same x, gm_newton_point.h).  Counted per env beside the CU id.
    if (it == 0 && decoupled) {
      newton_point_decoupled<CL>(S, m, T, fresh_lane(), R, act, prof);
      if (prof && lane == 0) S.tph[27] += 1ull << 32;
    } else
#endif
    newton_point<CL>(S, m, T, fresh_lane(), R, act, prof);
    if (prof) t0 = clock64();
    real jx[4], jxl;
    rows_jar<CL>(S, m, T, obj_only, S.xs, lane, R, jx, jxl);
    bool differ = false;
#pragma unroll
    for (int e = 0; e < 4; e++) differ = differ || (clane && ((jx[e] < 0) != act[e]));
    if (__builtin_expect(__ballot(differ) == 0ull, 1)) {
      if (lane < nv) S.qacc[lane] = S.xs[lane];
#pragma unroll
      for (int e = 0; e < 4; e++) jq[e] = jx[e];
      jql = jxl;
      it++;
      capped = false;
      break;
    }
    // exact line search along d = x - q (d overwrites x); H~ q formed when first needed
    // (only iteration 0 reaches here with q unchanged: the oracle does the same)
    if (it == 0) smooth_matvec<CL>(S, T, S.qacc, S.Ma, lane);
    if (lane < nv) S.xs[lane] = S.xs[lane] - S.qacc[lane];
    GM_WAVE_SYNC();
    smooth_matvec<CL>(S, T, S.xs, S.Mv, lane);
    const real xl = S.xs[lane];   // (lanes past nv read the next LDS vector; selected away)
    const real dd = lane < nv ? xl : 0.0;
    const real g0 = wave_sum(lane < nv ? dd * (S.Ma[lane] - S.frc[lane]) : 0.0);
    const real h0 = wave_sum(lane < nv ? dd * S.Mv[lane] : 0.0);
    real dj[4];
#pragma unroll
    for (int e = 0; e < 4; e++) dj[e] = jx[e] - jq[e];
    const real djl = jxl - jql;
    const LineSearch ls = line_search(lane, ncon, nl, R, jq, jql, dj, djl, g0, h0, nls);
    ls_cap = ls_cap || ls.capped;
    const real alpha = ls.alpha;
    if (lane < nv) {
      S.qacc[lane] = S.qacc[lane] + alpha * S.xs[lane];
      S.Ma[lane] = S.Ma[lane] + alpha * S.Mv[lane];
    }
#pragma unroll
    for (int e = 0; e < 4; e++) jq[e] = jq[e] + alpha * dj[e];
    jql = jql + alpha * djl;
    GM_WAVE_SYNC();
  }
  PH(13);
  // A capped solve (wave-uniform, rare: none in the benchmarks): qacc is no optimum, so what
  // mj_Euler integrates, qfrc_smooth + J^T efc, differs from H~ qacc by the residual
  // r = H~ qacc - qfrc_smooth - J^T efc.  J^T efc is the Newton right-hand side with the row
  // forces in place of D aref (efc = -D jar on the active rows: caref := -jq); H~ qacc is Ma,
  // which the line search of every capped iteration kept up to date.  r goes to S.Mv for
  // euler_damping; the object rows (decoupled from the gripper in M, undamped) take their
  // correction Moo^-1 r right here on lane 0 (oracle/physics.c ldl6_solve, same order).
  if (lane == 0) S.res_valid = capped ? 1 : 0;
  if (capped) {
    RowsT Rc = R;
    bool ac[4];
#pragma unroll
    for (int e = 0; e < 4; e++) { Rc.caref[e] = -jq[e]; ac[e] = clane && jq[e] < 0; }
    Rc.laref = -jql;
    newton_point<CL, true>(S, m, T, fresh_lane(), Rc, ac, false);
    if (lane < nv) S.Mv[lane] = S.Ma[lane] - S.xs[lane];
    GM_WAVE_SYNC();
    if (lane == 0) {
      real A[6][6], x[6];
      for (int k = 0; k < 6; k++)
        for (int l = 0; l <= k; l++) A[k][l] = S.Ho[TRI(k, l)];
      for (int k = 0; k < 6; k++) x[k] = S.Mv[T->dof_obj + k];
      for (int k = 5; k >= 0; k--) {
        const real ik = 1.0 / A[k][k];
        real col[6];
        for (int i = 0; i < k; i++) col[i] = A[k][i];
        for (int i = 0; i < k; i++) {
          const real a = col[i] * ik;
          for (int j = 0; j <= i; j++) A[i][j] = A[i][j] - a * col[j];
          A[k][i] = a;
        }
      }
      for (int k = 5; k >= 0; k--)
        for (int i = 0; i < k; i++) x[i] = x[i] - A[k][i] * x[k];
      for (int k = 0; k < 6; k++) x[k] = x[k] / A[k][k];
      for (int k = 0; k < 6; k++)
        for (int i = 0; i < k; i++) x[k] = x[k] - A[k][i] * x[i];
      for (int k = 0; k < 6; k++) S.Mv[T->dof_obj + k] = x[k];
    }
    GM_WAVE_SYNC();
  }
  // constraint forces at the solution and the contact-frame forces (mj_contactForce)
  real fe[4];
#pragma unroll
  for (int e = 0; e < 4; e++) fe[e] = (clane && jq[e] < 0) ? -(R.cD * jq[e]) : 0.0;
  if (clane) {
    real* C = S.con[lane];
    const real mu = C[10];
    C[11] = ((fe[0] + fe[1]) + fe[2]) + fe[3];
    C[12] = mu * (fe[0] - fe[1]);
    C[13] = mu * (fe[2] - fe[3]);
#pragma unroll
    for (int e = 0; e < 4; e++) S.dbg.efc[nl + 4 * lane + e] = fe[e];
  }
  if (lane < nl) S.dbg.efc[lane] = -(R.lD * jql);
  if (lane < nv) S.s.qacc_warm[lane] = S.qacc[lane];
  if (lane == 0) {
    S.work_nefc += nl + 4 * ncon;
    S.work_newton += it;
    if (capped || ls_cap) S.s.newton_caps += 1;   // (the oracle counts the same, physics.c newton_solve)
    if (prof) { S.tph[28] += nl + 4 * ncon; S.tph[30] += it; S.tph[31] += nls; }
  }
  GM_WAVE_SYNC();
}
GM_PHYSICS_END
using gmf::newton_solve;
