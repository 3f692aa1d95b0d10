// gm_newton_point.h -- the Newton point of physics stage 3: x = H^-1 rhs for one active pattern
// of the constraint rows (gm_rows.h), called by the Newton solve (gm_newton.hip).
//
// The Hessian H~ + J_a^T D_a J_a is assembled in spatial form -- per contact the 3x3
// Q = sum_e D_e u_e u_e^T of its active pyramid edges, per body the 6x6 K = S Q S^T summed over
// the body's contacts, suffix-scanned along each finger chain like composite inertias -- so its
// cost follows the bodies, not the constraint rows, and no per-row Jacobian or Delassus matrix is
// ever formed.  It is factored on the arrow layout of gm_arrow.h: each finger chain's block on
// its 16-lane row with the border [base, object 0..5] as extra columns (leaf-first LDL^T,
// row_newbcast pivots), Schur complements into the border, a 7x7 border LDL^T on row 3.
// Lane roles: contact lanes build Q / F; scan lanes (GmTopo lane_body) sum their body's contacts
// and suffix-scan along the chains; factor lanes -- finger chain rows on 16 f + p (p = 1..CL),
// border rows [base, obj0..5] on 48..54, the palm on 56 -- assemble H and rhs, factor, solve.
// oracle/physics.c newton_assemble and newton_factor_solve restate it operation for operation
// (the oracle's lane emulation).  The stages that are functions here (newton_contact_qf,
// newton_ground_composites, newton_schur, newton_border_factor, newton_backsolve) and the
// shared pieces (composite_add, object_columns, gm_arrow.h's) are the ones that leave every
// kernel's vector code as it was; the rest of the assembly and the chain factor stay in
// newton_point's body (profiles/newton_stages_code_identity.txt has the trials).
// newton_point_decoupled, at the end of the file, is the same point for solves whose contacts
// are all the object's with the ground: two independent blocks factored side by side.

// SharedT: reads con, cbody, pair_off / pair_cnt, cdof, Hf / Hp / Ho / Hbb, frc; writes go, xs and
// the union's nw.QF, st, fs.
#pragma once
#include "gm_rows.h"
#include "gm_arrow.h"

GM_PHYSICS_BEGIN
// K = S Q S^T, S = [skew(p); I]: [A xx yy zz xy xz yz | B row-major | Q xx yy zz xy xz yz]
__device__ __forceinline__ void spatial_K(const real* Q, const real* p, real* K) {
  const real Qm[3][3] = {{Q[0], Q[3], Q[4]}, {Q[3], Q[1], Q[5]}, {Q[4], Q[5], Q[2]}};
  real Bm[3][3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    real c[3];
    cross3(c, p, Qm[j]);
    Bm[0][j] = c[0]; Bm[1][j] = c[1]; Bm[2][j] = c[2];
  }
  real Am[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++) cross3(Am[i], p, Bm[i]);
  K[0] = Am[0][0]; K[1] = Am[1][1]; K[2] = Am[2][2]; K[3] = Am[0][1]; K[4] = Am[0][2]; K[5] = Am[1][2];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) K[6 + 3 * i + j] = Bm[i][j];
#pragma unroll
  for (int k = 0; k < 6; k++) K[15 + k] = Q[k];
}
__device__ __forceinline__ void symK_mul(const real* K, const real* v, real* y) {
  const real *A = K, *B = K + 6, *Q = K + 15;
  const real w0 = v[0], w1 = v[1], w2 = v[2], l0 = v[3], l1 = v[4], l2 = v[5];
  y[0] = A[0] * w0 + A[3] * w1 + A[4] * w2 + B[0] * l0 + B[1] * l1 + B[2] * l2;
  y[1] = A[3] * w0 + A[1] * w1 + A[5] * w2 + B[3] * l0 + B[4] * l1 + B[5] * l2;
  y[2] = A[4] * w0 + A[5] * w1 + A[2] * w2 + B[6] * l0 + B[7] * l1 + B[8] * l2;
  y[3] = B[0] * w0 + B[3] * w1 + B[6] * w2 + Q[0] * l0 + Q[3] * l1 + Q[4] * l2;
  y[4] = B[1] * w0 + B[4] * w1 + B[7] * w2 + Q[3] * l0 + Q[1] * l1 + Q[5] * l2;
  y[5] = B[2] * w0 + B[5] * w1 + B[8] * w2 + Q[4] * l0 + Q[5] * l1 + Q[2] * l2;
}

// one contact's spatial composite K = S Q S^T and force [p x F; F] from its Q / F (qf[0..6),
// qf[6..9)) at the contact position
__device__ __forceinline__ void contact_composite(const real* qf, const real* pos, real* Kc, real* Fs) {
  spatial_K(qf, pos, Kc);
  cross3(Fs, pos, qf + 6);
  Fs[3] = qf[6]; Fs[4] = qf[7]; Fs[5] = qf[8];
}
// contact c's composite added to body b's K / F (the force's sign by which of the contact's
// bodies b is)
template <int CL>
__device__ __forceinline__ void composite_add(const SharedT<CL>& S, int c, int b, real* K, real* F) {
  const real* qf = S.nw.QF[c];
  const real pos[3] = {S.con[c][1], S.con[c][2], S.con[c][3]};
  const real sg = (S.cbody[c][1] == b) ? 1.0 : -1.0;
  real Kc[21], Fs[6];
  contact_composite(qf, pos, Kc, Fs);
#pragma unroll
  for (int k = 0; k < 21; k++) K[k] += Kc[k];
#pragma unroll
  for (int k = 0; k < 6; k++) F[k] += sg * Fs[k];
}
// the object's six motion subspaces (wave-uniform reads), in two batches of three loads:
// col(l, cdof of object dof l) for l = 0..5
template <int CL, class Col>
__device__ __forceinline__ void object_columns(const SharedT<CL>& S, const GmTopo* T, Col col) {
#pragma unroll
  for (int k0 = 0; k0 < 6; k0 += 3) {
    real co[18];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int t = 0; t < 6; t++) co[6 * k + t] = S.cdof[T->dof_obj + k0 + k][t];
    keep_n<18>(co);
#pragma unroll
    for (int k = 0; k < 3; k++) col(k0 + k, co + 6 * k);
  }
}
// ---- contact lanes: Q = sum_e D u u^T and F = sum_e D aref u over the active edges, kept in
// the lane's registers and written to S.nw.QF
template <int CL>
__device__ __forceinline__ void newton_contact_qf(SharedT<CL>& S, int lane, int ncon, const RowsT& R, const bool* act,
                                                  real (&Q)[6], real (&F)[3]) {
#pragma unroll
  for (int k = 0; k < 6; k++) Q[k] = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) F[k] = 0;
  if (lane < ncon) {
    const real* C = S.con[lane];
    real t2[3];
    cross3(t2, C + 4, C + 7);
#pragma unroll
    for (int ed = 0; ed < 4; ed++) {
      real u[3];
      edge_dir(C, t2, ed, u);
      const real w = act[ed] ? R.cD : 0.0;
      const real du[3] = {w * u[0], w * u[1], w * u[2]};
      Q[0] += du[0] * u[0]; Q[1] += du[1] * u[1]; Q[2] += du[2] * u[2];
      Q[3] += du[0] * u[1]; Q[4] += du[0] * u[2]; Q[5] += du[1] * u[2];
      const real g = w * R.caref[ed];
      F[0] += g * u[0]; F[1] += g * u[1]; F[2] += g * u[2];
    }
    real* qf = S.nw.QF[lane];
#pragma unroll
    for (int k = 0; k < 6; k++) qf[k] = Q[k];
    qf[6] = F[0]; qf[7] = F[1]; qf[8] = F[2];
  }
  GM_WAVE_SYNC();
}

// ---- the object's ground contacts into S.go (its other contacts reach it through the base
// composite).  Each contact lane of the object-ground pair forms its own K and F from the
// Q / F it still holds and hands the 27 values over in the chain-root stage (dead until
// the roots are written by newton_body_composites; QF stays as it is for the ground pass);
// lane k < 27 then sums entry k over the pair's slots in order, starting from 0: the serial
// loop's additions, operand for operand (sg = +-1 makes sg * Fs exact, fused or not).  Eight
// contacts fill the stage, so a longer pair takes further rounds (a plane pair makes at
// most four: one round).
template <int CL>
__device__ __forceinline__ void newton_ground_composites(SharedT<CL>& S, const GmTopo* T, int lane, int ncon,
                                                         const real (&Q)[6], const real (&F)[3]) {
  static_assert(sizeof(S.st.root) >= sizeof(real) * 8 * 27, "ground composites: eight contacts per round in the chain-root stage");
  real (*gs)[27] = reinterpret_cast<real (*)[27]>(&S.st.root[0][0]);
  const int pr = T->pair_gobj;
  int c0 = 0, c1 = 0;
  if (pr >= 0) {
    c0 = __builtin_amdgcn_readfirstlane((int)S.pair_off[pr]);
    c1 = c0 + __builtin_amdgcn_readfirstlane((int)S.pair_cnt[pr]);
    if (c1 > ncon) c1 = ncon;
  }
  real gacc = 0;
  for (int r0 = c0; r0 < c1; r0 += 8) {
    if (r0 > c0) GM_WAVE_SYNC();   // (the round before is summed)
    if (lane >= r0 && lane < r0 + 8 && lane < c1) {
      const real qf[9] = {Q[0], Q[1], Q[2], Q[3], Q[4], Q[5], F[0], F[1], F[2]};
      const real pos[3] = {S.con[lane][1], S.con[lane][2], S.con[lane][3]};
      const real sg = (S.cbody[lane][1] == T->body_obj) ? 1.0 : -1.0;
      real Kc[21], Fs[6];
      contact_composite(qf, pos, Kc, Fs);
      real* g = gs[lane - r0];
#pragma unroll
      for (int k = 0; k < 21; k++) g[k] = Kc[k];
#pragma unroll
      for (int k = 0; k < 6; k++) g[21 + k] = sg * Fs[k];
    }
    GM_WAVE_SYNC();
    if (lane < 27) {
      real v[8];   // (all eight slots read in one batch; those past the pair are selected away)
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = gs[j][lane];
      keep_n<8>(v);
#pragma unroll
      for (int j = 0; j < 8; j++) gacc = (r0 + j < c1) ? gacc + v[j] : gacc;
    }
  }
  if (lane < 27) S.go[lane] = gacc;
}

// ---- Schur complements of the chain and palm pivots into the border (S.fs.bbx): one lane per
// border entry (i, j), elimination order
template <int CL>
__device__ __forceinline__ void newton_schur(SharedT<CL>& S, int lane) {
  if (lane < 28) {
    int i = 0;
#pragma unroll
    for (int t = 1; t < 7; t++) i += (lane >= t * (t + 1) / 2) ? 1 : 0;
    const int j = lane - i * (i + 1) / 2;
    real acc[3];
    border_transfer_sums<CL>(S, i, [&](int f, int k1) { return S.fs.lbub[f][k1][7 + j]; }, acc);
    real v = S.fs.bbx[lane];
    v = (((v - acc[0]) - acc[1]) - acc[2]) - S.fs.plb[i] * S.fs.plb[7 + j];
    S.fs.bbx[lane] = v;
  }
}

// ---- border LDL^T on row 3 (lanes 48 + k, pivots 6 .. 0) from the Schur complements: L in hb
// (scaled), 1 / d in invd
template <int CL>
__device__ __forceinline__ void newton_border_factor(SharedT<CL>& S, int lane, real (&hb)[7], real& invd) {
  const int bi = lane - 48;
  const bool border = lane >= 48 && lane < 55;
  if (border) {
#pragma unroll
    for (int j = 0; j < 7; j++)
      if (j <= bi) hb[j] = S.fs.bbx[bi * (bi + 1) / 2 + j];
    // border LDL^T: pivots 6 .. 0 (row 3 lanes 48 + k)
#pragma unroll
    for (int k = 6; k >= 0; k--) {
      const real ihk = rcp_piv(row_bcast(hb[k], k));
      real bk[7];
#pragma unroll
      for (int j = 0; j < k; j++) bk[j] = row_bcast(hb[j], k);
      const bool upd = bi < k, piv = bi == k;
      real Bik = 0.0;
#pragma unroll
      for (int j = 0; j < k; j++) Bik = (bi == j) ? bk[j] : Bik;
      const real a = Bik * ihk;
      const real aa = upd ? a : 0.0;
#pragma unroll
      for (int j = 0; j < k; j++) hb[j] = hb[j] - bk[j] * aa;   // (pivot row scaled after the loop)
      hb[k] = upd ? a : hb[k];
      invd = piv ? ihk : invd;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) hb[j] = (j < bi) ? hb[j] * invd : hb[j];
  }
}

// ---- solve (oracle newton_factor_solve, second half): forward (chains leaf first, border
// sums, border), D, backward; x goes to S.xs
template <int CL>
__device__ __forceinline__ void newton_backsolve(SharedT<CL>& S, const GmTopo* T, int lane,
                                                 const real (&h)[CL + 1], const real (&hb)[7], real rhs, real invd) {
  const int rowf = lane >> 4, p = lane & 15, bi = lane - 48;
  const bool border = (lane >= 48 && lane < 55);
  real y = rhs;
  if (lane < 48) {
    y = chain_forward<CL>(y, h, p);
    if ((rowf < 3 && p >= 1 && p <= CL)) S.fs.ych[rowf][p - 1] = y;
  } else if (lane == GM_LANE_PALM_F) {
    S.fs.ypalm = y;
  }
  GM_WAVE_SYNC();
  if (border) {
    real acc[3];
    border_transfer_sums<CL>(S, bi, [&](int f, int k1) { return S.fs.ych[f][k1]; }, acc);
    y = (((y - acc[0]) - acc[1]) - acc[2]) - S.fs.plb[bi] * S.fs.ypalm;
#pragma unroll
    for (int k = 6; k >= 0; k--) {
      const real yk = row_bcast(y, k);
      const real Lc = (bi < k) ? hb[k] : 0.0;
      y = y - Lc * yk;
    }
  }
  y = y * invd;
  if (border) {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const real xj = row_bcast(y, j);
      const real Lr = (j < bi) ? hb[j] : 0.0;
      y = y - Lr * xj;
    }
  }
  // the border solution to every lane (row 3 lanes 48..54)
  real xb[7];
#pragma unroll
  for (int t = 0; t < 7; t++) xb[t] = readlane_real(y, 48 + t);
  if (lane < 48) {
#pragma unroll
    for (int t = 0; t < 7; t++) y = y - hb[t] * xb[t];
    y = chain_backward<CL>(y, h, p);
    if ((rowf < 3 && p >= 1 && p <= CL)) S.xs[T->dof_f0[rowf] + p - 1] = y;
  } else if (lane == GM_LANE_PALM_F) {
#pragma unroll
    for (int t = 0; t < 7; t++) y = y - hb[t] * xb[t];
    S.xs[T->dof_palm] = y;
  } else if (border) {
    S.xs[bi == 0 ? T->dof_base : T->dof_obj + bi - 1] = y;
  }
  GM_WAVE_SYNC();
}

// The Newton point x = H^-1 rhs for the active pattern (oracle newton_assemble +
// newton_factor_solve); x goes to S.xs.
// RHS_ONLY: stop after the assembly and leave the right-hand side f + J_a^T (D aref)_a in S.xs
// (the capped-solve residual of newton_solve calls it with D aref replaced by the row forces,
// so S.xs = qfrc_smooth + J^T efc)
// (The scan-lane composites, the H rows, the cold ground pass, the lock rows and the chain
// factor stay in this body: moved into functions of their own they compile to different vector
// code, profiles/newton_stages_code_identity.txt.)
template <int CL, bool RHS_ONLY = false>
__device__ void newton_point(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T, int lane,
                             const RowsT& R, const bool* act, bool prof) {
  unsigned long long t0 = prof ? clock64() : 0;
  const int ncon = S.ncon, nl = S.nl;
  real Q[6], F[3];
  newton_contact_qf<CL>(S, lane, ncon, R, act, Q, F);
  newton_ground_composites<CL>(S, T, lane, ncon, Q, F);
  // ---- scan lanes: the body's contacts with the object.  Contacts of gripper bodies with
  // the ground (rare) are added in a second pass below, so the common path keeps one
  // 27-value composite per lane in registers instead of two.
  const int b = T->lane_body[lane];
  real Ko[21], Fo[6];
#pragma unroll
  for (int k = 0; k < 21; k++) Ko[k] = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) Fo[k] = 0;
  bool have_g = false;
  // the lane's (up to two) object pairs' contacts, in pair order, as one loop (one set of
  // accumulator phis instead of one per pair)
  int cs[2] = {0, 0}, ns[2] = {0, 0};
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const int pr = T->lane_opair[lane][s];
    const int pg = T->lane_gpair[lane][s];
    if (pg >= 0 && S.pair_cnt[pg] > 0 && S.pair_off[pg] < ncon) have_g = true;
    if (pr >= 0) {
      const int c0 = S.pair_off[pr];
      int c1 = c0 + S.pair_cnt[pr];
      if (c1 > ncon) c1 = ncon;
      cs[s] = c0;
      ns[s] = c1 > c0 ? c1 - c0 : 0;
    }
  }
  const bool have_o = ns[0] + ns[1] > 0;
  {
    for (int t = 0; t < ns[0] + ns[1]; t++) {
      const int c = t < ns[0] ? cs[0] + t : cs[1] + (t - ns[0]);
      composite_add<CL>(S, c, b, Ko, Fo);
    }
  }
  const bool any_g = __ballot(have_g) != 0ull;
  // no gripper body touches the object (wave-uniform): the gripper rows' composites are
  // zero and their Hessian entries are H~'s own
  const bool any_o = __ballot(have_o) != 0ull;
  PH(3);
  // ---- suffix sums along the chains (composite, like Ic)
  if (any_o) {
#pragma unroll
    for (int off = 1; off < CL; off <<= 1) {
#pragma unroll
      for (int k = 0; k < 21; k++) Ko[k] += row_shl(Ko[k], off);
#pragma unroll
      for (int k = 0; k < 6; k++) Fo[k] += row_shl(Fo[k], off);
    }
  }
  // ---- chain roots (fingers at position 1, the palm) to the stage (which sits after the
  // per-contact Q / F in the union: the ground pass below still reads them)
  {
    const int root = (lane == 1) ? 0 : (lane == 17) ? 1 : (lane == 33) ? 2 : (lane == 49) ? 3 : -1;
    if (root >= 0) {
      real* st = S.st.root[root];
#pragma unroll
      for (int k = 0; k < 21; k++) st[k] = Ko[k];
#pragma unroll
      for (int k = 0; k < 6; k++) st[42 + k] = Fo[k];
    }
  }
  GM_WAVE_SYNC();
  // ---- base composites (the four roots in order) and the object's totals
  if (lane < 27) {
    const int k = lane < 21 ? lane : 42 + lane - 21;
    real acc = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) acc += S.st.root[c][k];
    S.st.comp[k] = acc;
  }
  GM_WAVE_SYNC();
  if (lane < 27) {
    // Koo = KBo + Kgo (21), Fobj = Fgo - FBo (6)
    S.st.oo[lane] = (lane < 21) ? S.st.comp[lane] + S.go[lane] : S.go[lane] - S.st.comp[42 + lane - 21];
  }
  GM_WAVE_SYNC();
  PH(4);
  // ---- H and rhs on the factor lanes
  real h[CL + 1], hb[7], rhs = 0;
#pragma unroll
  for (int j = 0; j <= CL; j++) h[j] = 0;
#pragma unroll
  for (int k = 0; k < 7; k++) hb[k] = 0;
  const int rowf = lane >> 4, p = lane & 15;
  const real* cdb = S.cdof[T->dof_base];
  if (rowf < 3 && p >= 1 && p <= CL) {
    const int d = T->dof_f0[rowf] + p - 1;
    const real* H = S.Hf[rowf];
    if (any_o) {
      real cd[6], y[6], Hr[CL + 1];
#pragma unroll
      for (int k = 0; k < 6; k++) cd[k] = S.cdof[d][k];
#pragma unroll
      for (int j = 0; j <= CL; j++) Hr[j] = H[TRI(p, j)];   // (the row, in range for every p)
      keep_n<CL + 1>(Hr);
      symK_mul(Ko, cd, y);
      // (all CL entries computed and kept for j <= p; the motion subspace of chain position
      // j is lane j's cd, taken by row_newbcast instead of an LDS round trip per entry)
#pragma unroll
      for (int j = 1; j <= CL; j++) {
        real cj[6];
#pragma unroll
        for (int k = 0; k < 6; k++) cj[k] = row_bcast(cd[k], j);
        const real v = Hr[j] + dot6(cj, y);
        keep(v);
        h[j] = (j <= p) ? v : h[j];
      }
      hb[0] = Hr[0] + dot6(cdb, y);
      // the object's six motion subspaces (wave-uniform reads), in two batches of three
      object_columns<CL>(S, T, [&](int l, const real* co) { hb[1 + l] = -dot6(co, y); });
      rhs = S.frc[d] + dot6(cd, Fo);
    } else {
      real Hr[CL + 1];
#pragma unroll
      for (int j = 0; j <= CL; j++) Hr[j] = H[TRI(p, j)];
      keep_n<CL + 1>(Hr);
#pragma unroll
      for (int j = 1; j <= CL; j++) h[j] = (j <= p) ? Hr[j] : h[j];
      hb[0] = Hr[0];
      rhs = S.frc[d];
    }
  } else if (lane == GM_LANE_PALM_F && !any_o) {
    h[1] = S.Hp[TRI(1, 1)];
    hb[0] = S.Hp[TRI(1, 0)];
    rhs = S.frc[T->dof_palm];
  } else if (lane == GM_LANE_PALM_F) {
    const int d = T->dof_palm;
    const real* st = S.st.root[3];
    real K0[27], y[6];   // the palm root's composite (21) then its cdof (6), one batch
#pragma unroll
    for (int k = 0; k < 21; k++) K0[k] = st[k];
#pragma unroll
    for (int k = 0; k < 6; k++) K0[21 + k] = S.cdof[d][k];
    keep_n<27>(K0);
    const real* cd = K0 + 21;
    symK_mul(K0, cd, y);
    h[1] = S.Hp[TRI(1, 1)] + dot6(cd, y);
    hb[0] = S.Hp[TRI(1, 0)] + dot6(cdb, y);
    object_columns<CL>(S, T, [&](int l, const real* co) { hb[1 + l] = -dot6(co, y); });
    rhs = S.frc[d] + dot6(cd, st + 42);
  } else if (lane >= 48 && lane < 55) {
    const int i = lane - 48;
    const real* cp = S.st.comp;
    real yob[6] = {0, 0, 0, 0, 0, 0};
    if (any_o) {
      real KBo[21];
#pragma unroll
      for (int k = 0; k < 21; k++) KBo[k] = cp[k];
      keep_n<21>(KBo);
      symK_mul(KBo, cdb, yob);
    }
    if (i == 0) {
      hb[0] = any_o ? S.Hbb + dot6(cdb, yob) : S.Hbb;
      rhs = any_o ? S.frc[T->dof_base] + dot6(cdb, cp + 42) : S.frc[T->dof_base];
    } else {
      const int k = i - 1;
      real KC[27], yk[6];   // Koo (21) then the row's cdof (6), loaded in one batch
#pragma unroll
      for (int t = 0; t < 21; t++) KC[t] = S.st.oo[t];
#pragma unroll
      for (int t = 0; t < 6; t++) KC[21 + t] = S.cdof[T->dof_obj + k][t];
      keep_n<27>(KC);
      const real* cok = KC + 21;
      symK_mul(KC, cok, yk);
      hb[0] = -dot6(cok, yob);
      object_columns<CL>(S, T, [&](int l, const real* co) {
        const real v = S.Ho[TRI(k, l)] + dot6(co, yk);
        keep(v);
        hb[1 + l] = (l <= k) ? v : hb[1 + l];
      });
      rhs = S.frc[T->dof_obj + k] + dot6(cok, S.st.oo + 21);
    }
  }
  // ---- contacts of gripper bodies with the ground (wave-uniform, rare): their composite
  // Kg is added to the chain rows' and the base's entries (the object rows do not see it)
  if (__builtin_expect(any_g, 0)) {   // cold: keep it out of the hot code's cache lines
    real Kg[21], Fg[6];
#pragma unroll
    for (int k = 0; k < 21; k++) Kg[k] = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) Fg[k] = 0;
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const int pr = T->lane_gpair[lane][s];
      if (pr < 0) continue;
      const int c0 = S.pair_off[pr];
      int c1 = c0 + S.pair_cnt[pr];
      if (c1 > ncon) c1 = ncon;
      for (int c = c0; c < c1; c++) {
        composite_add<CL>(S, c, b, Kg, Fg);
      }
    }
#pragma unroll
    for (int off = 1; off < CL; off <<= 1) {
#pragma unroll
      for (int k = 0; k < 21; k++) Kg[k] += row_shl(Kg[k], off);
#pragma unroll
      for (int k = 0; k < 6; k++) Fg[k] += row_shl(Fg[k], off);
    }
    const int root = (lane == 1) ? 0 : (lane == 17) ? 1 : (lane == 33) ? 2 : (lane == 49) ? 3 : -1;
    if (root >= 0) {
      real* st = S.st.root[root];
#pragma unroll
      for (int k = 0; k < 21; k++) st[21 + k] = Kg[k];
#pragma unroll
      for (int k = 0; k < 6; k++) st[48 + k] = Fg[k];
    }
    GM_WAVE_SYNC();
    const bool chainrow = rowf < 3 && p >= 1 && p <= CL;
    if (lane == GM_LANE_PALM_F) {
#pragma unroll
      for (int k = 0; k < 21; k++) Kg[k] = S.st.root[3][21 + k];
#pragma unroll
      for (int k = 0; k < 6; k++) Fg[k] = S.st.root[3][48 + k];
    } else if (lane == 48) {
#pragma unroll
      for (int k = 0; k < 21; k++) Kg[k] = ((S.st.root[0][21 + k] + S.st.root[1][21 + k]) + S.st.root[2][21 + k]) + S.st.root[3][21 + k];
#pragma unroll
      for (int k = 0; k < 6; k++) Fg[k] = ((S.st.root[0][48 + k] + S.st.root[1][48 + k]) + S.st.root[2][48 + k]) + S.st.root[3][48 + k];
    }
    if (chainrow || lane == GM_LANE_PALM_F || lane == 48) {
      const int d = chainrow ? T->dof_f0[rowf] + p - 1 : lane == 48 ? T->dof_base : T->dof_palm;
      real cd[6], yg[6];
#pragma unroll
      for (int k = 0; k < 6; k++) cd[k] = S.cdof[d][k];
      symK_mul(Kg, cd, yg);
      if (chainrow) {
#pragma unroll
        for (int j = 1; j <= CL; j++)
          if (j <= p) h[j] += dot6(S.cdof[T->dof_f0[rowf] + j - 1], yg);
      } else if (lane == GM_LANE_PALM_F) {
        h[1] += dot6(cd, yg);
      }
      hb[0] += dot6(cdb, yg);
      rhs += dot6(cd, Fg);
    }
  }
  // motor-lock rows (1-dof joint equalities): D on the diagonal, D aref on the rhs
  for (int r = 0; r < nl; r++) {
    const int d = __builtin_amdgcn_readlane(R.ldof, r);
    const real lD = readlane_real(R.lD, r), lR = readlane_real(R.lD * R.laref, r);
    if (T->dof_grp[d] < 3) {
      const int f = T->dof_grp[d], pd = T->dof_p[d];
      if (rowf == f && p == pd) {
#pragma unroll
        for (int j = 1; j <= CL; j++) if (j == pd) h[j] += lD;
        rhs += lR;
      }
    } else if (lane == GM_LANE_PALM_F) {
      h[1] += lD;
      rhs += lR;
    }
  }
  if constexpr (RHS_ONLY) {
    if (rowf < 3 && p >= 1 && p <= CL) S.xs[T->dof_f0[rowf] + p - 1] = rhs;
    else if (lane == GM_LANE_PALM_F) S.xs[T->dof_palm] = rhs;
    else if (lane >= 48 && lane < 55) S.xs[lane == 48 ? T->dof_base : T->dof_obj + lane - 49] = rhs;
    GM_WAVE_SYNC();
    return;
  }
  GM_WAVE_SYNC();   // the stage is read; the factor's transfers reuse the union
  PH(7);
  // ---- factor: finger chains (rows 0..2), pivots CL .. 1
  real invd = 1.0;
  if (lane < 48) {
#pragma unroll
    for (int k = CL; k >= 1; k--) {
      const real hkk = row_bcast(h[k], k);
      const real ihk = rcp_piv(hkk);
      real hk[CL + 1], hkb[7];
#pragma unroll
      for (int j = 1; j < k; j++) hk[j] = row_bcast(h[j], k);
#pragma unroll
      for (int t = 0; t < 7; t++) hkb[t] = row_bcast(hb[t], k);
      const bool upd = p >= 1 && p < k, piv = p == k;
      real Hpk = 0.0;
#pragma unroll
      for (int j = 1; j < k; j++) Hpk = (p == j) ? hk[j] : Hpk;
      const real a = Hpk * ihk;
      const real aa = upd ? a : 0.0;
      if (piv && rowf < 3) {
        real* ub = S.fs.lbub[rowf][k - 1] + 7;
#pragma unroll
        for (int t = 0; t < 7; t++) ub[t] = hb[t];
      }
      // (the pivot row's scaling by 1 / d_k is applied once after the loop: no later step
      // changes the row, whose updates from here on subtract exact zeros)
#pragma unroll
      for (int j = 1; j < k; j++) h[j] = h[j] - hk[j] * aa;
#pragma unroll
      for (int t = 0; t < 7; t++) hb[t] = hb[t] - hkb[t] * aa;
      h[k] = upd ? a : h[k];
      invd = piv ? ihk : invd;
    }
#pragma unroll
    for (int j = 1; j < CL; j++) h[j] = (j < p) ? h[j] * invd : h[j];
#pragma unroll
    for (int t = 0; t < 7; t++) hb[t] = hb[t] * invd;
    if (rowf < 3 && p >= 1 && p <= CL) {
      real* lb = S.fs.lbub[rowf][p - 1];
#pragma unroll
      for (int t = 0; t < 7; t++) lb[t] = hb[t];
    }
  } else if (lane == GM_LANE_PALM_F) {
    const real ih = rcp_piv(h[1]);
    real* pl = S.fs.plb;
#pragma unroll
    for (int t = 0; t < 7; t++) { pl[7 + t] = hb[t]; hb[t] = hb[t] * ih; pl[t] = hb[t]; }
    invd = ih;
  } else if (lane >= 48 && lane < 55) {
    // border rows to the entry transfer: lower triangle, row-major
    const int i = lane - 48;
#pragma unroll
    for (int j = 0; j < 7; j++)
      if (j <= i) S.fs.bbx[i * (i + 1) / 2 + j] = hb[j];
  }
  GM_WAVE_SYNC();
  // Schur complements: one lane per border entry (i, j), elimination order
  newton_schur<CL>(S, lane);
  GM_WAVE_SYNC();
  newton_border_factor<CL>(S, lane, hb, invd);
  PH(14);
  newton_backsolve<CL>(S, T, lane, h, hb, rhs, invd);
  PH(24);
}

#ifndef GM_NO_DECOUPLED_POINT
// ---- the decoupled Newton point: newton_point's x, bit for bit, when every contact is the
// object on the ground (constraint_setup's obj_only, which implies !any_o && !any_g there).
// H is then block diagonal: the gripper's arrow matrix with the base as its only border column,
// and the object's 6x6 block.  newton_point still strings both into one chain (CL chain
// pivots, the LDS hand-off, 28 Schur entries, 7 border pivots; the same again in the solve);
// here the object's block rides on the chains' own instructions.  Lanes 48 + i (i = 1..6) keep
// the object row's entries in h[1..i] -- row 3 has no chain, so h is free there -- and its
// base-column entry in hb0; lane 48 keeps the base row.  The chain pivot statement on
// position p of a DPP row is newton_border_factor's statement on border row bi = p, so pivots
// 6 .. 1 of the chains and of the border are one instruction stream (the chains' pivots
// CL .. 7 run on rows 0..2 alone), and so are the substitutions.  Only border entry (0, 0)
// needs a Schur sum and a forward sum; both accumulate inside the loops, in newton_schur's
// order (per chain k = CL .. 1 from +0, then rows 0, 1, 2, the palm), without LDS.
//
// What is left out are operations whose one operand is an exact zero, and a zero operand can
// still change a bit: x - (+-0) (fused: x + (-+0)) returns x for every x but x = -0, which a
// subtracted -0 turns into +0.  (Pivots are positive, H being positive definite, so scaling a
// zero keeps its sign; no value is NaN or infinite.)  Entry by entry:
//  - chain and palm rows' object columns hb[1..6] start at +0, stay +0 through the pivots
//    (+0 - (+-0) = +0) and the scaling: lb = ub = +0 on these columns.
//  - Schur entries (i, j >= 1): every sum is +0 (it starts at +0) and the palm's product is
//    +0 * +0, so the entry is unchanged, whatever it is.  Entries (i >= 1, 0): the sums are +0
//    again, the palm's product is +0 * ub_palm, -0 for a negative ub_palm; that subtraction is
//    kept (hb0 - 0.0 * Hp(1,0)).  The entry itself, -dot6(cdof, 0), is computed as before.
//  - Koo = comp + go with comp = +0: go[k] is a sum that starts at +0 and so is never -0, and
//    +0 + x = x for every other x.  Fobj = go - (+0) = go.
//  - the border pivots 6 .. 1 run as they did, column 0 included (lane 48 takes its multipliers
//    a_k, zeros with a sign, from hb0's broadcast as newton_border_factor does from bk[0]); they
//    leave entry (0, 0) alone (its update subtracts zero * zero from a positive number), so the
//    base pivot can follow them.
//  - forward, rows i >= 1: the sums are +0, the palm's product +0 * y_palm is kept.  Row 0:
//    Y = rhs - sums, then Y - a_k y_k (k = 6 .. 1), zeros that matter only to Y = -0: lane 48
//    runs these steps on a probe q = -0, which ends -0 if every product was +0 and +0
//    otherwise, and Y + q is then what the steps make of any Y.  The k = 0 step
//    (y - 0.0 * y_base on every border lane) is kept.
//  - backward, border: j = 0 (y - hb0 * x_base with lane 48's value before its own step) and
//    j = 1 .. 5 as they were.  Chain and palm rows: y - hb0 * x_base, then six subtractions of
//    +0 * x_obj[t]: -0 for a negative x_obj[t], so together they subtract -0 if any x_obj[t] has
//    its sign bit set and +0 otherwise; that one subtraction is kept.  The object's back
//    substitution therefore runs before the chains', as in newton_point.
template <int CL>
__device__ void newton_point_decoupled(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T, int lane,
                                       const RowsT& R, const bool* act, bool prof) {
  static_assert(CL >= 7, "the object's six columns sit in h[1..6] and ride on pivots 6 .. 1");
  unsigned long long t0 = prof ? clock64() : 0;
  const int ncon = S.ncon, nl = S.nl;
  real Q[6], F[3];
  newton_contact_qf<CL>(S, lane, ncon, R, act, Q, F);
  newton_ground_composites<CL>(S, T, lane, ncon, Q, F);
  PH(3);
  GM_WAVE_SYNC();   // S.go is written
  PH(4);
  // ---- H and rhs on the factor lanes: H~'s own entries on the gripper rows
  real h[CL + 1], hb0 = 0, rhs = 0;
#pragma unroll
  for (int j = 0; j <= CL; j++) h[j] = 0;
  const int rowf = lane >> 4, p = lane & 15;
  const bool chainrow = rowf < 3 && p >= 1 && p <= CL;
  const bool border = lane >= 48 && lane < 55;
  if (chainrow) {
    const int d = T->dof_f0[rowf] + p - 1;
    const real* H = S.Hf[rowf];
    real Hr[CL + 1];
#pragma unroll
    for (int j = 0; j <= CL; j++) Hr[j] = H[TRI(p, j)];
    keep_n<CL + 1>(Hr);
#pragma unroll
    for (int j = 1; j <= CL; j++) h[j] = (j <= p) ? Hr[j] : h[j];
    hb0 = Hr[0];
    rhs = S.frc[d];
  } else if (lane == GM_LANE_PALM_F) {
    h[1] = S.Hp[TRI(1, 1)];
    hb0 = S.Hp[TRI(1, 0)];
    rhs = S.frc[T->dof_palm];
  } else if (lane == 48) {
    hb0 = S.Hbb;
    rhs = S.frc[T->dof_base];
  } else if (border) {
    const int k = lane - 49;
    const real yob[6] = {0, 0, 0, 0, 0, 0};
    real KC[27], yk[6];   // Koo (21) then the row's cdof (6), loaded in one batch
#pragma unroll
    for (int t = 0; t < 21; t++) KC[t] = S.go[t];
#pragma unroll
    for (int t = 0; t < 6; t++) KC[21 + t] = S.cdof[T->dof_obj + k][t];
    keep_n<27>(KC);
    const real* cok = KC + 21;
    symK_mul(KC, cok, yk);
    hb0 = -dot6(cok, yob);
    hb0 = hb0 - 0.0 * S.Hp[TRI(1, 0)];   // (the Schur step's palm product)
    object_columns<CL>(S, T, [&](int l, const real* co) {
      const real v = S.Ho[TRI(k, l)] + dot6(co, yk);
      keep(v);
      h[1 + l] = (l <= k) ? v : h[1 + l];
    });
    rhs = S.frc[T->dof_obj + k] + dot6(cok, S.go + 21);
  }
  // motor-lock rows (1-dof joint equalities): D on the diagonal, D aref on the rhs
  for (int r = 0; r < nl; r++) {
    const int d = __builtin_amdgcn_readlane(R.ldof, r);
    const real lD = readlane_real(R.lD, r), lR = readlane_real(R.lD * R.laref, r);
    if (T->dof_grp[d] < 3) {
      const int f = T->dof_grp[d], pd = T->dof_p[d];
      if (rowf == f && p == pd) {
#pragma unroll
        for (int j = 1; j <= CL; j++) if (j == pd) h[j] += lD;
        rhs += lR;
      }
    } else if (lane == GM_LANE_PALM_F) {
      h[1] += lD;
      rhs += lR;
    }
  }
  PH(7);
  // ---- factor.  The palm's pivot first (wave-uniform copies: ub, lb, y); the base sum
  // sacc = sum lb ub of the lane's own chain accumulates beside the pivots
  real invd = 1.0, sacc = 0.0;
  const real pub = readlane_real(hb0, GM_LANE_PALM_F), ypalm = readlane_real(rhs, GM_LANE_PALM_F);
  const real pih = rcp_piv(readlane_real(h[1], GM_LANE_PALM_F));
  const real plb = pub * pih;
  // one pivot of the chain factor (newton_point's statements with a one-wide border); ROW3:
  // the border rows ride (newton_border_factor's statements: bi = p, column 0 in hb0)
#define GM_DEC_PIVOT(ROW3) do { \
    const real hkk = row_bcast(h[k], k); \
    const real ihk = rcp_piv(hkk); \
    real hk[CL + 1]; \
    _Pragma("unroll") for (int j = 1; j < k; j++) hk[j] = row_bcast(h[j], k); \
    const real hkb = row_bcast(hb0, k); \
    const bool upd = ((ROW3) && rowf == 3) ? p < k : (p >= 1 && p < k); \
    const bool piv = p == k; \
    real Hpk = ((ROW3) && lane == 48) ? hkb : 0.0; \
    _Pragma("unroll") for (int j = 1; j < k; j++) Hpk = (p == j) ? hk[j] : Hpk; \
    const real a = Hpk * ihk; \
    const real aa = upd ? a : 0.0; \
    const real lbk = hkb * ihk; \
    sacc = sacc + lbk * hkb; \
    _Pragma("unroll") for (int j = 1; j < k; j++) h[j] = h[j] - hk[j] * aa; \
    hb0 = hb0 - hkb * aa; \
    h[k] = upd ? a : h[k]; \
    invd = piv ? ihk : invd; \
  } while (0)
  if (lane < 48) {
#pragma unroll
    for (int k = CL; k >= 7; k--) GM_DEC_PIVOT(false);
  }
  if (lane < 55) {
#pragma unroll
    for (int k = 6; k >= 1; k--) GM_DEC_PIVOT(true);
#pragma unroll
    for (int j = 1; j < CL; j++) h[j] = (j < p) ? h[j] * invd : h[j];
    hb0 = (lane == 48) ? hb0 : hb0 * invd;
  } else if (lane == GM_LANE_PALM_F) {
    hb0 = hb0 * pih;
    invd = pih;
  }
#undef GM_DEC_PIVOT
  // border entry (0, 0): newton_schur's sums, then the base pivot
  const real sa0 = readlane_real(sacc, 1), sa1 = readlane_real(sacc, 17), sa2 = readlane_real(sacc, 33);
  if (lane == 48) {
    hb0 = (((hb0 - sa0) - sa1) - sa2) - plb * pub;
    invd = rcp_piv(hb0);
  }
  PH(14);
  // ---- solve: forward (the base row's sum facc = sum lb y beside the steps; lane 48 runs
  // the probe), the base row, D, backward
  real y = rhs, facc = 0.0;
  if (border) y = (lane == 48) ? -0.0 : y - 0.0 * ypalm;
#define GM_DEC_FORWARD(ROW3) do { \
    const real yk = row_bcast(y, k); \
    const real lbk = row_bcast(hb0, k); \
    facc = facc + lbk * yk; \
    const bool upd = ((ROW3) && rowf == 3) ? p < k : (p >= 1 && p < k); \
    const real Lc = upd ? h[k] : 0.0; \
    y = y - Lc * yk; \
  } while (0)
  if (lane < 48) {
#pragma unroll
    for (int k = CL; k >= 7; k--) GM_DEC_FORWARD(false);
  }
  if (lane < 55) {
#pragma unroll
    for (int k = 6; k >= 1; k--) GM_DEC_FORWARD(true);
  }
#undef GM_DEC_FORWARD
  const real fa0 = readlane_real(facc, 1), fa1 = readlane_real(facc, 17), fa2 = readlane_real(facc, 33);
  if (lane == 48) {
    const real Y = (((rhs - fa0) - fa1) - fa2) - plb * ypalm;
    y = Y + y;
  }
  const real yb6 = readlane_real(y, 48);
  if (border) y = y - 0.0 * yb6;
  y = y * invd;
  const real tb = readlane_real(y, 48);
  if (border) {
    const real Lr0 = (lane > 48) ? hb0 : 0.0;
    y = y - Lr0 * tb;
#pragma unroll
    for (int j = 1; j < 6; j++) {
      const real xj = row_bcast(y, j);
      const real Lr = (j < p) ? h[j] : 0.0;
      y = y - Lr * xj;
    }
  }
  real xb[7];
#pragma unroll
  for (int t = 0; t < 7; t++) xb[t] = readlane_real(y, 48 + t);
  bool neg = false;
#pragma unroll
  for (int t = 1; t < 7; t++) neg = neg || __double_as_longlong(xb[t]) < 0;
  const real zsub = neg ? -0.0 : 0.0;
  if (lane < 48) {
    y = y - hb0 * xb[0];
    y = y - zsub;
    y = chain_backward<CL>(y, h, p);
    if (chainrow) S.xs[T->dof_f0[rowf] + p - 1] = y;
  } else if (lane == GM_LANE_PALM_F) {
    y = y - hb0 * xb[0];
    y = y - zsub;
    S.xs[T->dof_palm] = y;
  } else if (border) {
    S.xs[lane == 48 ? T->dof_base : T->dof_obj + lane - 49] = y;
  }
  GM_WAVE_SYNC();
  PH(24);
}
#endif
GM_PHYSICS_END
