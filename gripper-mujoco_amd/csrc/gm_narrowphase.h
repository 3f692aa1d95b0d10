// gm_narrowphase.h -- the pair colliders of physics stage 2: the plane / sphere / box
// primitives, the convex (MPR) collider for cylinders and mjc_BoxBox (oracle/physics.c
// bb_setup).  Geometry in, Hit out; of SharedT only xpos / xquat and s.obj_* (geom poses).
#pragma once
#include "gm_real.h"

GM_PHYSICS_BEGIN
// ============================================================ collision
struct Hit { real dist, pos[3], n[3]; };

__device__ void make_frame(real* F, const real* n) {
  real a[3] = {0, 0, 0};
  if (fabs(n[0]) < 0.5) a[0] = 1; else a[1] = 1;
  real d = dot3(a, n);
  real t1[3] = {a[0] - d * n[0], a[1] - d * n[1], a[2] - d * n[2]};
  const real il = rsq_n(dot3(t1, t1));
  t1[0] *= il; t1[1] *= il; t1[2] *= il;
  real t2[3];
  cross3(t2, n, t1);
  F[0] = n[0]; F[1] = n[1]; F[2] = n[2];
  F[3] = t1[0]; F[4] = t1[1]; F[5] = t1[2];
  F[6] = t2[0]; F[7] = t2[1]; F[8] = t2[2];
}

struct GeomV { int type; real size[3]; real c[3]; real R[9]; real rbound; real friction; };

// world pose of a geom on body b with local pose (gp, gq) (oracle.c fk, geom part),
// computed where a pair lane needs it
template <int CL>
__device__ __forceinline__ void geom_pose(SharedT<CL>& S, int b, const double* gpos, const double* gquat, real* c,
                                          real* Rw) {
  real R[9];
  if (b == 0) {
    R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1;
  } else {
    body_R(S, b, R);
  }
  real gp[3], t[3], gq[4], Rg[9];
  ld3(gp, gpos);
  mulmv3(t, R, gp);
  const real bp0 = b == 0 ? 0.0 : S.xpos[b][0], bp1 = b == 0 ? 0.0 : S.xpos[b][1], bp2 = b == 0 ? 0.0 : S.xpos[b][2];
  c[0] = bp0 + t[0]; c[1] = bp1 + t[1]; c[2] = bp2 + t[2];
  ld4(gq, gquat);
  quat2mat(Rg, gq);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++)
      Rw[3 * i + k] = R[3 * i] * Rg[k] + R[3 * i + 1] * Rg[3 + k] + R[3 * i + 2] * Rg[6 + k];
}

// geom slot sl (0: pair_a, 1: pair_b) of candidate pair pr from the pair's flattened
// constants (GmTopo pr_*); the live object's geom reads its type and size from the env
template <int CL>
__device__ __forceinline__ void load_pair_geom(SharedT<CL>& S, const GmTopo* __restrict__ T, int pr, int sl, GeomV& G) {
  const int t = T->pr_type[pr][sl];
  if (t < 0) {
    G.type = S.s.obj_type;
    G.size[0] = S.s.obj_size[0]; G.size[1] = S.s.obj_size[1]; G.size[2] = S.s.obj_size[2];
    G.rbound = S.s.obj_rbound; G.friction = S.s.obj_friction;
  } else {
    G.type = t;
    ld3(G.size, T->pr_size[pr][sl]);
    G.rbound = (real)T->pr_rbound[pr][sl];
    G.friction = (real)T->pr_fric[pr][sl];
  }
  geom_pose(S, T->pr_body[pr][sl], T->pr_pos[pr][sl], T->pr_quat[pr][sl], G.c, G.R);
}

// plane-X multi-contact generators: k-th candidate point (returns 0 if none)
__device__ __forceinline__ int plane_box_point(const GeomV& P, const GeomV& B, int i, Hit& h) {
  real nz[3] = {P.R[2], P.R[5], P.R[8]};
  real s[3] = {(i & 1) ? B.size[0] : -B.size[0], (i & 2) ? B.size[1] : -B.size[1], (i & 4) ? B.size[2] : -B.size[2]};
  real v[3];
  mulmv3(v, B.R, s);
  v[0] += B.c[0]; v[1] += B.c[1]; v[2] += B.c[2];
  real dv[3] = {v[0] - P.c[0], v[1] - P.c[1], v[2] - P.c[2]};
  real d = dot3(dv, nz);
  if (!(d < 0)) return 0;
  h.dist = d;
  for (int k = 0; k < 3; k++) { h.pos[k] = v[k] - 0.5 * d * nz[k]; h.n[k] = nz[k]; }
  return 1;
}
// per-pair part of the plane-cylinder rim test (the rim frame: axis a, w = the in-plane
// direction towards the plane, a x w), computed once per pair instead of once per rim
// point -- the same operations, so the same values
struct CylFrame { real nz[3], a[3], w[3], axw[3]; };
__device__ __forceinline__ void cyl_frame(const GeomV& P, const GeomV& Cy, CylFrame& F) {
  F.nz[0] = P.R[2]; F.nz[1] = P.R[5]; F.nz[2] = P.R[8];
  F.a[0] = Cy.R[2]; F.a[1] = Cy.R[5]; F.a[2] = Cy.R[8];
  real na = dot3(F.nz, F.a);
  real w[3] = {-F.nz[0] + na * F.a[0], -F.nz[1] + na * F.a[1], -F.nz[2] + na * F.a[2]};
  const real lw2 = dot3(w, w);
  const real lw = sqrt_n(lw2), ilw = rsq_n(lw2);   // (independent: the test and the scale)
  if (lw < 1e-6) { w[0] = Cy.R[0]; w[1] = Cy.R[3]; w[2] = Cy.R[6]; }
  else { w[0] = w[0] * ilw; w[1] = w[1] * ilw; w[2] = w[2] * ilw; }
  F.w[0] = w[0]; F.w[1] = w[1]; F.w[2] = w[2];
  cross3(F.axw, F.a, F.w);
}
__device__ __forceinline__ int plane_cyl_point(const GeomV& P, const GeomV& Cy, const CylFrame& F, int i, Hit& h) {
  const real* nz = F.nz;
  const real* a = F.a;
  real r = Cy.size[0], hh = Cy.size[1];
  int s = i >> 2, k = i & 3;
  real sg = s == 0 ? 1.0 : -1.0;
  real dir[3];
  if (k == 0) { dir[0] = F.w[0]; dir[1] = F.w[1]; dir[2] = F.w[2]; }
  else if (k == 1) { dir[0] = F.axw[0]; dir[1] = F.axw[1]; dir[2] = F.axw[2]; }
  else if (k == 2) { dir[0] = -F.w[0]; dir[1] = -F.w[1]; dir[2] = -F.w[2]; }
  else { dir[0] = -F.axw[0]; dir[1] = -F.axw[1]; dir[2] = -F.axw[2]; }
  real v[3];
  for (int t = 0; t < 3; t++) v[t] = Cy.c[t] + sg * hh * a[t] + r * dir[t];
  real dv[3] = {v[0] - P.c[0], v[1] - P.c[1], v[2] - P.c[2]};
  real d = dot3(dv, nz);
  if (!(d < 0)) return 0;
  h.dist = d;
  for (int t = 0; t < 3; t++) { h.pos[t] = v[t] - 0.5 * d * nz[t]; h.n[t] = nz[t]; }
  return 1;
}
__device__ __forceinline__ int plane_sphere(const GeomV& P, const GeomV& Sp, Hit& h) {
  real nz[3] = {P.R[2], P.R[5], P.R[8]};
  real r = Sp.size[0];
  real dv[3] = {Sp.c[0] - P.c[0], Sp.c[1] - P.c[1], Sp.c[2] - P.c[2]};
  real dist = dot3(dv, nz) - r;
  if (!(dist < 0)) return 0;
  h.dist = dist;
  for (int k = 0; k < 3; k++) { h.pos[k] = Sp.c[k] - nz[k] * (r + 0.5 * dist); h.n[k] = nz[k]; }
  return 1;
}
__device__ __forceinline__ int sphere_box(const GeomV& Sp, const GeomV& B, Hit& h) {
  const real* R = B.R;
  const real* hs = B.size;
  real r = Sp.size[0];
  real dv[3] = {Sp.c[0] - B.c[0], Sp.c[1] - B.c[1], Sp.c[2] - B.c[2]};
  real cl[3];
  mulmtv3(cl, R, dv);
  real q[3];
  int inside = 1;
  for (int k = 0; k < 3; k++) {
    q[k] = cl[k];
    if (q[k] > hs[k]) { q[k] = hs[k]; inside = 0; }
    if (q[k] < -hs[k]) { q[k] = -hs[k]; inside = 0; }
  }
  real nl[3], dist, ql[3];
  if (!inside) {
    real df[3] = {cl[0] - q[0], cl[1] - q[1], cl[2] - q[2]};
    const real l2 = dot3(df, df);
    real l = sqrt_n(l2);
    if (l < 1e-12) return 0;
    dist = l - r;
    if (!(dist < 0)) return 0;
    const real il = rsq_n(l2);
    nl[0] = -df[0] * il; nl[1] = -df[1] * il; nl[2] = -df[2] * il;
    ql[0] = q[0]; ql[1] = q[1]; ql[2] = q[2];
  } else {
    int kmin = 0;
    real best = hs[0] - fabs(cl[0]);
    for (int k = 1; k < 3; k++) { real v = hs[k] - fabs(cl[k]); if (v < best) { best = v; kmin = k; } }
    const real clk = kmin == 0 ? cl[0] : (kmin == 1 ? cl[1] : cl[2]);
    const real hsk = kmin == 0 ? hs[0] : (kmin == 1 ? hs[1] : hs[2]);
    real sg = clk >= 0 ? 1.0 : -1.0;
    dist = -(best + r);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      nl[k] = (k == kmin) ? -sg : 0.0;
      ql[k] = (k == kmin) ? sg * hsk : cl[k];
    }
  }
  real n[3], qw[3];
  mulmv3(n, R, nl);
  mulmv3(qw, R, ql);
  h.dist = dist;
  for (int k = 0; k < 3; k++) {
    qw[k] += B.c[k];
    real sp = Sp.c[k] + n[k] * r;
    h.pos[k] = 0.5 * (qw[k] + sp);
    h.n[k] = n[k];
  }
  return 1;
}

// ---- MPR ----
struct SV { real v[3], p1[3], p2[3]; };
// TYPE: the geom type when known at compile time (mpr's cylinder-box instance), -1 = read it
template <int TYPE = -1>
__device__ __forceinline__ void support_geom(const GeomV& G, const real* d, real* out) {
  real dl[3];
  mulmtv3(dl, G.R, d);
  real pl[3] = {0, 0, 0};
  const int type = TYPE >= 0 ? TYPE : G.type;
  // face / rim-line ties take the centre (oracle.c support_geom, GM_SUPPORT_TIE)
  if (type == GM_GEOM_BOX) {
    for (int k = 0; k < 3; k++) pl[k] = fabs(dl[k]) < GM_SUPPORT_TIE ? 0.0 : (dl[k] >= 0 ? G.size[k] : -G.size[k]);
  } else if (type == GM_GEOM_CYLINDER) {
    const real rr2 = dl[0] * dl[0] + dl[1] * dl[1];
    if (rr2 > 1e-24) { const real irr = rsq_n(rr2); pl[0] = (G.size[0] * dl[0]) * irr; pl[1] = (G.size[0] * dl[1]) * irr; }
    pl[2] = fabs(dl[2]) < GM_SUPPORT_TIE ? 0.0 : (dl[2] >= 0 ? G.size[1] : -G.size[1]);
  } else if (type == GM_GEOM_SPHERE) {
    const real l2 = dot3(dl, dl);
    real l = sqrt_n(l2);
    if (l > 1e-12) { const real il = rsq_n(l2); pl[0] = (dl[0] * G.size[0]) * il; pl[1] = (dl[1] * G.size[0]) * il; pl[2] = (dl[2] * G.size[0]) * il; }
  }
  mulmv3(out, G.R, pl);
  out[0] += G.c[0]; out[1] += G.c[1]; out[2] += G.c[2];
}
template <int TA, int TB>
__device__ __forceinline__ void mpr_support(const GeomV& A, const GeomV& B, const real* d, SV& sv) {
  real nd[3] = {-d[0], -d[1], -d[2]};
  support_geom<TA>(A, d, sv.p1);
  support_geom<TB>(B, nd, sv.p2);
  sv.v[0] = sv.p1[0] - sv.p2[0]; sv.v[1] = sv.p1[1] - sv.p2[1]; sv.v[2] = sv.p1[2] - sv.p2[2];
}
__device__ __forceinline__ int fzero(real x) { return fabs(x) < 1e-12; }
// (1 / |d| as one refined reciprocal square root: half the dependent chain of sqrt then
// reciprocal; the oracle's 1 / sqrt(x) rounds twice, this once -- the MPR iterates agree to
// the last bits, the collider's contacts to ~1e-15 relative)
__device__ __forceinline__ void normalize3(real* d) {
  const real l2 = dot3(d, d);
  if (l2 > 0) { const real il = rsq_n(l2); d[0] *= il; d[1] *= il; d[2] *= il; }
}
// The simplex vertices are four named values (not an array), conditional vertex copies
// are per-component selects and every helper is inlined, so the whole MPR state stays in
// VGPRs (an indexable array, or a branch between whole-struct copies, goes to scratch).
__device__ __forceinline__ void sv_take(SV& dst, const SV& src, bool c) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    dst.v[k] = c ? src.v[k] : dst.v[k];
    dst.p1[k] = c ? src.p1[k] : dst.p1[k];
    dst.p2[k] = c ? src.p2[k] : dst.p2[k];
  }
}
__device__ __forceinline__ void portal_dir(const SV& P1, const SV& P2, const SV& P3, real* dir) {
  real a[3] = {P2.v[0] - P1.v[0], P2.v[1] - P1.v[1], P2.v[2] - P1.v[2]};
  real b[3] = {P3.v[0] - P1.v[0], P3.v[1] - P1.v[1], P3.v[2] - P1.v[2]};
  cross3(dir, a, b);
  normalize3(dir);
}
__device__ __forceinline__ void expand_portal(const SV& P0, SV& P1, SV& P2, SV& P3, const SV& v4) {
  real v4v0[3];
  cross3(v4v0, v4.v, P0.v);
  const bool s1 = dot3(P1.v, v4v0) > 0;
  const bool s2 = dot3(P2.v, v4v0) > 0;
  const bool s3 = dot3(P3.v, v4v0) > 0;
  // d1 > 0: (d2 > 0 ? P1 : P3) = v4;  else: (d3 > 0 ? P2 : P1) = v4
  sv_take(P1, v4, s1 ? s2 : !s3);
  sv_take(P2, v4, !s1 && s3);
  sv_take(P3, v4, s1 && !s2);
}
__device__ __forceinline__ int reach_tol(const SV& P1, const SV& P2, const SV& P3, const SV& v4, const real* dir, real tol) {
  real dv1 = dot3(P1.v, dir), dv2 = dot3(P2.v, dir), dv3 = dot3(P3.v, dir), dv4 = dot3(v4.v, dir);
  real d1 = dv4 - dv1, d2 = dv4 - dv2, d3 = dv4 - dv3;
  real dd = fmin(fmin(d1, d2), d3);
  return dd < tol || fabs(dd - tol) < 1e-12;
}
__device__ __forceinline__ void tri_closest_origin(const real* a, const real* b, const real* c, real* out) {
  real ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  real ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  real ap[3] = {-a[0], -a[1], -a[2]};
  real d1 = dot3(ab, ap), d2 = dot3(ac, ap);
  if (d1 <= 0 && d2 <= 0) { out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; return; }
  real bp[3] = {-b[0], -b[1], -b[2]};
  real d3 = dot3(ab, bp), d4 = dot3(ac, bp);
  if (d3 >= 0 && d4 <= d3) { out[0] = b[0]; out[1] = b[1]; out[2] = b[2]; return; }
  real vc = d1 * d4 - d3 * d2;
  if (vc <= 0 && d1 >= 0 && d3 <= 0) { real v = div_n(d1, d1 - d3); for (int k = 0; k < 3; k++) out[k] = a[k] + v * ab[k]; return; }
  real cp[3] = {-c[0], -c[1], -c[2]};
  real d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  if (d6 >= 0 && d5 <= d6) { out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; return; }
  real vb = d5 * d2 - d1 * d6;
  if (vb <= 0 && d2 >= 0 && d6 <= 0) { real w = div_n(d2, d2 - d6); for (int k = 0; k < 3; k++) out[k] = a[k] + w * ac[k]; return; }
  real va = d3 * d6 - d5 * d4;
  if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) {
    real w = div_n(d4 - d3, (d4 - d3) + (d5 - d6));
    for (int k = 0; k < 3; k++) out[k] = b[k] + w * (c[k] - b[k]);
    return;
  }
  real den = rcp_n(va + vb + vc);
  real v = vb * den, w = vc * den;
  for (int k = 0; k < 3; k++) out[k] = a[k] + ab[k] * v + ac[k] * w;
}
__device__ __forceinline__ void mpr_pos(const SV& P0, const SV& P1, const SV& P2, const SV& P3, real* pos) {
  real dir[3];
  portal_dir(P1, P2, P3, dir);
  real t[3];
  cross3(t, P1.v, P2.v); real b0 = dot3(t, P3.v);
  cross3(t, P3.v, P2.v); real b1 = dot3(t, P0.v);
  cross3(t, P0.v, P1.v); real b2 = dot3(t, P3.v);
  cross3(t, P2.v, P1.v); real b3 = dot3(t, P0.v);
  real sum = b0 + b1 + b2 + b3;
  if (sum <= 0) {
    b0 = 0;
    cross3(t, P2.v, P3.v); b1 = dot3(t, dir);
    cross3(t, P3.v, P1.v); b2 = dot3(t, dir);
    cross3(t, P1.v, P2.v); b3 = dot3(t, dir);
    sum = b1 + b2 + b3;
  }
  real inv = rcp_n(sum);
  real p1[3] = {0, 0, 0}, p2[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    p1[k] += b0 * P0.p1[k]; p2[k] += b0 * P0.p2[k];
    p1[k] += b1 * P1.p1[k]; p2[k] += b1 * P1.p2[k];
    p1[k] += b2 * P2.p1[k]; p2[k] += b2 * P2.p2[k];
    p1[k] += b3 * P3.p1[k]; p2[k] += b3 * P3.p2[k];
  }
  for (int k = 0; k < 3; k++) pos[k] = 0.5 * (p1[k] + p2[k]) * inv;
}
// TA, TB: the two geoms' types when known at compile time (-1: read per lane)
template <int TA = -1, int TB = -1>
__device__ __forceinline__ int mpr(const GeomV& A, const GeomV& B, real tol, int maxit, Hit& h) {
  SV P0, P1, P2, P3;
  for (int k = 0; k < 3; k++) { P0.v[k] = A.c[k] - B.c[k]; P0.p1[k] = A.c[k]; P0.p2[k] = B.c[k]; }
  if (fzero(P0.v[0]) && fzero(P0.v[1]) && fzero(P0.v[2])) P0.v[0] += 1e-5;
  real d[3] = {-P0.v[0], -P0.v[1], -P0.v[2]};
  normalize3(d);
  mpr_support<TA, TB>(A, B, d, P1);
  if (dot3(P1.v, d) <= 0) return 0;
  cross3(d, P0.v, P1.v);
  if (fzero(sqrt_n(dot3(d, d)))) {
    real l1 = sqrt_n(dot3(P1.v, P1.v));
    if (fzero(l1)) return 0;
    h.dist = -l1;
    real il = rcp_n(l1);
    for (int k = 0; k < 3; k++) { h.n[k] = P1.v[k] * il; h.pos[k] = 0.5 * (P1.p1[k] + P1.p2[k]); }
    return 1;
  }
  normalize3(d);
  mpr_support<TA, TB>(A, B, d, P2);
  if (dot3(P2.v, d) <= 0) return 0;
  real va[3], vb[3];
  for (int k = 0; k < 3; k++) { va[k] = P1.v[k] - P0.v[k]; vb[k] = P2.v[k] - P0.v[k]; }
  cross3(d, va, vb);
  normalize3(d);
  if (dot3(d, P0.v) > 0) {
    const SV t = P1;
    sv_take(P1, P2, true); sv_take(P2, t, true);
    d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2];
  }
  int it = 0;
  for (;;) {
    mpr_support<TA, TB>(A, B, d, P3);
    if (dot3(P3.v, d) <= 0) return 0;
    cross3(va, P1.v, P3.v);
    const bool c2 = dot3(va, P0.v) < -1e-12;
    cross3(va, P3.v, P2.v);
    const bool c1 = !c2 && dot3(va, P0.v) < -1e-12;
    sv_take(P2, P3, c2);
    sv_take(P1, P3, c1);
    if (!(c1 || c2)) break;
    for (int k = 0; k < 3; k++) { va[k] = P1.v[k] - P0.v[k]; vb[k] = P2.v[k] - P0.v[k]; }
    cross3(d, va, vb);
    normalize3(d);
    if (++it > maxit) return 0;
  }
  it = 0;
  for (;;) {
    portal_dir(P1, P2, P3, d);
    if (dot3(d, P1.v) >= -1e-12) break;
    SV v4;
    mpr_support<TA, TB>(A, B, d, v4);
    real dv4 = dot3(v4.v, d);
    if (!(fzero(dv4) || dv4 > 0)) return 0;
    if (reach_tol(P1, P2, P3, v4, d, tol)) return 0;
    expand_portal(P0, P1, P2, P3, v4);
    if (++it > maxit) return 0;
  }
  it = 0;
  for (;;) {
    portal_dir(P1, P2, P3, d);
    SV v4;
    mpr_support<TA, TB>(A, B, d, v4);
    if (reach_tol(P1, P2, P3, v4, d, tol) || it > maxit) {
      real cp[3];
      tri_closest_origin(P1.v, P2.v, P3.v, cp);
      const real dp2 = dot3(cp, cp);
      real depth = sqrt_n(dp2);
      if (fzero(depth)) return 0;
      h.dist = -depth;
      real id = rsq_n(dp2);
      h.n[0] = cp[0] * id; h.n[1] = cp[1] * id; h.n[2] = cp[2] * id;
      mpr_pos(P0, P1, P2, P3, h.pos);
      return depth > 0;
    }
    expand_portal(P0, P1, P2, P3, v4);
    it++;
  }
}

// ------------------------------------------------------------ box-box (mjc_BoxBox)
// Separating axes, then the face-clipped manifold (see oracle/physics.c bb_setup): the
// face case keeps up to 8 of 24 candidates (incident vertices inside the reference face,
// reference corners inside the incident face, edge crossings) below the reference face.
#define BB_NCAND 24
struct BBox {
  int kind;                     // 0 none, 1 face, 2 edge
  real n[3], pen, sgn;
  real crf[3], ru[3], rv[3], hu, hv;
  real V[4][3], cinc[3], ninc[3], pu[4], pv[4];
};

__device__ __forceinline__ void bb_setup(const GeomV& A, const GeomV& B, BBox& S, real* ea, real* eb, real* da,
                                         real* db) {
  S.kind = 0;
  const real d[3] = {B.c[0] - A.c[0], B.c[1] - A.c[1], B.c[2] - A.c[2]};
  real a[3][3], b[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) { a[i][k] = A.R[3 * k + i]; b[i][k] = B.R[3 * k + i]; }
  real Ca[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) Ca[i][j] = fabs(dot3(a[i], b[j]));
  real best = 0;
  int code = -1;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const real rb = B.size[0] * Ca[i][0] + B.size[1] * Ca[i][1] + B.size[2] * Ca[i][2];
    const real pen = (A.size[i] + rb) - fabs(dot3(d, a[i]));
    if (pen < 0) return;
    if (code < 0 || pen < best) { best = pen; code = i; }
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const real ra = A.size[0] * Ca[0][j] + A.size[1] * Ca[1][j] + A.size[2] * Ca[2][j];
    const real pen = (ra + B.size[j]) - fabs(dot3(d, b[j]));
    if (pen < 0) return;
    if (pen < best) { best = pen; code = 3 + j; }
  }
  real ebest = 0, eL[3] = {0, 0, 0};
  int ecode = -1;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      real L[3];
      cross3(L, a[i], b[j]);
      const real len2 = dot3(L, L);
      const real len = sqrt_n(len2);
      if (len < 1e-6) continue;
      const real il = rsq_n(len2);
      L[0] *= il; L[1] *= il; L[2] *= il;
      const real ra = A.size[0] * fabs(dot3(a[0], L)) + A.size[1] * fabs(dot3(a[1], L)) + A.size[2] * fabs(dot3(a[2], L));
      const real rb = B.size[0] * fabs(dot3(b[0], L)) + B.size[1] * fabs(dot3(b[1], L)) + B.size[2] * fabs(dot3(b[2], L));
      const real pen = (ra + rb) - fabs(dot3(d, L));
      if (pen < 0) return;
      if (ecode < 0 || pen < ebest) { ebest = pen; ecode = 3 * i + j; eL[0] = L[0]; eL[1] = L[1]; eL[2] = L[2]; }
    }
  if (ecode >= 0 && ebest < 0.95 * best) {
    const int i = ecode / 3, j = ecode % 3;
    real L[3] = {eL[0], eL[1], eL[2]};
    if (dot3(d, L) < 0) { L[0] = -L[0]; L[1] = -L[1]; L[2] = -L[2]; }
    S.kind = 2;
    S.pen = ebest;
    S.n[0] = L[0]; S.n[1] = L[1]; S.n[2] = L[2];
#pragma unroll
    for (int k = 0; k < 3; k++) { ea[k] = A.c[k]; eb[k] = B.c[k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      da[k] = (i == 0) ? a[0][k] : (i == 1) ? a[1][k] : a[2][k];
      db[k] = (j == 0) ? b[0][k] : (j == 1) ? b[1][k] : b[2][k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (k != i) {
        const real s = dot3(a[k], L) >= 0 ? A.size[k] : -A.size[k];
#pragma unroll
        for (int t = 0; t < 3; t++) ea[t] += s * a[k][t];
      }
      if (k != j) {
        const real s = dot3(b[k], L) >= 0 ? -B.size[k] : B.size[k];
#pragma unroll
        for (int t = 0; t < 3; t++) eb[t] += s * b[k][t];
      }
    }
    return;
  }
  const bool ref_is_a = code < 3;
  const int ri = ref_is_a ? code : code - 3;
  // reference / incident box data by selection (no pointer to a register array)
  real rc[3], ic[3], rs[3], is[3], ra[3][3], ia[3][3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    rc[k] = ref_is_a ? A.c[k] : B.c[k];
    ic[k] = ref_is_a ? B.c[k] : A.c[k];
    rs[k] = ref_is_a ? A.size[k] : B.size[k];
    is[k] = ref_is_a ? B.size[k] : A.size[k];
#pragma unroll
    for (int t = 0; t < 3; t++) { ra[k][t] = ref_is_a ? a[k][t] : b[k][t]; ia[k][t] = ref_is_a ? b[k][t] : a[k][t]; }
  }
  real rax[3], rau[3], rav[3];
  const int ui = (ri + 1) % 3, vi = (ri + 2) % 3;
#pragma unroll
  for (int t = 0; t < 3; t++) {
    rax[t] = ri == 0 ? ra[0][t] : ri == 1 ? ra[1][t] : ra[2][t];
    rau[t] = ui == 0 ? ra[0][t] : ui == 1 ? ra[1][t] : ra[2][t];
    rav[t] = vi == 0 ? ra[0][t] : vi == 1 ? ra[1][t] : ra[2][t];
  }
  const real rsi = ri == 0 ? rs[0] : ri == 1 ? rs[1] : rs[2];
  const real dd[3] = {ic[0] - rc[0], ic[1] - rc[1], ic[2] - rc[2]};
  const real s0 = dot3(dd, rax) >= 0 ? 1.0 : -1.0;
  S.kind = 1;
  S.pen = best;
  S.sgn = ref_is_a ? 1.0 : -1.0;
#pragma unroll
  for (int k = 0; k < 3; k++) S.n[k] = s0 * rax[k];
#pragma unroll
  for (int k = 0; k < 3; k++) { S.crf[k] = rc[k] + rsi * S.n[k]; S.ru[k] = rau[k]; S.rv[k] = rav[k]; }
  S.hu = ui == 0 ? rs[0] : ui == 1 ? rs[1] : rs[2];
  S.hv = vi == 0 ? rs[0] : vi == 1 ? rs[1] : rs[2];
  int jm = 0;
  real bm = fabs(dot3(S.n, ia[0]));
#pragma unroll
  for (int j = 1; j < 3; j++) { const real v = fabs(dot3(S.n, ia[j])); if (v > bm) { bm = v; jm = j; } }
  real iaj[3], ie1[3], ie2[3];
  const int e1 = (jm + 1) % 3, e2 = (jm + 2) % 3;
#pragma unroll
  for (int t = 0; t < 3; t++) {
    iaj[t] = jm == 0 ? ia[0][t] : jm == 1 ? ia[1][t] : ia[2][t];
    ie1[t] = e1 == 0 ? ia[0][t] : e1 == 1 ? ia[1][t] : ia[2][t];
    ie2[t] = e2 == 0 ? ia[0][t] : e2 == 1 ? ia[1][t] : ia[2][t];
  }
  const real isj = jm == 0 ? is[0] : jm == 1 ? is[1] : is[2];
  const real h1 = e1 == 0 ? is[0] : e1 == 1 ? is[1] : is[2];
  const real h2 = e2 == 0 ? is[0] : e2 == 1 ? is[1] : is[2];
  const real sj = dot3(S.n, iaj) >= 0 ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 3; k++) { S.ninc[k] = sj * iaj[k]; S.cinc[k] = ic[k] + isj * S.ninc[k]; }
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const real su = (q == 1 || q == 2) ? 1.0 : -1.0, sv = (q >= 2) ? 1.0 : -1.0;
#pragma unroll
    for (int k = 0; k < 3; k++) S.V[q][k] = S.cinc[k] + (su * h1) * ie1[k] + (sv * h2) * ie2[k];
    const real r[3] = {S.V[q][0] - S.crf[0], S.V[q][1] - S.crf[1], S.V[q][2] - S.crf[2]};
    S.pu[q] = dot3(r, S.ru);
    S.pv[q] = dot3(r, S.rv);
  }
}
// face candidate i (see oracle/physics.c bb_face_cand); i compile-time after unrolling
__device__ __forceinline__ int bb_face_cand(const BBox& S, int i, real* P, real& depth) {
  if (i < 4) {
    if (!(fabs(S.pu[i]) <= S.hu && fabs(S.pv[i]) <= S.hv)) return 0;
    P[0] = S.V[i][0]; P[1] = S.V[i][1]; P[2] = S.V[i][2];
  } else if (i < 8) {
    const int m = i - 4;
    const real cu = (m == 1 || m == 2) ? S.hu : -S.hu, cv = (m >= 2) ? S.hv : -S.hv;
    real sgn_min = 0, sgn_max = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int q1 = (q + 1) & 3;
      const real ex = S.pu[q1] - S.pu[q], ey = S.pv[q1] - S.pv[q];
      const real cr = ex * (cv - S.pv[q]) - ey * (cu - S.pu[q]);
      if (q == 0) { sgn_min = cr; sgn_max = cr; }
      else { sgn_min = fmin(sgn_min, cr); sgn_max = fmax(sgn_max, cr); }
    }
    if (!(sgn_min >= 0 || sgn_max <= 0)) return 0;
    real Q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) Q[k] = S.crf[k] + cu * S.ru[k] + cv * S.rv[k];
    const real den = dot3(S.ninc, S.n);
    if (fabs(den) < 1e-12) return 0;
    const real r[3] = {S.cinc[0] - Q[0], S.cinc[1] - Q[1], S.cinc[2] - Q[2]};
    const real t = div_n(dot3(S.ninc, r), den);
#pragma unroll
    for (int k = 0; k < 3; k++) P[k] = Q[k] + t * S.n[k];
  } else {
    const int q = (i - 8) >> 2, m = (i - 8) & 3;
    const int q1 = (q + 1) & 3;
    const real du = S.pu[q1] - S.pu[q], dv = S.pv[q1] - S.pv[q];
    real t;
    if (m < 2) {
      if (fabs(du) < 1e-15) return 0;
      const real bound = m == 0 ? -S.hu : S.hu;
      t = div_n(bound - S.pu[q], du);
      if (!(t > 0 && t < 1)) return 0;
      const real vt = S.pv[q] + t * dv;
      if (!(fabs(vt) < S.hv)) return 0;
    } else {
      if (fabs(dv) < 1e-15) return 0;
      const real bound = m == 2 ? -S.hv : S.hv;
      t = div_n(bound - S.pv[q], dv);
      if (!(t > 0 && t < 1)) return 0;
      const real ut = S.pu[q] + t * du;
      if (!(fabs(ut) < S.hu)) return 0;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) P[k] = S.V[q][k] + t * (S.V[q1][k] - S.V[q][k]);
  }
  const real r[3] = {S.crf[0] - P[0], S.crf[1] - P[1], S.crf[2] - P[2]};
  depth = dot3(S.n, r);
  return depth > 0;
}
__device__ __forceinline__ void bb_face_hit(const BBox& S, const real* P, real depth, Hit& h) {
  h.dist = -depth;
#pragma unroll
  for (int k = 0; k < 3; k++) { h.pos[k] = P[k] + (0.5 * depth) * S.n[k]; h.n[k] = S.sgn * S.n[k]; }
}
__device__ __forceinline__ int bb_edge_hit(const BBox& S, const real* ea, const real* eb, const real* da,
                                           const real* db, Hit& h) {
  const real w[3] = {ea[0] - eb[0], ea[1] - eb[1], ea[2] - eb[2]};
  const real b = dot3(da, db), dd = dot3(da, w), e = dot3(db, w);
  const real den = 1.0 - b * b;
  if (!(den > 1e-12)) return 0;
  const real s = div_n(b * e - dd, den), t = div_n(e - b * dd, den);
  h.dist = -S.pen;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const real pa = ea[k] + s * da[k], pb = eb[k] + t * db[k];
    h.pos[k] = 0.5 * (pa + pb);
    h.n[k] = S.n[k];
  }
  return 1;
}
GM_PHYSICS_END
