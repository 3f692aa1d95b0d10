// gm_collide.h -- physics stage 2, mj_collision: one lane per candidate geom pair (broadphase
// by bounding spheres, then gm_narrowphase.h), contacts written in pair order, one contact
// frame per lane.  SharedT: reads xpos, xquat, s.obj_*; writes con, cgeom, cbody, pair_off,
// pair_cnt, ncon, overflow, work_mpr and the box-box hit slots (cl.hit, or a DUO helper's own).
#pragma once
#include "gm_narrowphase.h"

__host__ __device__ constexpr int gm_pair_batches(int CL) { return CL <= 10 ? 1 : 2; }

GM_PHYSICS_BEGIN
// canonical (geom1, geom2): lower type first, then lower id
__device__ __forceinline__ void canon_pair(int a, int b, int ta, int tb, int& g1, int& g2) {
  if (ta > tb || (ta == tb && a > b)) { g1 = b; g2 = a; } else { g1 = a; g2 = b; }
}

// pass 2 stores the hit (depth, point, normal), friction and the geom/body ids; the contact
// frame's tangent and the zeroed tail are filled by collision()'s lane-per-contact epilogue
template <int CL>
__device__ __forceinline__ void write_contact(SharedT<CL>& S, int slot, int g1, int g2, int b1, int b2, const Hit& h,
                                              real mu) {
  real* C = S.con[slot];
  C[0] = h.dist;
  C[1] = h.pos[0]; C[2] = h.pos[1]; C[3] = h.pos[2];
  C[4] = h.n[0]; C[5] = h.n[1]; C[6] = h.n[2];
  C[10] = mu;
  S.cgeom[slot][0] = (int16_t)g1; S.cgeom[slot][1] = (int16_t)g2;
  S.cbody[slot][0] = (int16_t)b1; S.cbody[slot][1] = (int16_t)b2;
}

// hit: the box-box hit slots (S.cl.hit, in the union; a DUO workgroup's helper wave passes
// its own array, the union being live with crb_rne's composites while it runs)
template <int CL>
__device__ __forceinline__ bool collision(SharedT<CL>& S, const gm_model* __restrict__ m, const GmTopo* __restrict__ T, int lane,
                          bool prof, real (*hit)[8][4]) {
  unsigned long long t0 = prof ? clock64() : 0;
  (void)t0;
  // one lane per candidate pair, in batches of 64 pairs: the 6 N + 15 pairs fit one batch
  // for N <= 8 (CL <= 10), N = 9, 10 take two (gm_create checks npair against this);
  // contacts keep the pair order across batches
  constexpr int NBATCH = gm_pair_batches(CL);
  int written = 0;
  bool ran_mpr = false;   // profiling: a lane of this env ran the convex (MPR) collider
  // (not unrolled: with two batches (N = 9, 10) the unrolled copies held each other's
  // collider state live and the pair loop spilled ~1 K scratch operations per substep)
#pragma nounroll
  for (int bi = 0; bi < NBATCH; bi++) {
    const int pr = bi * NT + lane;
    int cnt = 0, kind = 0, g1 = 0, g2 = 0, b1 = 0, b2 = 0;
    unsigned hm = 0;   // multi-point colliders: the counted candidates (pass 2 revisits only these)
    Hit single;
    GeomV A, B;
    CylFrame cf;
    BBox bbs;
    int bslot = -1;          // box-box face case: this lane's hit slot (S.cl), -1 = none
    real bn[3] = {0, 0, 0}, bsg = 0;   // and its manifold normal / sign
    real ea[3], eb[3], da[3], db[3];
    if (pr < T->npair) {
      const int a = T->pr_g[pr][0], b = T->pr_g[pr][1];
      const int ta0 = T->pr_type[pr][0], tb0 = T->pr_type[pr][1];
      const int ta = ta0 < 0 ? S.s.obj_type : ta0, tb = tb0 < 0 ? S.s.obj_type : tb0;
      canon_pair(a, b, ta, tb, g1, g2);
      const int s1 = (g1 == a) ? 0 : 1;
      b1 = T->pr_body[pr][s1]; b2 = T->pr_body[pr][1 - s1];   // kept with the contact (LDS)
      load_pair_geom(S, T, pr, s1, A);
      load_pair_geom(S, T, pr, 1 - s1, B);
      bool pass;
      if (A.type == GM_GEOM_PLANE) {
        real nz[3] = {A.R[2], A.R[5], A.R[8]};
        real dv[3] = {B.c[0] - A.c[0], B.c[1] - A.c[1], B.c[2] - A.c[2]};
        pass = !(dot3(dv, nz) > B.rbound);
      } else {
        real dv[3] = {B.c[0] - A.c[0], B.c[1] - A.c[1], B.c[2] - A.c[2]};
        real rr = A.rbound + B.rbound;
        pass = !(dot3(dv, dv) > rr * rr);
      }
      if (pass) {
        if (A.type == GM_GEOM_PLANE) {
          if (B.type == GM_GEOM_SPHERE) { kind = 1; cnt = plane_sphere(A, B, single); }
          else if (B.type == GM_GEOM_BOX) {
            kind = 2;
            Hit t;
            for (int i = 0; i < 8 && cnt < 4; i++) {
              const int ok = plane_box_point(A, B, i, t);
              hm |= (unsigned)ok << i;
              cnt += ok;
            }
          } else if (B.type == GM_GEOM_CYLINDER) {
            kind = 3;
            Hit t;
            cyl_frame(A, B, cf);
            for (int i = 0; i < 8 && cnt < 4; i++) {
              const int ok = plane_cyl_point(A, B, cf, i, t);
              hm |= (unsigned)ok << i;
              cnt += ok;
            }
          }
        } else if (A.type == GM_GEOM_SPHERE && B.type == GM_GEOM_BOX) {
          kind = 1; cnt = sphere_box(A, B, single);
        } else if (A.type == GM_GEOM_BOX && B.type == GM_GEOM_BOX) {
          // mjc_BoxBox: separating axes, then the face-clipped manifold or one edge contact
          bb_setup(A, B, bbs, ea, eb, da, db);
          if (bbs.kind == 1) {
            kind = 4;
            // this lane's hit slot: its rank among the face-case lanes (the active lanes here)
            const unsigned long long fb = __ballot(1);
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(fb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)fb, 0u));
            bslot = rank < GM_BB_SLOTS ? rank : -1;
#pragma unroll
            for (int i = 0; i < BB_NCAND; i++) {
              if (cnt < 8) {
                real P[3], dep;
                const int ok = bb_face_cand(bbs, i, P, dep);
                if (ok && bslot >= 0) {
                  real* hs = hit[bslot][cnt];
                  hs[0] = P[0]; hs[1] = P[1]; hs[2] = P[2]; hs[3] = dep;
                }
                hm |= (unsigned)ok << i;
                cnt += ok;
              }
            }
            bn[0] = bbs.n[0]; bn[1] = bbs.n[1]; bn[2] = bbs.n[2]; bsg = bbs.sgn;
          } else if (bbs.kind == 2) {
            kind = 1; cnt = bb_edge_hit(bbs, ea, eb, da, db, single);
          }
        } else {
          ran_mpr = true;
          // a cylinder against a box (the gripper's links against a cylinder object) on every
          // MPR lane: the instance with the support types fixed, no type test per support call
          const bool cb = A.type == GM_GEOM_CYLINDER && B.type == GM_GEOM_BOX;
          if (__ballot(!cb) == 0ull)
            cnt = mpr<GM_GEOM_CYLINDER, GM_GEOM_BOX>(A, B, (real)m->mpr_tolerance, m->mpr_iterations, single);
          else
            cnt = mpr(A, B, (real)m->mpr_tolerance, m->mpr_iterations, single);
          kind = 1;
          if (cnt && !(single.dist < 0)) cnt = 0;
        }
      }
    }
    // contact slots: exclusive prefix sum of the per-lane counts (0..8, four bits) from
    // four ballots -- no LDS round trip
    int off = written, total = 0;
#pragma unroll
    for (int bit = 0; bit < 4; bit++) {
      const unsigned long long bal = __ballot((cnt >> bit) & 1);
      off += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u)) << bit;
      total += __popcll(bal) << bit;
    }
    if (pr < T->npair) { S.pair_off[pr] = (int16_t)off; S.pair_cnt[pr] = (int16_t)cnt; }
    if (cnt > 0) {
      real mu = fmax(A.friction, B.friction);
      if (kind == 1) {
        if (off < GM_MAX_CON) write_contact(S, off, g1, g2, b1, b2, single, mu);
      } else if (kind == 4 && bslot >= 0) {
        // the stored hits, in candidate order as pass 1 found them (bb_face_hit's operations)
        for (int w = 0; w < cnt; w++) {
          const real* hs = hit[bslot][w];
          const real dep = hs[3];
          Hit t;
          t.dist = -dep;
#pragma unroll
          for (int k = 0; k < 3; k++) { t.pos[k] = hs[k] + (0.5 * dep) * bn[k]; t.n[k] = bsg * bn[k]; }
          if (off + w < GM_MAX_CON) write_contact(S, off + w, g1, g2, b1, b2, t, mu);
        }
      } else if (kind == 4) {
        // (more face-case lanes than slots: the counted candidates again)
        int w = 0;
#pragma unroll
        for (int i = 0; i < BB_NCAND; i++) {
          if ((hm >> i) & 1u) {
            real P[3], dep;
            Hit t;
            bb_face_cand(bbs, i, P, dep);
            bb_face_hit(bbs, P, dep, t);
            if (off + w < GM_MAX_CON) write_contact(S, off + w, g1, g2, b1, b2, t, mu);
            w++;
          }
        }
      } else {
        Hit t;
        int w = 0;
        while (hm) {   // the counted corners in index order, as pass 1 found them
          const int i = __builtin_ctz(hm);
          hm &= hm - 1;
          if (kind == 2) plane_box_point(A, B, i, t);
          else plane_cyl_point(A, B, cf, i, t);
          if (off + w < GM_MAX_CON) write_contact(S, off + w, g1, g2, b1, b2, t, mu);
          w++;
        }
      }
    }
    written += total;
  }
  const bool any_mpr = __ballot(ran_mpr) != 0;
  if (lane == 0 && any_mpr) {
    S.work_mpr += 1;
    if (prof) S.tph[29] += 1;
  }
  // contact frames, one contact per lane (GM_MAX_CON <= 64): the normal and a tangent, as
  // make_frame builds them; the rest of the frame is implied by the two
  static_assert(GM_MAX_CON <= NT, "contact frames: one lane per contact");
  const int ncon = written < GM_MAX_CON ? written : GM_MAX_CON;
  GM_WAVE_SYNC();
  if (lane < ncon) {
    real* C = S.con[lane];
    const real n[3] = {C[4], C[5], C[6]};
    real F[9];
    make_frame(F, n);
    C[7] = F[3]; C[8] = F[4]; C[9] = F[5];
    C[11] = 0; C[12] = 0; C[13] = 0;
  }
  if (lane == 0) {
    S.ncon = ncon;
    S.overflow = written > GM_MAX_CON;
  }
  GM_WAVE_SYNC();
  return any_mpr;
}
GM_PHYSICS_END
using gmf::collision;
