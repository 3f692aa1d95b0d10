// gm_real.h -- small math: the correctly rounded sqrt / rcp / div family (selected by
// GM_LIBM_DIVSQRT and, twice, by the calibration unit's GM_CAL_TU), ld3 / ld4, gm_fphelpers.inc
// (included twice on purpose: unfused at file scope, contracted in namespace gmf), the topology
// accessors, the DPP row moves and the physics stages' fp-contraction bracket.  Restates no
// reference function; of SharedT it reads xquat (body_R).
#pragma once
#include "gm_shared.h"

// ------------------------------------------------------------ small math
// Correctly rounded fp64 sqrt, reciprocal and quotient on the compiler's own expansions
// (v_rsq_f64 / v_rcp_f64 and the same FMA refinement steps, operation for operation) minus
// their range pre-/post-scaling and special-value fix-ups, which cost a third of the
// instructions and sit on the dependent chain.  Bit-identical to sqrt(x), 1.0 / b and a / b
// wherever the scaling is inactive: x >= 2^-767 or x == +-0; |a|, |b|, |a / b| roughly
// inside [2^-900, 2^900] -- every call site's operands are lengths in metres, masses,
// pivots and contact quantities.  (b == 0 gives NaN where the library gives inf; every
// caller guards its zero case or is in a blown-up state already.)  -DGM_LIBM_DIVSQRT
// selects the library operations.
#ifndef GM_LIBM_DIVSQRT
__device__ __forceinline__ double sqrt_n(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = y * 0.5;
  const double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  double d = fma(-g, g, x);
  h = fma(h, r, h);
  g = fma(d, h, g);
  d = fma(-g, g, x);
  g = fma(d, h, g);
  return x == 0.0 ? x : g;
}
// 1 / sqrt(x) for normal x > 0: v_rsq_f64 and two Newton steps (normalising directions in
// the physics substep); rcp_piv: a factor pivot's reciprocal, two Newton steps without the
// final correction.  The calibration build (GM_CAL_TU: stability verdicts compared with the
// oracle candidate for candidate) takes the correctly rounded forms instead.
#ifndef GM_CAL_TU
__device__ __forceinline__ double rsq_n(double x) {
  double y = __builtin_amdgcn_rsq(x);
  const double hx = 0.5 * x;
  double e = fma(-hx * y, y, 0.5);
  y = fma(y, e, y);
  e = fma(-hx * y, y, 0.5);
  return fma(y, e, y);
}
#endif
__device__ __forceinline__ double rcp_refined(double b) {
  double r = __builtin_amdgcn_rcp(b);
  double e = fma(-b, r, 1.0);
  r = fma(r, e, r);
  e = fma(-b, r, 1.0);
  return fma(r, e, r);
}
__device__ __forceinline__ double rcp_n(double b) {
  const double r = rcp_refined(b);
  return fma(fma(-b, r, 1.0), r, r);
}
__device__ __forceinline__ double div_n(double a, double b) {
  const double r = rcp_refined(b);
  const double q = a * r;
  return fma(fma(-b, q, a), r, q);
}
#ifdef GM_CAL_TU
__device__ __forceinline__ double rsq_n(double x) { return rcp_n(sqrt_n(x)); }
__device__ __forceinline__ double rcp_piv(double b) { return rcp_n(b); }
#else
__device__ __forceinline__ double rcp_piv(double b) { return rcp_refined(b); }
#endif
#else
__device__ __forceinline__ double sqrt_n(double x) { return sqrt(x); }
__device__ __forceinline__ double rsq_n(double x) { return 1.0 / sqrt(x); }
__device__ __forceinline__ double rcp_piv(double b) { return 1.0 / b; }
__device__ __forceinline__ double rcp_n(double b) { return 1.0 / b; }
__device__ __forceinline__ double div_n(double a, double b) { return a / b; }
#endif

__device__ __forceinline__ void ld3(float* r, const double* a) { r[0] = (float)a[0]; r[1] = (float)a[1]; r[2] = (float)a[2]; }
__device__ __forceinline__ void ld3(double* r, const double* a) { r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; }
__device__ __forceinline__ void ld4(double* r, const double* a) { r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3]; }
__device__ __forceinline__ void ld4(float* r, const double* a) { r[0] = (float)a[0]; r[1] = (float)a[1]; r[2] = (float)a[2]; r[3] = (float)a[3]; }

#include "gm_fphelpers.inc"
template <int CL>
__device__ __forceinline__ void body_R(const SharedT<CL>& S, int b, real* R) {
  const real q[4] = {S.xquat[b][0], S.xquat[b][1], S.xquat[b][2], S.xquat[b][3]};
  quat2mat(R, q);
}   // (one definition: ADL on SharedT would make a second one ambiguous)

// ------------------------------------------------------------ topology helpers
// chain c: 0..2 finger, 3 palm, 4 object.  Chain lengths (positions >= 1).
__device__ __forceinline__ int chain_len(const GmTopo* T, int c) { return c < 3 ? T->CL : (c == 3 ? 1 : 6); }
__device__ __forceinline__ int chain_body(const GmTopo* T, int c, int p) {
  if (c < 3) return T->body_f0[c] + p - 1;
  if (c == 3) return T->body_palm;
  return T->body_obj;
}
__device__ __forceinline__ int chain_dof(const GmTopo* T, int c, int p) {
  if (c < 3) return T->dof_f0[c] + p - 1;
  if (c == 3) return T->dof_palm;
  return T->dof_obj + p;   // object uses positions 0..5
}

// Segmented-scan shuffles inside a 16-lane DPP row (chains live on the scan lanes of
// GmTopo::lane_body): row_shr / row_shl by a compile-time distance, 0 shifted in at the
// row edge.  A VALU op with a DPP modifier, no LDS round trip (ds_bpermute).
template <int CTRL>
__device__ __forceinline__ real dpp_move(real x) {
  const long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// value from the lane `off` positions lower in the row (off in 1, 2, 4, 8)
__device__ __forceinline__ real row_shr(real x, int off) {
  switch (off) {
    case 1: return dpp_move<0x111>(x);
    case 2: return dpp_move<0x112>(x);
    case 4: return dpp_move<0x114>(x);
    default: return dpp_move<0x118>(x);
  }
}
// value from the lane `off` positions higher in the row
__device__ __forceinline__ real row_shl(real x, int off) {
  switch (off) {
    case 1: return dpp_move<0x101>(x);
    case 2: return dpp_move<0x102>(x);
    case 4: return dpp_move<0x104>(x);
    default: return dpp_move<0x108>(x);
  }
}
// row_newbcast is the one DPP control the 64-bit data path takes (gfx90a+ DP-ALU DPP):
// one v_mov_b64_dpp instead of two 32-bit halves
template <int CTRL>
__device__ __forceinline__ real dpp_bcast64(real x) {
  return __builtin_amdgcn_update_dpp(0.0, x, CTRL, 0xF, 0xF, true);
}
// value of position k of this lane's 16-lane DPP row (row_newbcast:k), k compile-time
// after unrolling
__device__ __forceinline__ real row_bcast(real x, int k) {
  switch (k) {
    case 0: return dpp_bcast64<0x150>(x);
    case 1: return dpp_bcast64<0x151>(x);
    case 2: return dpp_bcast64<0x152>(x);
    case 3: return dpp_bcast64<0x153>(x);
    case 4: return dpp_bcast64<0x154>(x);
    case 5: return dpp_bcast64<0x155>(x);
    case 6: return dpp_bcast64<0x156>(x);
    case 7: return dpp_bcast64<0x157>(x);
    case 8: return dpp_bcast64<0x158>(x);
    case 9: return dpp_bcast64<0x159>(x);
    case 10: return dpp_bcast64<0x15A>(x);
    case 11: return dpp_bcast64<0x15B>(x);
    case 12: return dpp_bcast64<0x15C>(x);
    case 13: return dpp_bcast64<0x15D>(x);
    case 14: return dpp_bcast64<0x15E>(x);
    default: return dpp_bcast64<0x15F>(x);
  }
}
__device__ __forceinline__ real readlane_real(real x, int l) {
  const long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readlane((int)b, l);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// The physics substep (kinematics .. integrate, the collider and the constraint solver)
// is compiled with FMA contraction: its dot products and small matrix products issue as
// fused multiply-adds (fewer fp64 instructions and shorter dependent chains, -11 % kernel
// time).  The oracle evaluates the same expressions unfused, so device and oracle physics
// agree to ~1e-12 per substep instead of bit for bit (tests/test_grasp_parity.py bounds);
// everything outside the namespace -- stepper, sensors, events, observations, resets and
// spawns -- keeps contraction off and stays bit-exact.  The calibration build (gm_calib.hip)
// keeps it off too: its timestep search compares stability verdicts at the edge of
// stability, candidate for candidate with the oracle.
// Each physics stage header opens and closes the mode and the namespace together (the third
// GM_CAL_TU selection), so none depends on what the header included before it left behind.
#ifdef GM_CAL_TU
#define GM_PHYSICS_BEGIN _Pragma("clang fp contract(off)") namespace gmf {
#else
#define GM_PHYSICS_BEGIN _Pragma("clang fp contract(fast)") namespace gmf {
#endif
#define GM_PHYSICS_END } _Pragma("clang fp contract(off)")
GM_PHYSICS_BEGIN
#define GM_FP_PHYSICS
#include "gm_fphelpers.inc"
#undef GM_FP_PHYSICS
GM_PHYSICS_END
