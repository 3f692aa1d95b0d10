// gm_arrow.h -- what the two arrow-matrix solves of the substep share: the Newton point's
// H~ + J_a^T D_a J_a (gm_newton_point.h) and mj_Euler's M + h D (gm_euler.h).  The arrow matrix
// is the finger-chain blocks, each on its 16-lane DPP row (chain position p = 1..CL on lane
// 16 f + p, factored leaf first), the palm's single pivot on lane 56, and a border every block
// couples to: [base, object 0..5] on lanes 48..54 for the Newton point, the base alone (held
// wave-uniformly) for the Euler solve.  Here are the lane roles, the substitutions along a
// chain, the sum over the DPP rows and the border's sums over the chain pivots' transfers; each
// solve keeps its own pivot loop (Newton selects the pivot column from broadcasts, Euler takes
// it from the lane's own full row: different operations).  gm_euler.h reads its lane roles from
// FactorLane; the Newton point still spells them out where it uses them, because its code
// objects change when it takes them from a value (profiles/newton_stages_code_identity.txt).

// SharedT: reads the union's fs.lbub (border_transfer_sums).
#pragma once
#include "gm_real.h"

GM_PHYSICS_BEGIN
#define GM_LANE_PALM_F 56

// A lane's role in the factor layout: its DPP row and position, the border row's index, and
// whether it holds a finger chain's row, the palm's or a border row
struct FactorLane {
  int rowf, p, bi;
  bool chainrow, palm, border;
};
template <int CL>
__device__ __forceinline__ FactorLane factor_lane(int lane) {
  const int rowf = lane >> 4, p = lane & 15;
  return {rowf, p, lane - 48, rowf < 3 && p >= 1 && p <= CL, lane == GM_LANE_PALM_F, lane >= 48 && lane < 55};
}

// forward substitution along a finger chain, leaf first: L[k] is the lane's multiplier of
// pivot k (row_newbcast hands every lane of the row pivot k's y)
template <int CL>
__device__ __forceinline__ real chain_forward(real y, const real* L, int p) {
#pragma unroll
  for (int k = CL; k >= 1; k--) {
    const real yk = row_bcast(y, k);
    const real Lc = (p >= 1 && p < k) ? L[k] : 0.0;
    y = y - Lc * yk;
  }
  return y;
}
// back substitution along a finger chain, root -> leaf: L[j] (j < p) is the lane's row of L^T
template <int CL>
__device__ __forceinline__ real chain_backward(real y, const real* L, int p) {
#pragma unroll
  for (int j = 1; j < CL; j++) {
    const real xj = row_bcast(y, j);
    const real Lr = (j < p) ? L[j] : 0.0;
    y = y - Lr * xj;
  }
  return y;
}

// The sum of s over the factor lanes, wave-uniform: per DPP row an inclusive scan (lane 15 of
// the row holds the row total; lanes outside the chains hold zeros), then rows 0, 1, 2 and the
// palm read back as scalars and added in that order
__device__ __forceinline__ real row_totals(real s) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) {
    const real t = row_shr(s, off);
    s += t;
  }
  return ((readlane_real(s, 15) + readlane_real(s, 31)) + readlane_real(s, 47)) + readlane_real(s, GM_LANE_PALM_F);
}

// Border entry i's sums over the chain pivots' transfers: acc[f] = sum over k = CL .. 1 of
// lbub[f][k - 1][i] * second(f, k - 1), one partial sum per finger chain (three independent
// dependent-chains of CL terms), four pivots' transfers per batch of loads
template <int CL, class Second>
__device__ __forceinline__ void border_transfer_sums(const SharedT<CL>& S, int i, Second second, real (&acc)[3]) {
#pragma unroll
  for (int f = 0; f < 3; f++) acc[f] = 0.0;
#pragma unroll
  for (int k0 = CL; k0 >= 1; k0 -= 4) {
    real lv[24];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int f = 0; f < 3; f++) {
        const int k = (k0 - q >= 1) ? k0 - q : 1;
        lv[6 * q + 2 * f] = S.fs.lbub[f][k - 1][i];
        lv[6 * q + 2 * f + 1] = second(f, k - 1);
      }
    keep_n<24>(lv);
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int f = 0; f < 3; f++)
        if (k0 - q >= 1) acc[f] = acc[f] + lv[6 * q + 2 * f] * lv[6 * q + 2 * f + 1];
  }
}
GM_PHYSICS_END
