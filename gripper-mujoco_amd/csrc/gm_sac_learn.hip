// gm_sac_learn.hip -- the SAC learner's kernels: the gradient of compute_loss_q with respect to
// both critics (gm_sac_grad_q_kernel: the two critics of a tile as two workgroups side by side)
// and the gradient of compute_loss_pi with respect to the actor, differentiated through the
// frozen critics into the action and on through tanh and the reparameterised sample into the
// actor's [mu | log_std] head (gm_sac_grad_pi_kernel).  One wave per 16 rows; the tile's forward
// and backward are gm_learn.hip's gl_layers_rows / gl_forward_rows / gl_backward_rows with the
// handle's activation as a literal (the template argument), the way down a frozen critic is its
// gl_delta_prev alone; the sampler is gm_sac_net.h's gs_sample.  The sum over tiles, both
// optimiser steps and the polyak update are gm_learn.hip's gm_learn_step_kernel on ranges of the
// blob.  gm_sac_learn.h has the launch arguments and the row layout.
#pragma once
#include "gm_learn.hip"
#include "gm_sac.hip"
#include "gm_sac_learn.h"

// rows e0 .. e0 + 15 of cat(state, action) straight into the plan's input rows (gs_q_rows' rule:
// zero beyond n and beyond the input width); a barrier must follow
__device__ __forceinline__ void gsl_q_rows(const float* __restrict__ state, const float* __restrict__ action, int e0,
                                           int n, int n_obs, int n_act, int k0, float* A0, int S0, int lane) {
  for (int i = lane; i < GP_TILE * k0; i += 64) {
    const int r = i / k0, k = i - r * k0;
    float v = 0.0f;
    if (e0 + r < n) {
      if (k < n_obs) v = state[(size_t)(e0 + r) * n_obs + k];
      else if (k < n_obs + n_act) v = action[(size_t)(e0 + r) * n_act + (k - n_obs)];
    }
    A0[r * S0 + k] = v;
  }
}

// The gradient of mean((q_j(state, action) - y)^2) with respect to critic j's packed weights for
// tile blockIdx.x and critic j = blockIdx.y: into partials[tile][j's half of [q1 | q2]] (every
// entry written, padding entries with 0), the tile's sum of squares into tile_loss[j][tile].
template <int ACT>
__global__ __launch_bounds__(64) void gm_sac_grad_q_kernel(GslQArgs a) {
  __shared__ float arena[GL_ARENA];
  __shared__ float row_loss[GP_TILE];
  const int lane = threadIdx.x;
  const int tile = blockIdx.x, j = blockIdx.y;
  const int e0 = tile * GP_TILE;
  const GpNet& P = a.net.q;
  const GlPlan& L = a.plan;
  float* base = L.total <= GL_ARENA ? arena : a.spill + ((size_t)tile * 2 + j) * (size_t)L.total;
  const float* __restrict__ params = a.params + (j == 0 ? a.net.q1_off : a.net.q2_off);
  float* part = a.partials + (size_t)tile * 2 * (size_t)a.q_total + (size_t)j * (size_t)a.q_total;

  gsl_q_rows(a.state, a.action, e0, a.n, a.net.pi.width[0], a.net.n_act, P.kpad[0], base + L.a_off[0], L.a_stride[0], lane);
  __syncthreads();
  gl_layers_rows(params, P, L, base, ACT, lane);

  // ---- loss and the delta of the critic's output: one lane per row
  const int nl = P.n_layers;
  if (lane < GP_TILE) {
    float* drow = base + L.d_off[0] + lane * L.d_stride;
    const int wd = P.tiles[nl - 1] * 16;
    float ls = 0.0f, dq = 0.0f;
    if (e0 + lane < a.n) {
      const float d = base[L.a_off[nl] + lane * L.a_stride[nl]] - a.y[e0 + lane];
      ls = d * d;
      dq = 2.0f * d / (float)a.n;
    }
    drow[0] = dq;
    for (int c = 1; c < wd; c++) drow[c] = 0.0f;
    row_loss[lane] = ls;
  }
  __syncthreads();
  if (lane == 0) {
    float s = 0.0f;
    for (int r = 0; r < GP_TILE; r++) s += row_loss[r];
    a.tile_loss[j * GL_MAX_TILES + tile] = s;
  }
  gl_backward_rows(params, P, L, base, part, ACT, false, lane);
}

// The standard normal draw of action i of batch row gid at `decision`: gs_sample's four lines,
// repeated here and not factored out of it (gs_sample is compiled into the rollout's step kernels,
// whose registers a shared inline would have to leave alone), for the debug output z only -- u, a
// and logp are gs_sample's own.
__device__ __forceinline__ float gsl_draw_z(uint64_t seed, uint64_t decision, uint64_t gid, int i) {
  const uint64_t h = gp_mix(seed ^ gp_mix(gid * 0x100000001B3ull + decision));
  const uint64_t c1 = gp_mix(h + 3ull * (uint64_t)i + 1ull), c2 = gp_mix(h + 3ull * (uint64_t)i + 2ull);
  const float u1 = (float)((double)((c1 >> 40) + 1ull) * (1.0 / 16777216.0));
  const float u2 = (float)((double)(c2 >> 40) * (1.0 / 16777216.0));
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// A frozen critic's delta with respect to its action inputs, from the deltas of its output in the
// plan's delta rows 0: down the layers with gl_delta_prev alone (no dW, no db), and at layer 0 the
// same product without an activation derivative (the input is no activation's output) for the
// column blocks that hold the action columns n_obs .. n_obs + n_act - 1 only:
//   ga[i][c] (+)= sum_j D0[i][j] W0[j][n_obs + c]
// `add`: added to what ga holds (each entry is read and written by the same lane every time).
template <int ACT>
__device__ __forceinline__ void gsl_action_delta(const float* __restrict__ params, const GpNet& P, const GlPlan& L,
                                                 float* base, int n_obs, int n_act, float (*ga)[GA_MAX_ACT], bool add,
                                                 int lane) {
  const int Sd = L.d_stride;
  int cur = 0;
  for (int l = P.n_layers - 1; l >= 1; l--) {
    const float* A = base + L.a_off[l];
    const int Sa = L.a_stride[l];
    float* Dn = base + L.d_off[cur ^ 1];
    gl_delta_prev(params + P.woff[l], P.kpad[l], (P.width[l + 1] + 3) & ~3, base + L.d_off[cur], Sd, 0,
                  P.tiles[l - 1] * 16, lane,
                  [&](int i, int k, float c) { Dn[i * Sd + k] = gl_act_grad(c, A[i * Sa + k], ACT); });
    __syncthreads();
    cur ^= 1;
  }
  gl_delta_prev(params + P.woff[0], P.kpad[0], (P.width[1] + 3) & ~3, base + L.d_off[cur], Sd, n_obs & ~15,
                (n_obs + n_act + 15) & ~15, lane, [&](int i, int k, float c) {
                  if (k >= n_obs && k < n_obs + n_act) ga[i][k - n_obs] = add ? ga[i][k - n_obs] + c : c;
                });
  __syncthreads();
}

// The gradient of mean(alpha logp_pi - min(q1, q2)(state, pi(state))) with respect to the actor's
// packed weights for tile blockIdx.x, into partials[tile][pi's packed count], and the tile's loss
// sum into tile_loss[tile].  Per row, with t = tanh(u), a = limit t, u = mu + exp(ls) z and
// g_a = d(-min q)/da (the selected critic's input delta from an output delta of -1/n; a tie goes
// to q1):
//   d_u  = g_a limit (1 - t^2) + (alpha / n) 2 t          (d(-corr)/du = 2 tanh u)
//   d_mu = d_u
//   d_ls = d_u (u - mu) - alpha / n, 0 where the raw log_std lies outside [ls_min, ls_max]
// (the Normal term is -z^2 / 2 - ls - const in terms of z: it does not depend on mu, and on ls
// only through -ls).
template <int ACT>
__global__ __launch_bounds__(64) void gm_sac_grad_pi_kernel(GslPiArgs a) {
  __shared__ float arena[GL_ARENA];
  __shared__ float ga[GP_TILE][GA_MAX_ACT];
  __shared__ float row_loss[GP_TILE];
  const int lane = threadIdx.x;
  const int tile = blockIdx.x;
  const int e0 = tile * GP_TILE;
  const int n = a.n;
  const GpNet& P = a.net.pi;
  const GpNet& Q = a.net.q;
  const GlPlan& Lp = a.plan_pi;
  const GlPlan& Lq = a.plan_q;
  const long long rows = gsl_pi_rows(Lp, Lq);
  float* base = rows <= GL_ARENA ? arena : a.spill + (size_t)tile * (size_t)rows;
  float* bq[2] = {base + Lp.total, base + Lp.total + Lq.total};
  const int na = a.net.n_act, n_obs = P.width[0];
  const int nl = P.n_layers, nlq = Q.n_layers;
  const bool mine = lane < GP_TILE && e0 + lane < n;
  const float inv_n = 1.0f / (float)n;

  // 1. the actor's forward, its rows kept
  gl_forward_rows(a.state, (size_t)e0, (size_t)n, a.params, P, Lp, base, ACT, lane);

  // 2. one lane per row: sample, squash and logp; the action goes straight into q1's input row,
  //    u into the actor's delta rows 1 (free until its backward)
  const float* head = base + Lp.a_off[nl] + (lane & 15) * Lp.a_stride[nl];
  float* urow = base + Lp.d_off[1] + (lane & 15) * Lp.d_stride;
  const int S0 = Lq.a_stride[0];
  float logp = 0.0f;
  if (lane < GP_TILE) {
    float* arow = bq[0] + Lq.a_off[0] + lane * S0 + n_obs;
    if (mine) {
      const size_t row = (size_t)(e0 + lane);
      logp = gs_sample(head, na, GM_SAC_SAMPLE, a.net.limit, a.net.ls_min, a.net.ls_max, a.seed, a.draw, (uint64_t)row,
                       arow, urow, nullptr);
      if (a.logp) a.logp[row] = logp;
      for (int i = 0; i < na; i++) {
        if (a.z) a.z[row * na + i] = gsl_draw_z(a.seed, a.draw, (uint64_t)row, i);
        if (a.u) a.u[row * na + i] = urow[i];
        if (a.a) a.a[row * na + i] = arow[i];
      }
    } else {
      for (int i = 0; i < na; i++) arow[i] = 0.0f;
    }
  }
  __syncthreads();
  // the critics' input rows [state | a]: the state from the actor's input rows, a from q1's row
  {
    const int k0 = Q.kpad[0];
    const float* As = base + Lp.a_off[0];
    float* A1 = bq[0] + Lq.a_off[0];
    float* A2 = bq[1] + Lq.a_off[0];
    for (int i = lane; i < GP_TILE * k0; i += 64) {
      const int r = i / k0, k = i - r * k0;
      const float v = k < n_obs ? As[r * Lp.a_stride[0] + k] : (k < n_obs + na ? A1[r * S0 + k] : 0.0f);
      A1[r * S0 + k] = v;
      A2[r * S0 + k] = v;
    }
  }
  __syncthreads();

  // 3. both critics' forwards, rows kept
  gl_layers_rows(a.params + a.net.q1_off, Q, Lq, bq[0], ACT, lane);
  gl_layers_rows(a.params + a.net.q2_off, Q, Lq, bq[1], ACT, lane);

  // 4. the min select, the loss and the critics' output deltas
  if (lane < GP_TILE) {
    const float v1 = bq[0][Lq.a_off[nlq] + lane * Lq.a_stride[nlq]];
    const float v2 = bq[1][Lq.a_off[nlq] + lane * Lq.a_stride[nlq]];
    const bool first = v1 <= v2;
    const int wd = Q.tiles[nlq - 1] * 16;
    float* d1 = bq[0] + Lq.d_off[0] + lane * Lq.d_stride;
    float* d2 = bq[1] + Lq.d_off[0] + lane * Lq.d_stride;
    d1[0] = mine && first ? -inv_n : 0.0f;
    d2[0] = mine && !first ? -inv_n : 0.0f;
    for (int c = 1; c < wd; c++) d1[c] = d2[c] = 0.0f;
    row_loss[lane] = mine ? a.alpha * logp - (first ? v1 : v2) : 0.0f;
    if (mine) {
      if (a.q1) a.q1[e0 + lane] = v1;
      if (a.q2) a.q2[e0 + lane] = v2;
    }
  }
  __syncthreads();
  if (lane == 0) {
    float s = 0.0f;
    for (int r = 0; r < GP_TILE; r++) s += row_loss[r];
    a.tile_loss[tile] = s;
  }

  // 5. the critics' input deltas on the action columns
  gsl_action_delta<ACT>(a.params + a.net.q1_off, Q, Lq, bq[0], n_obs, na, ga, false, lane);
  gsl_action_delta<ACT>(a.params + a.net.q2_off, Q, Lq, bq[1], n_obs, na, ga, true, lane);

  // 6. the head deltas [d_mu | d_ls] into the actor's delta rows 0
  if (lane < GP_TILE) {
    float* drow = base + Lp.d_off[0] + lane * Lp.d_stride;
    const int wd = P.tiles[nl - 1] * 16;
    const float an = a.alpha * inv_n;
    if (mine) {
      for (int i = 0; i < na; i++) {
        const float ui = urow[i];
        const float t = tanhf(ui);
        const float du = ga[lane][i] * a.net.limit * (1.0f - t * t) + an * (2.0f * t);
        const float raw = head[na + i];
        drow[i] = du;
        drow[na + i] = (raw >= a.net.ls_min && raw <= a.net.ls_max) ? du * (ui - head[i]) - an : 0.0f;
      }
      for (int c = 2 * na; c < wd; c++) drow[c] = 0.0f;
    } else {
      for (int c = 0; c < wd; c++) drow[c] = 0.0f;
    }
  }
  __syncthreads();

  // 7. the actor's backward
  gl_backward_rows(a.params, P, Lp, base, a.partials + (size_t)tile * (size_t)a.pi_total, ACT, false, lane);
}
