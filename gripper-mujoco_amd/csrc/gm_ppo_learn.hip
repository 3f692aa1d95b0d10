// gm_ppo_learn.hip -- the PPO learner's kernels: the gradients of compute_loss_pi and
// compute_loss_v over a batch (gm_ppo_grad_pi_kernel, its categorical twin
// gm_ppo_grad_pi_cat_kernel and gm_ppo_grad_vf_kernel: one wave per
// workgroup, G workgroups, each over its own tiles of 16 rows), the kernel that sums the G
// partial gradients in order, forms the losses and info scalars and latches the KL stop
// (gm_ppo_reduce_kernel), and PPOBuffer.get's advantage normalisation
// (gm_ac_adv_normalise_kernel).  The tile's forward and backward are gm_learn.hip's
// gl_forward_rows / gl_backward_rows, called with tanh as a literal; the optimiser step is
// gm_learn.hip's gm_learn_step_kernel.  gm_ppo_learn.h has the tile-to-workgroup map.
#pragma once
#include "gm_learn.hip"
#include "gm_ppo_learn.h"

// One workgroup's tiles of one net.  POLICY: per row i (one lane per row)
//   logp = sum_a -(act - mu)^2 / (2 sigma^2) - log_std_a - 1/2 log 2 pi      (ga_sample's order)
//   r = exp(logp - logp_old)
//   clip:  loss_i = -min(r A, clamp(r, 1 - eps, 1 + eps) A),
//          dL/dlogp = -A r / n, 0 where (r > 1 + eps and A > 0) or (r < 1 - eps and A < 0)
//   KL:    loss = -mean(r A) + beta mean(logp_old - logp),  dL/dlogp = -(A r + beta) / n
//   dL/dmu_a = dL/dlogp (act_a - mu_a) / sigma_a^2           the deltas of the actor's outputs
//   dL/dlog_std_a += dL/dlogp ((act_a - mu_a)^2 / sigma_a^2 - 1)   summed over the rows in row order
// else the critic: loss_i = (v - ret)^2, delta = 2 (v - ret) / n.
// GQ_CAT, the categorical policy: the outputs x_j are logits and act[row][0] the taken index a
// (clamped into the row).  In ga_sample_cat's order
//   m = max_j x_j, e_j = expf(x_j - m), s = sum_j e_j, lse = m + logf(s), logp_j = x_j - lse
//   logp = logp_a;  r, loss_i, dL/dlogp, kl and cf exactly as above
//   p_j = e_j / s,  H = -sum_j p_j logp_j     (a class with e_j == 0 adds exactly 0)
//   delta_j = dL/dlogp ([j == a] - p_j)  + (c_ent / n) p_j (logp_j + H) with entropy regularisation
// (d(-c_ent mean H)/dx_j; the reduce kernel takes ent = mean H from the fourth row sum).
template <int MODE>
__device__ __forceinline__ void gq_grad(const GqGradArgs& a) {
  constexpr bool POLICY = MODE == GQ_PI;
  constexpr int N_INFO = MODE == GQ_CAT ? 4 : MODE == GQ_PI ? 3 : 1;
  extern __shared__ float arena[];               // the plan's rows when they fit GL_ARENA (then the partial, lds_part)
  __shared__ float row_info[MODE == GQ_CAT ? 4 : 3][GP_TILE];   // per row: loss, logp_old - logp, clipped, (GQ_CAT) entropy
  if (a.stop && *a.stop) return;                 // (uniform) the KL stop has latched
  const int lane = threadIdx.x;
  const GpNet& P = a.net;
  const GlPlan& L = a.plan;
  const size_t n = (size_t)a.n;
  const size_t tiles = (n + GP_TILE - 1) / GP_TILE;
  float* base = L.total <= GL_ARENA ? arena : a.spill + (size_t)blockIdx.x * (size_t)a.spill_stride;
  // the running sum of this workgroup's tiles: in LDS behind the rows where the packed net fits
  // there (written out once at the end), else in place in partials[g]
  float* gpart = a.partials + (size_t)blockIdx.x * (size_t)a.total;
  float* part = a.lds_part ? arena + L.total : gpart + a.net_off;
  const float* __restrict__ params = a.params + a.net_off;
  const float* __restrict__ log_std = a.params + a.log_std_off;
  const int nl = P.n_layers;
  const int n_out = P.width[nl];
  const int Sd = L.d_stride;
  const int wd = P.tiles[nl - 1] * 16;
  float sums[4] = {0.0f, 0.0f, 0.0f, 0.0f};      // lane 0: this workgroup's loss, kl, clipped and entropy sums
  bool add = false;
  for (size_t tile = blockIdx.x; tile < tiles; tile += (size_t)a.n_groups) {
    const size_t e0 = tile * GP_TILE;
    gl_forward_rows(a.obs, e0, n, params, P, L, base, GP_ACT_TANH, lane);

    // ---- loss and the deltas of the outputs: one lane per row
    if (lane < GP_TILE) {
      const size_t row = e0 + (size_t)lane;
      float* drow = base + L.d_off[0] + lane * Sd;
      float* srow = base + L.d_off[1] + lane * Sd;    // (policy) the row's log_std gradient terms
      const float* out = base + L.a_off[nl] + lane * L.a_stride[nl];
      float ls = 0.0f, kl = 0.0f, cf = 0.0f, en = 0.0f;
      if (row < n) {
        if (MODE == GQ_CAT) {
          float m = out[0];
          for (int j = 1; j < n_out; j++)
            if (out[j] > m) m = out[j];
          float s = 0.0f;
          for (int j = 0; j < n_out; j++) {
            const float e = expf(out[j] - m);
            srow[j] = e;                         // (the row the Gaussian keeps its log_std terms in)
            s += e;
          }
          const float lse = m + logf(s);
          int ai = (int)a.act[row];
          ai = ai < 0 ? 0 : (ai >= n_out ? n_out - 1 : ai);
          const float logp = out[ai] - lse;
          const float lold = a.logp_old[row], A = a.adv[row];
          const float r = expf(logp - lold);
          float dl;
          if (a.use_kl) {
            ls = -(r * A);
            dl = -(A * r + a.beta) / (float)n;
          } else {
            ls = -fminf(r * A, fminf(fmaxf(r, a.clip_lo), a.clip_hi) * A);
            const bool flat = (r > a.clip_hi && A > 0.0f) || (r < a.clip_lo && A < 0.0f);
            dl = flat ? 0.0f : -(A * r) / (float)n;
          }
          kl = lold - logp;
          cf = (r > a.clip_hi || r < a.clip_lo) ? 1.0f : 0.0f;
          float hs = 0.0f;
          for (int j = 0; j < n_out; j++) hs += (srow[j] / s) * (out[j] - lse);
          en = -hs;
          const float ce = a.c_ent / (float)n;
          for (int j = 0; j < n_out; j++) {
            const float p = srow[j] / s;
            float d = dl * ((j == ai ? 1.0f : 0.0f) - p);
            if (a.use_ent) d = d + ce * (p * ((out[j] - lse) + en));
            drow[j] = d;
          }
        } else if (POLICY) {
          const float* ac = a.act + row * (size_t)n_out;
          float logp = 0.0f;
          for (int i = 0; i < n_out; i++) {
            const float lsd = log_std[i];
            const float sd = expf(lsd);
            const float d = ac[i] - out[i];
            logp += -(d * d) / (2.0f * (sd * sd)) - lsd - 0.91893853320467274178f;
          }
          const float lold = a.logp_old[row], A = a.adv[row];
          const float r = expf(logp - lold);
          float dl;
          if (a.use_kl) {
            ls = -(r * A);
            dl = -(A * r + a.beta) / (float)n;
          } else {
            ls = -fminf(r * A, fminf(fmaxf(r, a.clip_lo), a.clip_hi) * A);
            const bool flat = (r > a.clip_hi && A > 0.0f) || (r < a.clip_lo && A < 0.0f);
            dl = flat ? 0.0f : -(A * r) / (float)n;
          }
          kl = lold - logp;
          cf = (r > a.clip_hi || r < a.clip_lo) ? 1.0f : 0.0f;
          for (int i = 0; i < n_out; i++) {
            const float sd = expf(log_std[i]);
            const float s2 = sd * sd;
            const float d = ac[i] - out[i];
            drow[i] = dl * (d / s2);
            srow[i] = dl * ((d * d) / s2 - 1.0f);
          }
        } else {
          const float d = out[0] - a.ret[row];
          ls = d * d;
          drow[0] = 2.0f * d / (float)n;
        }
        for (int j = n_out; j < wd; j++) drow[j] = 0.0f;
      } else {
        for (int j = 0; j < wd; j++) drow[j] = 0.0f;
        if (POLICY)
          for (int i = 0; i < n_out; i++) srow[i] = 0.0f;
      }
      row_info[0][lane] = ls;
      row_info[1][lane] = kl;
      row_info[2][lane] = cf;
      if (MODE == GQ_CAT) row_info[3][lane] = en;
    }
    __syncthreads();
    if (lane == 0)
      for (int q = 0; q < N_INFO; q++) {
        float s = 0.0f;
        for (int r = 0; r < GP_TILE; r++) s += row_info[q][r];
        sums[q] += s;
      }
    if (POLICY && lane < n_out) {
      const float* S = base + L.d_off[1];
      float s = 0.0f;
      for (int r = 0; r < GP_TILE; r++) s += S[r * Sd + lane];
      float* q = gpart + a.log_std_off + lane;
      *q = add ? *q + s : s;
    }
    __syncthreads();                             // the log_std terms are read before the backward reuses their rows

    gl_backward_rows(params, P, L, base, part, GP_ACT_TANH, add, lane);
    add = true;
    __syncthreads();                             // the rows are read before the next tile's forward writes them
  }
  if (a.lds_part && (size_t)blockIdx.x < tiles)
    for (long long i = lane; i < a.net_total; i += 64) gpart[a.net_off + i] = part[i];
  if (lane == 0 && (size_t)blockIdx.x < tiles) {
    float* w = a.wg_info + (size_t)blockIdx.x * GQ_INFO;
    w[0] = sums[0];
    w[1] = sums[1];
    w[2] = sums[2];
    if (MODE == GQ_CAT) w[3] = sums[3];
  }
}

__global__ __launch_bounds__(64) void gm_ppo_grad_pi_kernel(GqGradArgs a) { gq_grad<GQ_PI>(a); }
__global__ __launch_bounds__(64) void gm_ppo_grad_pi_cat_kernel(GqGradArgs a) { gq_grad<GQ_CAT>(a); }
__global__ __launch_bounds__(64) void gm_ppo_grad_vf_kernel(GqGradArgs a) { gq_grad<GQ_VF>(a); }

// grad = the sum of the workgroups' partials in workgroup order, for one optimiser's elements;
// with entropy regularisation -c_ent / n_act more on every log_std element (the entropy of Normal
// is 1/2 + 1/2 log 2 pi + log_std, averaged over all [n][n_act] elements).  Thread 0: the mean
// loss, kl = mean(logp_old - logp), ent, cf = clipped rows / n, and the KL stop: the reference
// tests kl at the top of every policy iteration and breaks before backward, so the latch is set
// by the first iteration whose kl exceeds kl_stop and no later one counts or steps (their
// gradient launches exit at once, so this kernel re-adds the same partials to the same bytes).
__global__ __launch_bounds__(256) void gm_ppo_reduce_kernel(GqReduceArgs a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.count) return;
  const long long e = a.first + i + (i >= a.gap_at ? a.gap_len : 0);
  float g = 0.0f;
  for (int p = 0; p < a.n_parts; p++) g += a.partials[(size_t)p * (size_t)a.total + (size_t)e];
  if (a.policy && a.use_ent && !a.categorical && e >= a.log_std_off) g = g - a.c_ent / (float)a.n_act;
  a.grad[e] = g;
  if (i != 0) return;
  float s[3] = {0.0f, 0.0f, 0.0f};
  for (int p = 0; p < a.n_parts; p++)
    for (int q = 0; q < 3; q++) s[q] += a.wg_info[(size_t)p * GQ_INFO + q];
  const float nf = (float)a.n;
  if (!a.policy) {
    const float loss = s[0] / nf;
    a.scalars[GQ_LOSS_V] = loss;
    if (a.first_out) a.first_out[GQ_LOSS_V] = loss;
    if (a.last_out) a.last_out[GQ_LOSS_V] = loss;
    return;
  }
  const float kl = s[1] / nf;
  float ent = 0.0f;
  if (a.categorical) {   // the mean of the rows' entropies, summed like the other three
    for (int p = 0; p < a.n_parts; p++) ent += a.wg_info[(size_t)p * GQ_INFO + 3];
    ent = ent / nf;
  } else {
    for (int j = 0; j < a.n_act; j++) ent += 1.41893853320467274178f + a.params[a.log_std_off + j];
    ent = ent / (float)a.n_act;
  }
  float loss = s[0] / nf;
  if (a.use_kl) loss = loss + a.beta * kl;
  if (a.use_ent) loss = loss - a.c_ent * ent;
  const float v[GQ_SCALARS] = {loss, 0.0f, kl, ent, s[2] / nf};
  for (int q = 0; q < GQ_SCALARS; q++)
    if (q != GQ_LOSS_V) {
      a.scalars[q] = v[q];
      if (a.first_out) a.first_out[q] = v[q];
      if (a.last_out) a.last_out[q] = v[q];
    }
  if (a.stop && a.stop[0] == 0) {
    if ((double)kl > a.kl_stop) a.stop[0] = 1;
    else a.stop[1] += 1;
  }
}

// adv <- (adv - mean) / std with the unbiased standard deviation (torch.std_mean, PPOBuffer.get).
// One workgroup: thread t sums elements t, t + 1024, ... in double, the 1024 sums are added by a
// tree of fixed shape, first for the mean and then for the squared deviations from it, so the
// result does not depend on timing.  mean and std are rounded to f32 where they meet the tensor.
__global__ __launch_bounds__(1024) void gm_ac_adv_normalise_kernel(float* __restrict__ adv, long long n) {
  __shared__ double red[1024];
  const int t = threadIdx.x;
  double mean = 0.0;
  for (int pass = 0; pass < 2; pass++) {
    double s = 0.0;
    for (size_t i = (size_t)t; i < (size_t)n; i += 1024) {
      const double d = (double)adv[i] - mean;
      s += pass == 0 ? d : d * d;
    }
    red[t] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
      if (t < w) red[t] += red[t + w];
      __syncthreads();
    }
    const double total = red[0];
    __syncthreads();
    if (pass == 0) {
      mean = total / (double)n;
    } else {
      const float mf = (float)mean, sf = (float)sqrt(total / (double)(n - 1));
      for (size_t i = (size_t)t; i < (size_t)n; i += 1024) adv[i] = (adv[i] - mf) / sf;
    }
  }
}
