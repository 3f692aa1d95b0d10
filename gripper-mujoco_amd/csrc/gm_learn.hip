// gm_learn.hip -- the DQN learner's kernels: the loss gradient of a batch (gm_learn_grad_kernel,
// one wave per 16 rows, partial sums per tile) and the elementwise kernel that sums the tiles in
// order, steps Adam / AdamW and soft-updates a target net (gm_learn_step_kernel).  Shared rules
// and the row plan are gm_learn.h's; the forward is gm_policy_net.h's chain, kept layer by layer.
// The layer-wise forward and backward of one tile (gl_forward_rows, gl_backward_rows) and the step
// kernel are also the PPO learner's (gm_ppo_learn.hip), which passes tanh where this file passes ReLU,
// and the SAC learner's (gm_sac_learn.hip), which also walks gl_delta_prev alone down its frozen critics.
//
// Kernels are ordered by the context's stream and, inside a kernel, by workgroup barriers only:
// no workgroup waits for another one, and no float atomic is used, so two runs give the same bits.
#pragma once
#include "gm_learn.h"

#define GL_AHEAD 8   // k steps whose operands gl_forward_rows / gl_backward_rows load ahead of the MFMA chain

// The layers of gl_forward_rows on input rows already under the plan (a[0]: [16][kpad[0]], 0 where
// a row or a column is padding, written before a barrier): the only MFMA loop of the learners'
// forwards.  The SAC learner (gm_sac_learn.hip) assembles [state | action] rows there itself.
__device__ __forceinline__ void gl_layers_rows(const float* __restrict__ params, const GpNet& P, const GlPlan& L,
                                               float* base, int code, int lane) {
  const int g = lane >> 4, nn = lane & 15;
  for (int l = 0; l < P.n_layers; l++) {
    const float* __restrict__ W = params + P.woff[l];
    const float* __restrict__ Bv = params + P.boff[l];
    const int ksteps = P.kpad[l] >> 2;
    const bool last = (l == P.n_layers - 1);
    const int outw = P.width[l + 1];
    const float* in = base + L.a_off[l];
    float* out = base + L.a_off[l + 1];
    const int Si = L.a_stride[l], So = L.a_stride[l + 1];
    for (int t = 0; t < P.tiles[l]; t++) {
      gp_f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
      const float* Wt = W + (size_t)t * ksteps * 64;
      // GL_AHEAD k steps' operands are loaded ahead of their MFMAs (one wait for the loads of W
      // where one per MFMA would serialise the chain on L2's latency); the MFMAs keep their k order
      for (int s0 = 0; s0 < ksteps; s0 += GL_AHEAD) {
        const int m = min(GL_AHEAD, ksteps - s0);
        float a[GL_AHEAD], b[GL_AHEAD];
#pragma unroll
        for (int u = 0; u < GL_AHEAD; u++) {
          a[u] = u < m ? in[nn * Si + 4 * (s0 + u) + g] : 0.0f;
          b[u] = u < m ? Wt[(s0 + u) * 64 + lane] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < GL_AHEAD; u++)
          if (u < m) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], c, 0, 0, 0);
      }
      const int j = t * 16 + nn;
      const float bias = Bv[j];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        float v = c[r] + bias;
        if (!last) v = gp_activate(v, code);
        out[(g * 4 + r) * So + j] = (j < outw) ? v : 0.0f;
      }
    }
    __syncthreads();
  }
}

// One tile's forward with every layer's rows kept: gp_forward_tile's arithmetic (same MFMA chain,
// k order, bias placement; hidden layers through gp_activate(code), a caller's literal) on rows
// e0 .. e0 + 15 of x[n][width 0], the post-activation rows of every layer left under the plan L
// from `base` -- LDS when the plan fits GL_ARENA, else the caller's global spill rows (written
// and read by this wave only, between barriers).  Rows >= n and padded columns are 0.
__device__ __forceinline__ void gl_forward_rows(const float* __restrict__ x, size_t e0, size_t n,
                                                const float* __restrict__ params, const GpNet& P, const GlPlan& L,
                                                float* base, int code, int lane) {
  {
    const int n_obs = P.width[0], k0 = P.kpad[0], S0 = L.a_stride[0];
    float* A0 = base + L.a_off[0];
    for (int i = lane; i < GP_TILE * k0; i += 64) {
      const int r = i / k0, k = i - r * k0;
      A0[r * S0 + k] = (e0 + r < n && k < n_obs) ? x[(e0 + r) * n_obs + k] : 0.0f;
    }
  }
  __syncthreads();
  gl_layers_rows(params, P, L, base, code, lane);
}

// dL/dz of a hidden layer from dL/da (c) and the stored activation a: ReLU's [a > 0], tanh's 1 - a^2
__device__ __forceinline__ float gl_act_grad(float c, float a, int code) {
  return code == GP_ACT_TANH ? c * (1.0f - a * a) : (a > 0.0f ? c : 0.0f);
}

// The product that carries deltas down through a layer's packed weights W ([.][kpad] in B-fragment
// order): store(i, k, sum_j D[i][j] W[j][k]) for the 16 rows i and every k of the 16-wide column
// blocks kb_lo, kb_lo + 16, ... < kb_hi (0 for k >= kpad), j running over [0, jmax) (the deltas of
// padded columns are 0).  MFMA with M = the 16 rows, N = 16 k's, reduction over j in steps of 4, W
// gathered from the B-fragment order (4 consecutive floats per (k, j quad)); lane (g, nn) stores
// rows 4 g .. 4 g + 3 of column kb + nn, the same entries on every call.  gl_backward_rows' step
// between two layers; the SAC learner's way down a frozen critic to its input (gm_sac_learn.hip).
template <class Store>
__device__ __forceinline__ void gl_delta_prev(const float* __restrict__ W, int kpad, int jmax, const float* D, int Sd,
                                              int kb_lo, int kb_hi, int lane, Store store) {
  const int g = lane >> 4, nn = lane & 15;
  const int ksteps = kpad >> 2;
  for (int kb = kb_lo; kb < kb_hi; kb += 16) {
    gp_f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
    const int k = kb + nn;
    for (int q0 = 0; q0 < jmax; q0 += 4 * GL_AHEAD) {     // (operands ahead of their MFMAs, as in the forward)
      const int m = min(GL_AHEAD, (jmax - q0) >> 2);
      float a[GL_AHEAD], b[GL_AHEAD];
#pragma unroll
      for (int u = 0; u < GL_AHEAD; u++) {
        const int j = q0 + 4 * u + g;
        a[u] = u < m ? D[nn * Sd + j] : 0.0f;
        b[u] = (u < m && k < kpad) ? W[((size_t)(j >> 4) * ksteps + (k >> 2)) * 64 + (k & 3) * 16 + (j & 15)] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < GL_AHEAD; u++)
        if (u < m) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], c, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) store(4 * g + r, k, c[r]);
  }
}

// One tile's backward through the layers, from the deltas of the last layer's outputs in the
// plan's delta rows 0 (0 in padded columns and in rows >= n): this tile's share of the gradient
// with respect to the packed weights into part[net's packed count] -- every entry written,
// padding entries with 0; with `add`, added to what part holds (a workgroup's running sum over
// its tiles: each entry is read and written by the same lane every time).  Per layer l from the
// last, with D the deltas dL/dz of layer l's outputs and A the layer's input rows,
//   dW[j][k] = sum_i D[i][j] A[i][k]   MFMA with M = 16 k's of four k steps, N = 16 j's of a tile,
//                                       reduction over the batch rows in four chunks of 4; row m
//                                       of the product stands for k = 4 (s0 + (m & 3)) + (m >> 2),
//                                       so register r of lane (g, n) is packed element
//                                       (tile t, k step s0 + r, lane 16 g + n): coalesced stores;
//   db[j]    = sum_i D[i][j]            in row order;
//   Dprev[i][k] = act'(A[i][k]) sum_j D[i][j] W[j][k]   gl_delta_prev.
__device__ __forceinline__ void gl_backward_rows(const float* __restrict__ params, const GpNet& P, const GlPlan& L,
                                                 float* base, float* __restrict__ part, int code, bool add, int lane) {
  const int g = lane >> 4, nn = lane & 15;
  const int nl = P.n_layers;
  const int Sd = L.d_stride;
  int cur = 0;
  for (int l = nl - 1; l >= 0; l--) {
    const float* __restrict__ W = params + P.woff[l];
    const int kpad = P.kpad[l], ksteps = kpad >> 2;
    const float* A = base + L.a_off[l];
    const int Sa = L.a_stride[l];
    const float* D = base + L.d_off[cur];
    // dW in packed order
    const int km = 4 * (nn & 3) + (nn >> 2);       // the k (within 16) that product row m = nn stands for
    for (int t = 0; t < P.tiles[l]; t++)
      for (int s0 = 0; s0 < ksteps; s0 += 4) {
        gp_f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
        const int k = 4 * s0 + km;
#pragma unroll
        for (int ch = 0; ch < 4; ch++) {
          const int i = 4 * ch + g;
          const float a = k < kpad ? A[i * Sa + k] : 0.0f;
          const float b = D[i * Sd + 16 * t + nn];
          c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
          if (s0 + r < ksteps) {
            float* q = part + P.woff[l] + ((long long)t * ksteps + s0 + r) * 64 + lane;
            *q = add ? *q + c[r] : c[r];
          }
      }
    // db
    for (int j = lane; j < P.tiles[l] * 16; j += 64) {
      float s = 0.0f;
      for (int i = 0; i < GP_TILE; i++) s += D[i * Sd + j];
      float* q = part + P.boff[l] + j;
      *q = add ? *q + s : s;
    }
    if (l == 0) break;
    // the deltas of the layer below, through W and the activation that made A
    float* Dn = base + L.d_off[cur ^ 1];
    gl_delta_prev(W, kpad, (P.width[l + 1] + 3) & ~3, D, Sd, 0, P.tiles[l - 1] * 16, lane,
                  [&](int i, int k, float c) { Dn[i * Sd + k] = gl_act_grad(c, A[i * Sa + k], code); });
    __syncthreads();
    cur ^= 1;
  }
}

// The gradient of mean_i loss(softmax(net(state_i))[action_i] - y_i) over n rows with respect to
// the packed weights: this tile's 16 rows' share into partials[tile][total] (every entry written,
// padding entries with 0) and the tile's loss sum into tile_loss[tile].  Forward and backward are
// gl_forward_rows and gl_backward_rows with ReLU as a literal (the PPO learner's kernels,
// gm_ppo_learn.hip, call the same two with tanh); rows in LDS when the plan fits GL_ARENA, else
// in this tile's part of `spill` (global, owned by the learner).
__global__ __launch_bounds__(64) void gm_learn_grad_kernel(const float* __restrict__ state,
                                                           const int32_t* __restrict__ action,
                                                           const float* __restrict__ y, int n,
                                                           const float* __restrict__ params, GpNet P, GlPlan L,
                                                           int loss_kind, float* __restrict__ spill,
                                                           float* __restrict__ partials, long long total,
                                                           float* __restrict__ tile_loss) {
  __shared__ float arena[GL_ARENA];
  __shared__ float row_loss[GP_TILE];
  const int lane = threadIdx.x;
  const int e0 = blockIdx.x * GP_TILE;
  float* base = L.total <= GL_ARENA ? arena : spill + (size_t)blockIdx.x * L.total;
  float* part = partials + (size_t)blockIdx.x * total;

  gl_forward_rows(state, (size_t)e0, (size_t)n, params, P, L, base, GP_ACT_RELU, lane);

  // ---- loss and the deltas of the logits: one lane per row
  const int nl = P.n_layers;
  const int n_out = P.width[nl];
  const int Sd = L.d_stride;
  {
    float* D = base + L.d_off[0];
    const int wd = P.tiles[nl - 1] * 16;
    if (lane < GP_TILE) {
      float* drow = D + lane * Sd;
      float ls = 0.0f;
      if (e0 + lane < n) {
        const size_t row = (size_t)(e0 + lane);
        float qa;
        gp_softmax_argmax(base + L.a_off[nl] + lane * L.a_stride[nl], n_out, drow, &qa);
        const int a = min(max(action[row], 0), n_out - 1);
        qa = drow[a];
        const float d = qa - y[row];
        float dq;
        if (loss_kind == GL_LOSS_MSE) {
          ls = d * d;
          dq = 2.0f * d / (float)n;
        } else {                                   // nn.SmoothL1Loss(), beta 1 (= nn.HuberLoss(), delta 1)
          ls = fabsf(d) < 1.0f ? 0.5f * d * d : fabsf(d) - 0.5f;
          dq = fminf(fmaxf(d, -1.0f), 1.0f) / (float)n;
        }
        const float s = dq * qa;                   // dL/dx_j = dL/dq_a q_a ([a == j] - q_j)
        for (int j = 0; j < n_out; j++) drow[j] = s * ((j == a ? 1.0f : 0.0f) - drow[j]);
        for (int j = n_out; j < wd; j++) drow[j] = 0.0f;
      } else {
        for (int j = 0; j < wd; j++) drow[j] = 0.0f;
      }
      row_loss[lane] = ls;
    }
  }
  __syncthreads();
  if (lane == 0) {
    float s = 0.0f;
    for (int r = 0; r < GP_TILE; r++) s += row_loss[r];
    tile_loss[blockIdx.x] = s;
  }

  gl_backward_rows(params, P, L, base, part, GP_ACT_RELU, false, lane);
}

// what one launch of gm_learn_step_kernel does, in this order, per packed element
struct GlStepArgs {
  int do_sum;            // grad = sum over tiles of the partials, in tile order; thread 0: the mean loss
  int do_step;           // clamp, then Adam / AdamW on p, m, v, vmax
  int do_soft;           // target <- tau p + (1 - tau) target
  int n_tiles, n;
  long long total;
  const float* partials;
  const float* tile_loss;
  const float* tile_loss2;   // NULL, or a second loss's per-tile sums: the loss is the sum of the two means (SAC's loss_q)
  float* grad;
  float* loss;           // [1]
  float* loss_out;       // [1] or NULL: a second copy (gm_learner_train's losses[u])
  float* p;
  float* m;
  float* v;
  float* vmax;
  float* target;
  float tau;
  GlOpt opt;
  const int* skip;       // NULL, or a device flag: nonzero makes the launch a no-op (the PPO learner's KL stop)
  long long gap_at, gap_len;   // element i >= gap_at lies gap_len further on (0: none; the PPO blob's
                               // [actor | critic | log_std], whose policy optimiser skips the critic)
};

__global__ __launch_bounds__(256) void gm_learn_step_kernel(GlStepArgs a) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.total || (a.skip && *a.skip)) return;
  if (a.gap_len != 0 && i >= a.gap_at) i += a.gap_len;   // (never with do_sum: the partials have no gap)
  float g = 0.0f;
  if (a.do_sum) {
    for (int t = 0; t < a.n_tiles; t++) g += a.partials[(size_t)t * a.total + i];
    a.grad[i] = g;             // the raw gradient: kept, readable (gm_learner_read)
    if (i == 0) {
      float s = 0.0f;
      for (int t = 0; t < a.n_tiles; t++) s += a.tile_loss[t];
      s = s / (float)a.n;
      if (a.tile_loss2) {
        float s2 = 0.0f;
        for (int t = 0; t < a.n_tiles; t++) s2 += a.tile_loss2[t];
        s = s + s2 / (float)a.n;
      }
      a.loss[0] = s;
      if (a.loss_out) a.loss_out[0] = s;
    }
  } else if (a.do_step) {
    g = a.grad[i];
  }
  float p = a.p[i];
  if (a.do_step) {
    if (a.opt.clamp > 0.0f) g = fminf(fmaxf(g, -a.opt.clamp), a.opt.clamp);   // clip_grad_value_
    float m = a.m[i], v = a.v[i], vmax = a.vmax[i];
    p = gl_adam(p, g, m, v, vmax, a.opt);
    a.p[i] = p;
    a.m[i] = m;
    a.v[i] = v;
    a.vmax[i] = vmax;
  }
  if (a.do_soft) a.target[i] = gl_soft(p, a.target[i], a.tau);
}
