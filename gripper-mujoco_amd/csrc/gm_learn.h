// gm_learn.h -- what the DQN learner's kernels (gm_learn.hip) and its host side (gm_capi.hip)
// share: the per-tile row plan of the gradient kernel, the optimiser's launch arguments, the
// elementwise update rules and the map between gm_policy_create's flat parameter order and
// gm_policy_pack's device order.
//
// Reference: rl/agents/DQN.py:317-327 (Agent_DQN.optimise_model from the loss on: criterion,
// backward, clip_grad_value_, optimiser.step) and :352-360 (update_step's soft target update).
// The packed layout is an element permutation of the flat parameters plus zero padding and every
// rule here is elementwise, so gradients and moments live in the packed layout, the step updates
// the policy's d_params in place and nothing is repacked.  A padding entry has weight 0 and
// gradient 0 (its activation column or its delta column is 0), and 0 stays 0 under every rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "gm_policy_net.h"

#define GL_MAX_BATCH 256                       // rows a learner is sized for
#define GL_MAX_TILES (GL_MAX_BATCH / GP_TILE)
#define GL_ARENA 15360                         // floats of LDS (60 KB) a tile's rows may take

#define GL_OPT_ADAM 0
#define GL_OPT_ADAMW 1
#define GL_LOSS_SMOOTH_L1 0
#define GL_LOSS_MSE 1

// One tile's rows, in floats from the tile's base: the post-activation rows of every layer
// (a[0]: the states; a[n_layers]: the logits) and two delta rows that ping-pong down the layers.
// A row set is [16 batch rows][stride]; stride = width rounded up to 32, plus 4 (GP_ROW's
// residue, 4 mod 32: see DESIGN.md "DQN learner" for the bank count of each access).
struct GlPlan {
  int a_off[GP_MAX_LAYERS + 1];
  int a_stride[GP_MAX_LAYERS + 1];
  int d_off[2];
  int d_stride;
  int total;                       // floats per tile; <= GL_ARENA: the rows stay in LDS
};

__host__ __device__ inline int gl_stride(int width) { return ((width + 31) & ~31) + 4; }

inline GlPlan gl_plan(const GpNet& P) {
  GlPlan L{};
  int off = 0, dmax = 0;
  for (int l = 0; l <= P.n_layers; l++) {
    const int w = l == 0 ? P.kpad[0] : P.tiles[l - 1] * 16;
    L.a_off[l] = off;
    L.a_stride[l] = gl_stride(w);
    off += GP_TILE * L.a_stride[l];
    if (l > 0 && w > dmax) dmax = w;
  }
  L.d_stride = gl_stride(dmax);
  for (int b = 0; b < 2; b++) {
    L.d_off[b] = off;
    off += GP_TILE * L.d_stride;
  }
  L.total = off;
  return L;
}

// the optimiser's arguments for one launch of gm_learn_step_kernel.  torch keeps the
// hyperparameters as doubles and rounds each derived scalar to f32 where it meets the tensor;
// the host does the same (gm_capi.hip learner_opt), the bias corrections of step t included.
struct GlOpt {
  int optimiser, amsgrad;
  float omb1;           // 1 - beta1
  float beta2, omb2;    // beta2, 1 - beta2
  float eps, wd;
  float decay;          // 1 - lr wd (AdamW)
  float clamp;          // clip_grad_value_'s bound; <= 0: none
  float step_size;      // lr / (1 - beta1^t)
  float bc2_sqrt;       // sqrt(1 - beta2^t)
};

// torch.optim.Adam / AdamW, single-tensor form, on one element: g the (already clamped) gradient
__device__ __forceinline__ float gl_adam(float p, float g, float& m, float& v, float& vmax, const GlOpt& o) {
  if (o.optimiser == GL_OPT_ADAMW)
    p = p * o.decay;                                    // param.mul_(1 - lr * weight_decay)
  else if (o.wd != 0.0f)
    g = g + o.wd * p;                                   // grad.add(param, alpha = weight_decay)
  m = m + o.omb1 * (g - m);                             // exp_avg.lerp_(grad, 1 - beta1)
  v = v * o.beta2 + o.omb2 * (g * g);                   // mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  float s = v;
  if (o.amsgrad) {
    vmax = fmaxf(vmax, v);
    s = vmax;
  }
  const float denom = sqrtf(s) / o.bc2_sqrt + o.eps;
  return p - o.step_size * (m / denom);                 // addcdiv_(exp_avg, denom, value = -step_size)
}

// theta' <- tau theta + (1 - tau) theta' (DQN.py:352-360).  The two products cancel where the
// nets differ in sign, so the sum is formed in double and rounded once: within half an ulp of the
// exact value for every pair, and tau = 1 copies theta bit for bit.
__device__ __forceinline__ float gl_soft(float online, float target, float tau) {
  return (float)((double)tau * (double)online + (1.0 - (double)tau) * (double)target);
}

// the packed layout of a net of these layer sizes: its packed float count, or -1 for more than
// GP_MAX_LAYERS layers or a width outside 1 .. GP_MAX_WIDTH
inline int64_t gl_layout(const int32_t* sizes, int n_sizes, GpNet* net) {
  if (!sizes || n_sizes < 2 || n_sizes - 1 > GP_MAX_LAYERS) return -1;
  GpNet P{};
  P.n_layers = n_sizes - 1;
  long long off = 0;
  for (int l = 0; l < n_sizes; l++) {
    if (sizes[l] < 1 || sizes[l] > GP_MAX_WIDTH) return -1;
    P.width[l] = sizes[l];
  }
  for (int l = 0; l < P.n_layers; l++) {
    P.kpad[l] = (P.width[l] + 3) & ~3;
    P.tiles[l] = (P.width[l + 1] + 15) / 16;
    P.woff[l] = off;
    off += (long long)P.tiles[l] * (P.kpad[l] / 4) * 64;
    P.boff[l] = off;
    off += (long long)P.tiles[l] * 16;
  }
  if (net) *net = P;
  return off;
}

// flat parameter count of a net, and the packed index of flat element i (gm_policy_pack's rule)
inline int64_t gl_flat_count(const GpNet& P) {
  int64_t n = 0;
  for (int l = 0; l < P.n_layers; l++) n += (int64_t)P.width[l + 1] * P.width[l] + P.width[l + 1];
  return n;
}
template <class F>
inline void gl_for_each_param(const GpNet& P, F f) {   // f(flat index, packed index)
  int64_t i = 0;
  for (int l = 0; l < P.n_layers; l++) {
    const int in = P.width[l], outw = P.width[l + 1], ks = P.kpad[l] / 4;
    for (int j = 0; j < outw; j++)
      for (int k = 0; k < in; k++)
        f(i++, (int64_t)P.woff[l] + ((int64_t)(j >> 4) * ks + (k >> 2)) * 64 + (k & 3) * 16 + (j & 15));
    for (int j = 0; j < outw; j++) f(i++, (int64_t)P.boff[l] + j);
  }
}
