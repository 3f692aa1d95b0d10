// Stand-alone host check of the SAC learner's flat <-> packed walks (csrc/gm_sac_learn.h:
// gsl_for_each_param, gsl_pack, gsl_unpack -- what gm_sac_learner_read, _get_state and _set_state run
// on the host for both optimisers' state) with exactly sized heap buffers, meant to be run under
// AddressSanitizer and UBSan on a machine without a GPU (no kernel is launched):
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Igripper-mujoco_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/sac_walk_check.hip -o sac_walk_check && ./sac_walk_check
// For each net: every flat element lands on its own packed index inside [0, total), the actor's
// elements inside [pi], q1's inside [q1] and q2's inside [q2] (so each optimiser's state stays in
// its own range), the padding entries (total - flat count of them) are 0, unpack(pack(x)) == x, and
// the stacked head puts mu_layer's row r at output row r and log_std_layer's at n_act + r.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "gm_sac_learn.h"

static int check(std::vector<int32_t> hidden, int n_obs, int na) {
  std::vector<int32_t> head{n_obs}, qsz{n_obs + na};
  for (int32_t h : hidden) { head.push_back(h); qsz.push_back(h); }
  head.push_back(2 * na);
  qsz.push_back(1);
  GsNet N{};
  const int64_t tp = gl_layout(head.data(), (int)head.size(), &N.pi);
  const int64_t tq = gl_layout(qsz.data(), (int)qsz.size(), &N.q);
  if (tp < 0 || tq < 0) { std::printf("layout rejected\n"); return 1; }
  N.n_act = na;
  N.q1_off = tp;
  N.q2_off = tp + tq;
  const int64_t total = tp + 2 * tq, n_raw = gsl_flat_count(N);
  const int64_t fpi = gl_flat_count(N.pi), fq = gl_flat_count(N.q);
  std::unique_ptr<float[]> flat(new float[(size_t)n_raw]), back(new float[(size_t)n_raw]), packed(new float[(size_t)total]);
  std::unique_ptr<int[]> hits(new int[(size_t)total]());
  for (int64_t i = 0; i < n_raw; i++) { flat[(size_t)i] = (float)(i + 1); back[(size_t)i] = -1.0f; }
  int64_t seen = 0, bad = 0;
  gsl_for_each_param(N, [&](int64_t i, int64_t k) {
    const int64_t lo = i < fpi ? 0 : (i < fpi + fq ? N.q1_off : N.q2_off);
    const int64_t hi = i < fpi ? N.q1_off : (i < fpi + fq ? N.q2_off : total);
    if (i != seen++ || k < lo || k >= hi) bad++;
    else hits[(size_t)k]++;
  });
  gsl_pack(N, total, flat.get(), packed.get());
  gsl_unpack(N, packed.get(), back.get());
  int64_t zeros = 0;
  for (int64_t k = 0; k < total; k++) {
    if (hits[(size_t)k] > 1) bad++;
    if (hits[(size_t)k] == 0) { zeros++; if (packed[(size_t)k] != 0.0f) bad++; }
  }
  for (int64_t i = 0; i < n_raw; i++) if (back[(size_t)i] != flat[(size_t)i]) bad++;
  if (seen != n_raw || zeros != total - n_raw) bad++;
  // the stacked head: flat order is mu W, mu b, log_std W, log_std b after the hidden layers
  const int L = N.pi.n_layers, in = N.pi.width[L - 1], ks = N.pi.kpad[L - 1] / 4;
  const int64_t h0 = fpi - 2 * ((int64_t)na * in + na);
  for (int r = 0; r < na; r++) {
    for (int head_i = 0; head_i < 2; head_i++) {
      const int j = head_i * na + r;
      const int64_t fb = h0 + head_i * ((int64_t)na * in + na);
      for (int k = 0; k < in; k++)
        if (packed[(size_t)(N.pi.woff[L - 1] + ((int64_t)(j >> 4) * ks + (k >> 2)) * 64 + (k & 3) * 16 + (j & 15))] !=
            flat[(size_t)(fb + (int64_t)r * in + k)]) bad++;
      if (packed[(size_t)(N.pi.boff[L - 1] + j)] != flat[(size_t)(fb + (int64_t)na * in + r)]) bad++;
    }
  }
  std::printf("hidden %zu layers, n_obs %d, n_act %d: %lld flat, %lld packed, %lld padding, %s\n", hidden.size(), n_obs,
              na, (long long)n_raw, (long long)total, (long long)zeros, bad ? "FAILED" : "ok");
  return bad != 0;
}

int main() {
  int rc = 0;
  rc |= check({256, 256}, 63, 9);
  rc |= check({20, 20}, 63, 9);
  rc |= check({256, 3}, 63, 9);
  rc |= check({3, 256}, 63, 9);
  rc |= check({}, 1, 1);
  rc |= check({5, 3}, 7, 3);
  rc |= check({256, 256, 256, 256, 256, 256, 256}, 63, 40);
  return rc;
}
