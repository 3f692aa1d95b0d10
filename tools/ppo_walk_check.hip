// Stand-alone host check of the PPO learner's flat <-> packed walks (csrc/gm_ppo_learn.h: gq_layout,
// gq_for_each_param, gq_pack, gq_unpack -- what gm_ac_get_params, gm_ppo_learner_read, _get_state
// and _set_state run on the host) with exactly sized heap buffers, meant to be run under
// AddressSanitizer and UBSan on a machine without a GPU (no kernel is launched):
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Igripper-mujoco_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/ppo_walk_check.hip -o ppo_walk_check && ./ppo_walk_check
// For each net: every flat element lands on its own packed index inside [0, total), the padding
// entries (total - flat count of them) are 0, and unpack(pack(x)) == x.  Each case runs for the
// Gaussian blob [actor | critic | log_std] and for the categorical one [actor | critic], whose flat
// and packed counts are the Gaussian's less n_actions.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "gm_ppo_learn.h"

static int check(std::vector<int32_t> asz, std::vector<int32_t> csz, int categorical = 0) {
  GaNet N;
  int64_t n_raw = 0;
  const int64_t total = gq_layout(asz.data(), (int)asz.size(), csz.data(), (int)csz.size(), &N, &n_raw, categorical);
  if (total < 0) { std::printf("layout rejected\n"); return 1; }
  if (categorical) {   // the Gaussian layout of the same nets less log_std, and nothing behind the critic
    GaNet G;
    int64_t g_raw = 0;
    const int64_t g_total = gq_layout(asz.data(), (int)asz.size(), csz.data(), (int)csz.size(), &G, &g_raw);
    if (g_total - total != asz.back() || g_raw - n_raw != asz.back() || N.log_std_off != total ||
        N.critic_off != G.critic_off || !N.categorical || G.categorical) {
      std::printf("categorical layout differs from the Gaussian one less log_std\n");
      return 1;
    }
  }
  std::unique_ptr<float[]> flat(new float[(size_t)n_raw]), back(new float[(size_t)n_raw]), packed(new float[(size_t)total]);
  std::unique_ptr<int[]> hits(new int[(size_t)total]());
  for (int64_t i = 0; i < n_raw; i++) { flat[(size_t)i] = (float)(i + 1); back[(size_t)i] = -1.0f; }
  int64_t seen = 0, bad = 0;
  gq_for_each_param(N, [&](int64_t i, int64_t k) {
    if (i != seen++ || k < 0 || k >= total) bad++;
    else hits[(size_t)k]++;
  });
  gq_pack(N, total, flat.get(), packed.get());
  gq_unpack(N, packed.get(), back.get());
  int64_t zeros = 0;
  for (int64_t k = 0; k < total; k++) {
    if (hits[(size_t)k] > 1) bad++;
    if (hits[(size_t)k] == 0) { zeros++; if (packed[(size_t)k] != 0.0f) bad++; }
  }
  for (int64_t i = 0; i < n_raw; i++) if (back[(size_t)i] != flat[(size_t)i]) bad++;
  if (seen != n_raw || zeros != total - n_raw) bad++;
  std::printf("%s actor %zu layers, critic %zu layers: %lld flat, %lld packed, %lld padding, %s\n",
              categorical ? "categorical" : "gaussian", asz.size() - 1, csz.size() - 1, (long long)n_raw, (long long)total, (long long)zeros, bad ? "FAILED" : "ok");
  return bad != 0;
}

int main() {
  int rc = 0;
  rc |= check({63, 64, 64, 4}, {63, 64, 64, 1});
  rc |= check({63, 20, 20, 4}, {63, 20, 20, 1});
  rc |= check({63, 256, 256, 200, 4}, {63, 256, 256, 200, 1});
  rc |= check({63, 256, 3, 4}, {63, 3, 256, 1});
  rc |= check({1, 1}, {1, 1});
  rc |= check({63, 256, 256, 256, 256, 256, 256, 256, 40}, {63, 1, 1});
  rc |= check({63, 64, 64, 8}, {63, 64, 64, 1}, 1);
  rc |= check({63, 20, 20, 9}, {63, 20, 20, 1}, 1);
  rc |= check({63, 256, 256, 200, 8}, {63, 256, 256, 200, 1}, 1);
  rc |= check({63, 256, 3, 2}, {63, 3, 256, 1}, 1);
  rc |= check({1, 1}, {1, 1}, 1);
  rc |= check({63, 256, 256, 256, 256, 256, 256, 256, 40}, {63, 1, 1}, 1);
  return rc;
}
