"""The host side of the SAC collection path, no GPU needed: gm_sac_pack's blob against
gm_policy_pack's layout of each net alone, its errors, the state-dict layout on a locally built
module with MLPActorCriticAC's key names, the float64 mirrors of the draws, the struct sizes and
the option names."""
import ctypes as C

import numpy as np
import pytest

from sac_model import make_module

N_OBS, N_ACT = 7, 3
HIDDEN = (5, 3)


def test_pack_places_every_weight_where_policy_pack_puts_that_net(gm):
    from gmx import sac, policy
    psz, qsz = sac.sizes(N_OBS, N_ACT, (21, 18))       # more than one output tile, k not a multiple of 4
    flat = np.arange(1, sac.n_params(psz, qsz) + 1, dtype=np.float32)     # every weight distinct and non-zero
    blob, q1_off, q2_off = sac.pack(psz, qsz, flat)
    sd = sac.flat_to_state_dict(psz, qsz, flat)
    # the actor as ONE net whose output layer is mu_layer stacked over log_std_layer
    head = psz[:-1] + [2 * N_ACT]
    pi_flat = np.concatenate(
        [sd[f"pi.net.{2 * l}.{w}"].ravel() for l in range(len(psz) - 2) for w in ("weight", "bias")] +
        [np.concatenate([sd["pi.mu_layer.weight"], sd["pi.log_std_layer.weight"]]).ravel(),
         np.concatenate([sd["pi.mu_layer.bias"], sd["pi.log_std_layer.bias"]])])
    pi = policy.pack(head, pi_flat)
    q = [policy.pack(qsz, np.concatenate([sd[f"{n}.q.{2 * l}.{w}"].ravel() for l in range(len(qsz) - 1)
                                          for w in ("weight", "bias")])) for n in ("q1", "q2")]
    assert q1_off == pi.size and q2_off == pi.size + q[0].size and blob.size == pi.size + 2 * q[0].size
    np.testing.assert_array_equal(blob[:q1_off], pi)
    np.testing.assert_array_equal(blob[q1_off:q2_off], q[0])
    np.testing.assert_array_equal(blob[q2_off:], q[1])
    # every weight lands exactly once, everything else is zero padding
    nz = blob[blob != 0]
    assert nz.size == flat.size and np.array_equal(np.sort(nz), flat)
    assert (blob == 0).sum() == blob.size - flat.size > 0
    # the stacked head: output row j of the last layer is mu_layer's row j (j < n_act) or
    # log_std_layer's row j - n_act, at gm_policy_pack's B-fragment position
    off = 0
    for l in range(len(head) - 2):
        kpad, tiles = (head[l] + 3) // 4 * 4, (head[l + 1] + 15) // 16
        off += tiles * (kpad // 4) * 64 + tiles * 16
    ks = (head[-2] + 3) // 4
    stacked = np.concatenate([sd["pi.mu_layer.weight"], sd["pi.log_std_layer.weight"]])
    for j in range(2 * N_ACT):
        for k in range(head[-2]):
            assert blob[off + ((j >> 4) * ks + (k >> 2)) * 64 + (k & 3) * 16 + (j & 15)] == stacked[j, k]
    boff = off + ((2 * N_ACT + 15) // 16) * ks * 64
    np.testing.assert_array_equal(blob[boff:boff + 2 * N_ACT],
                                  np.concatenate([sd["pi.mu_layer.bias"], sd["pi.log_std_layer.bias"]]))


def test_pack_rejects_unsupported_sizes(gm):
    from gmx import sac
    ok_p, ok_q = sac.sizes(N_OBS, N_ACT, HIDDEN)
    sac.pack(ok_p, ok_q, np.zeros(sac.n_params(ok_p, ok_q), np.float32))
    bad = [sac.sizes(N_OBS, N_ACT, (257, 4)),                          # a width above GP_MAX_WIDTH
           sac.sizes(N_OBS, sac.MAX_ACTIONS + 1, HIDDEN),              # n_actions above GA_MAX_ACT
           (ok_p, [N_OBS + N_ACT + 1, *HIDDEN, 1]),                    # q_sizes[0] != n_obs + n_actions
           sac.sizes(N_OBS, N_ACT, (4,) * 8)]                          # more than GP_MAX_LAYERS layers
    for psz, qsz in bad:
        with pytest.raises(ValueError, match="unsupported"):
            sac.pack(psz, qsz, np.zeros(sac.n_params(psz, qsz), np.float32))
    sac.pack(*sac.sizes(N_OBS, sac.MAX_ACTIONS, (256, 4)), np.zeros(sac.n_params(*sac.sizes(N_OBS, sac.MAX_ACTIONS, (256, 4))),
                                                                    np.float32))       # the limits themselves
    with pytest.raises(ValueError, match="parameters expected"):
        sac.pack(ok_p, ok_q, np.zeros(sac.n_params(ok_p, ok_q) + 1, np.float32))
    lib = gm.load_library()
    i32p = C.POINTER(C.c_int32)
    p, q = np.asarray(ok_p, np.int32), np.asarray(ok_q, np.int32)
    assert lib.gm_sac_pack(p.ctypes.data_as(i32p), len(p), q.ctypes.data_as(i32p), len(q), 2, None, None, None) < 0


def test_state_dict_layout_of_a_local_module(gm):
    import torch
    from gmx import sac
    mod = make_module(N_OBS, N_ACT, HIDDEN, seed=4)
    sd = mod.state_dict()
    assert list(sd) == ["pi.net.0.weight", "pi.net.0.bias", "pi.net.2.weight", "pi.net.2.bias", "pi.mu_layer.weight",
                        "pi.mu_layer.bias", "pi.log_std_layer.weight", "pi.log_std_layer.bias", "q1.q.0.weight",
                        "q1.q.0.bias", "q1.q.2.weight", "q1.q.2.bias", "q1.q.4.weight", "q1.q.4.bias", "q2.q.0.weight",
                        "q2.q.0.bias", "q2.q.2.weight", "q2.q.2.bias", "q2.q.4.weight", "q2.q.4.bias"]
    psz, qsz, flat = sac.params_from_state_dict(sd)
    assert (psz, qsz) == sac.sizes(N_OBS, N_ACT, HIDDEN) and flat.size == sac.n_params(psz, qsz)
    # torch's parameters() order is the flat order
    np.testing.assert_array_equal(flat, torch.cat([p.detach().reshape(-1) for p in mod.parameters()]).numpy())
    back = sac.flat_to_state_dict(psz, qsz, flat)
    assert list(back) == list(sd)
    for k in sd:
        np.testing.assert_array_equal(back[k], sd[k].numpy(), err_msg=k)
    assert sac.init_params(psz, qsz, seed=1).size == flat.size


def test_draw_mirrors(gm):
    from gmx import sac, ppo
    gids = np.arange(5000, 5257)
    u = sac.uniform_action_draws(9, gids, 77, 6)
    assert u.shape == (257, 6) and u.min() >= -1.0 and u.max() < 1.0
    np.testing.assert_array_equal(u.astype(np.float32).astype(np.float64), u)      # exact in f32
    assert len(np.unique(u)) > 1500 and abs(u.mean()) < 0.05
    np.testing.assert_array_equal(sac.normal_draws(9, gids, 77, 6), ppo.normal_draws(9, gids, 77, 6))
    assert not np.array_equal(u, sac.uniform_action_draws(9, gids, 78, 6))


def test_struct_sizes_and_options(gm):
    from gmx import sac
    from gmx._lib import SacReplay, SacBatch, SacOpt
    lib = gm.load_library()
    for which, cls in ((0, SacReplay), (1, SacBatch), (2, SacOpt)):
        assert lib.gm_sac_struct_size(which) == C.sizeof(cls)
    assert lib.gm_sac_struct_size(3) == -1
    o = SacOpt()
    lib.gm_sac_opt_default(C.byref(o))
    assert (o.activation, o.action_limit, o.log_std_min, o.log_std_max) == (0, 1.0, -20.0, 2.0)
    assert sac.sac_options() == sac.SAC_DEFAULTS
    assert sac.sac_options(alpha=0.1)["alpha"] == 0.1 and sac.SAC_DEFAULTS["alpha"] == 0.2
    assert sac.SAC_DEFAULTS["batch_size"] == 128 and sac.SAC_DEFAULTS["random_start_episodes"] == 1000
    with pytest.raises(ValueError, match="incorrect key: polyak"):
        sac.sac_options(polyak=0.995)
    assert gm.DeviceSAC is sac.DeviceSAC and gm.ActionReplayBuffer is sac.ActionReplayBuffer
