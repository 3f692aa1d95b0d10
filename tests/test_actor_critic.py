"""The PPO actor-critic's host side (gmx/ppo.py, gm_ac_pack): the device parameter layout, the
import of an MLPActorCriticPG state dict, the host mirror of the device's counter-based
normal / uniform draws, and gm_ac_create's argument checks (the one GPU part)."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import gpu_available

A = 4


def raw_params(asz, csz, seed):
    rng = np.random.default_rng(seed)
    n = sum(asz[i + 1] * asz[i] + asz[i + 1] for i in range(len(asz) - 1)) + \
        sum(csz[i + 1] * csz[i] + csz[i + 1] for i in range(len(csz) - 1)) + asz[-1]
    return rng.uniform(-1.0, 1.0, size=n).astype(np.float32) + 3.0    # (never zero: the padding is)


def expected_net(sizes, params, pos):
    """One net's packed layout per csrc/gm_policy_net.h, written out independently: for each
    layer, tiles of 16 outputs x k steps of 4, 64 floats each with lane l holding
    W[16 t + (l & 15)][4 s + (l >> 4)], then the bias padded to 16 per tile."""
    out = []
    for l in range(len(sizes) - 1):
        fin, fout = sizes[l], sizes[l + 1]
        W = params[pos:pos + fout * fin].reshape(fout, fin)
        pos += fout * fin
        b = params[pos:pos + fout]
        pos += fout
        tiles, ks = (fout + 15) // 16, (fin + 3) // 4
        Wp = np.zeros((tiles * 16, ks * 4), np.float32)
        Wp[:fout, :fin] = W
        blk = np.zeros((tiles, ks, 64), np.float32)
        for lane in range(64):
            blk[:, :, lane] = Wp[(lane & 15)::16, (lane >> 4)::4][:tiles, :ks]
        out.append(blk.ravel())
        bp = np.zeros(tiles * 16, np.float32)
        bp[:fout] = b
        out.append(bp)
    return np.concatenate(out), pos


@pytest.mark.parametrize("asz", [[63, 64, 64, A], [63, 20, 20, A], [5, 37, 3]])
def test_pack_layout(gm, asz):
    from gmx import ppo
    csz = asz[:-1] + [1]
    p = raw_params(asz, csz, 1)
    packed, coff, loff = ppo.pack(asz, csz, p)
    ea, pos = expected_net(asz, p, 0)
    ec, pos = expected_net(csz, p, pos)
    assert coff == ea.size and loff == ea.size + ec.size
    assert packed.size == loff + asz[-1]
    np.testing.assert_array_equal(packed[:coff], ea)
    np.testing.assert_array_equal(packed[coff:loff], ec)
    np.testing.assert_array_equal(packed[loff:], p[pos:])          # log_std after both nets
    assert pos + asz[-1] == p.size
    # every parameter lands exactly once, everything else is zero padding
    assert np.count_nonzero(packed) == p.size


def test_pack_rejects_unsupported_sizes(gm):
    lib = gm.load_library()
    i32p = C.POINTER(C.c_int32)

    def n(asz, csz):
        a, c = np.asarray(asz, np.int32), np.asarray(csz, np.int32)
        return lib.gm_ac_pack(a.ctypes.data_as(i32p), len(a), c.ctypes.data_as(i32p), len(c), None, None, None)
    assert n([63, 64, A], [63, 64, 1]) > 0
    assert n([63, 257, A], [63, 64, 1]) < 0
    assert n([63, 64, A], [63, 257, 1]) < 0
    assert n([63] + [8] * 8 + [A], [63, 64, 1]) < 0            # 9 layers
    assert n([63, 64, A], [63] + [8] * 8 + [1]) < 0
    assert n([63] + [8] * 7 + [A], [63] + [8] * 7 + [1]) > 0   # 8 layers
    from gmx import ppo
    with pytest.raises(ValueError):
        ppo.pack([63, 300, A], [63, 64, 1], np.zeros(1, np.float32))
    with pytest.raises(ValueError, match="parameters expected"):       # a short array is not read past its end
        ppo.pack([5, 37, 3], [5, 37, 1], np.zeros(10, np.float32))
    assert ppo.n_params([5, 37, 3], [5, 37, 1]) == (37 * 5 + 37 + 3 * 37 + 3) + (37 * 5 + 37 + 37 + 1) + 3


def test_state_dict_import(gm):
    import torch
    from torch import nn
    from gmx import ppo
    torch.manual_seed(0)

    def mlp(sizes):
        layers = []
        for i in range(len(sizes) - 1):
            layers += [nn.Linear(sizes[i], sizes[i + 1]), nn.Tanh() if i < len(sizes) - 2 else nn.Identity()]
        return nn.Sequential(*layers)
    asz, csz = [63, 64, 64, A], [63, 32, 1]
    mu_net, v_net = mlp(asz), mlp(csz)
    log_std = torch.linspace(-0.7, -0.1, A)
    sd = {"pi.log_std": log_std}
    sd.update({"pi.mu_net." + k: v for k, v in mu_net.state_dict().items()})
    sd.update({"vf.v_net." + k: v for k, v in v_net.state_dict().items()})
    a, c, flat = ppo.params_from_state_dict(sd)
    assert a == asz and c == csz
    want = [t.detach().numpy().ravel() for net in (mu_net, v_net) for t in net.parameters()] + [log_std.numpy()]
    np.testing.assert_array_equal(flat, np.concatenate(want))
    assert flat.dtype == np.float32


def test_init_params(gm):
    from gmx import ppo
    asz, csz = [63, 64, 64, A], [63, 64, 64, 1]
    p = ppo.init_params(asz, csz, seed=3)
    np.testing.assert_array_equal(p[-A:], np.full(A, -0.5, np.float32))       # MLPGaussianActor
    w0 = p[:64 * 63]
    assert np.abs(w0).max() <= 1 / math.sqrt(63) and np.abs(w0).max() > 0.9 / math.sqrt(63)
    assert not np.array_equal(p, ppo.init_params(asz, csz, seed=4))
    np.testing.assert_array_equal(p, ppo.init_params(asz, csz, seed=3))


def test_draws_reproduce_and_differ(gm):
    from gmx import ppo
    g = np.arange(100, 164)
    z = ppo.normal_draws(7, g, 12, A)
    assert z.shape == (64, A) and z.dtype == np.float64
    np.testing.assert_array_equal(z, ppo.normal_draws(7, g, 12, A))
    np.testing.assert_array_equal(z[5:9], ppo.normal_draws(7, g[5:9], 12, A))   # keyed by global env id
    assert len(np.unique(z)) == z.size                                          # envs and actions all differ
    assert not np.array_equal(z, ppo.normal_draws(8, g, 12, A))
    assert not np.array_equal(z, ppo.normal_draws(7, g, 13, A))
    u = ppo.noise_draws(7, g, 12, A, 0.05)
    np.testing.assert_array_equal(u, ppo.noise_draws(7, g, 12, A, 0.05))
    assert len(np.unique(u)) == u.size


def test_draw_statistics(gm):
    """4096 x 4 draws: mean, variance and the +-1 sigma mass within 5 standard errors of a
    standard normal's (se(mean) = 1 / sqrt(n), se(var) = sqrt(2 / n), binomial se for the mass);
    the noise inside [-a, a) with a uniform's mean and variance."""
    from gmx import ppo
    z = ppo.normal_draws(1234, np.arange(4096), 3, 4).ravel()
    n = z.size
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 5 / math.sqrt(n)
    assert abs(z.var() - 1) < 5 * math.sqrt(2 / n)
    p1 = math.erf(1 / math.sqrt(2))
    assert abs((np.abs(z) < 1).mean() - p1) < 5 * math.sqrt(p1 * (1 - p1) / n)
    a = 0.05
    u = ppo.noise_draws(1234, np.arange(4096), 3, 4, a).ravel()
    assert u.min() >= -a and u.max() < a
    assert abs(u.mean()) < 5 * (a / math.sqrt(3)) / math.sqrt(n)
    # var of U(-a, a) = a^2 / 3; se of the sample variance = sqrt((mu4 - var^2) / n), mu4 = a^4 / 5
    assert abs(u.var() - a * a / 3) < 5 * math.sqrt((a ** 4 / 5 - (a * a / 3) ** 2) / n)
    # the two streams are distinct counters
    assert abs(np.corrcoef(z, u)[0, 1]) < 5 / math.sqrt(n)


@pytest.mark.gpu
def test_create_checks(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    from gmx.ppo import DeviceActorCritic
    s = gm.canonical_settings(noise=False, seed=2)
    s.continous_actions = 0
    env = gm.BatchedGripperEnv(4, object_set="set1_synthetic", settings=s, seed=2)
    try:
        with pytest.raises(RuntimeError, match="continuous actions"):
            DeviceActorCritic(env, actor_sizes=[env.n_obs, 16, env.n_actions], critic_sizes=[env.n_obs, 16, 1])
        # gm_ac_create itself: GM_E_ARG (-1) and a message
        a = np.asarray([env.n_obs, 16, env.n_actions], np.int32)
        c = np.asarray([env.n_obs, 16, 1], np.int32)
        prm = np.zeros(100000, np.float32)
        i32p = C.POINTER(C.c_int32)
        h = C.c_void_p()
        rc = env.lib.gm_ac_create(env.ctx, a.ctypes.data_as(i32p), 3, c.ctypes.data_as(i32p), 3,
                                  prm.ctypes.data_as(C.POINTER(C.c_float)), C.byref(h))
        assert rc == -1 and not h.value
        assert b"continous_actions" in env.lib.gm_last_error(env.ctx)
    finally:
        env.close()
    env = gm.BatchedGripperEnv(4, object_set="set1_synthetic", settings=gm.canonical_settings(noise=False, seed=2), seed=2)
    try:
        no, na = env.n_obs, env.n_actions
        for asz, csz, word in (([no + 1, 16, na], [no, 16, 1], "actor"), ([no, 16, na + 1], [no, 16, 1], "actor"),
                               ([no, 16, na], [no, 16, 2], "critic"), ([no, 16, na], [no - 1, 16, 1], "critic")):
            with pytest.raises(RuntimeError, match=word):
                DeviceActorCritic(env, actor_sizes=asz, critic_sizes=csz)
        ac = DeviceActorCritic(env, hidden=(16,))
        ac.close()
    finally:
        env.close()
