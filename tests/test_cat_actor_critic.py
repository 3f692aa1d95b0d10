"""The categorical PPO actor-critic's host side (gmx/ppo.py, gm_ac_pack_categorical): the device
layout without log_std, the import of an MLPActorCriticPG(continous_actions=False) state dict
(pi.logits_net.* keys), and the host mirror of the sampler's one uniform per env.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from test_actor_critic import expected_net

A = 8


def raw_params(asz, csz, seed):
    rng = np.random.default_rng(seed)
    n = sum(s[i + 1] * s[i] + s[i + 1] for s in (asz, csz) for i in range(len(s) - 1))
    return rng.uniform(-1.0, 1.0, size=n).astype(np.float32) + 3.0    # (never zero: the padding is)


@pytest.mark.parametrize("asz", [[63, 64, 64, A], [63, 20, 20, A], [5, 37, 3], [63, 256, 3, 9]])
def test_pack_round_trip(gm, asz):
    """pack -> unpack: every parameter lands exactly once in gm_policy_pack's layout, [actor |
    critic] and nothing behind them, and the padding is exactly 0."""
    from gmx import ppo
    csz = asz[:-1] + [1]
    p = raw_params(asz, csz, 1)
    packed, coff, loff = ppo.pack(asz, csz, p, categorical=True)
    ea, pos = expected_net(asz, p, 0)
    ec, pos = expected_net(csz, p, pos)
    assert pos == p.size == ppo.n_params(asz, csz, categorical=True)
    assert coff == ea.size and loff == ea.size + ec.size == packed.size      # no log_std entries
    np.testing.assert_array_equal(packed[:coff], ea)
    np.testing.assert_array_equal(packed[coff:], ec)
    assert np.count_nonzero(packed) == p.size
    pad = ppo.pack(asz, csz, np.ones(p.size, np.float32), categorical=True)[0] == 0
    assert pad.any() and (packed[pad] == 0.0).all() and not np.signbit(packed[pad]).any()
    # unpack: with distinct values, the packed position of every flat entry is known, and
    # reading those positions gives the flat parameters back
    ids = np.arange(1, p.size + 1, dtype=np.float32)
    where = ppo.pack(asz, csz, ids, categorical=True)[0]
    slot = np.empty(p.size, np.int64)
    slot[where[~pad].astype(np.int64) - 1] = np.flatnonzero(~pad)
    np.testing.assert_array_equal(packed[slot], p)
    # and the Gaussian layout of the same nets is this one with log_std appended
    g = np.concatenate([p, np.full(asz[-1], -0.5, np.float32)])
    gp, gc, gl = ppo.pack(asz, csz, g)
    assert (gc, gl) == (coff, loff)
    np.testing.assert_array_equal(gp[:gl], packed)


def test_n_params_and_init(gm):
    from gmx import ppo
    asz, csz = [5, 37, 3], [5, 37, 1]
    nets = (37 * 5 + 37 + 3 * 37 + 3) + (37 * 5 + 37 + 37 + 1)
    assert ppo.n_params(asz, csz, categorical=True) == nets
    assert ppo.n_params(asz, csz) == nets + 3                          # the Gaussian's, unchanged
    p = ppo.init_params(asz, csz, seed=3, categorical=True)
    assert p.size == nets and p.dtype == np.float32
    np.testing.assert_array_equal(p, ppo.init_params(asz, csz, seed=3)[:nets])    # the same nets, no log_std
    with pytest.raises(ValueError, match="parameters expected"):
        ppo.pack(asz, csz, np.zeros(nets + 3, np.float32), categorical=True)


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
    asz, csz = [63, 20, 20, A], [63, 32, 1]
    logits_net, v_net = mlp(asz), mlp(csz)
    sd = {"pi.logits_net." + k: v for k, v in logits_net.state_dict().items()}
    sd.update({"vf.v_net." + k: v for k, v in v_net.state_dict().items()})
    a, c, flat = ppo.params_from_state_dict(sd)
    assert a == asz and c == csz
    want = [t.detach().numpy().ravel() for net in (logits_net, v_net) for t in net.parameters()]
    np.testing.assert_array_equal(flat, np.concatenate(want))
    assert flat.dtype == np.float32 and flat.size == ppo.n_params(asz, csz, categorical=True)


def test_symbols(gm):
    lib = gm.load_library()
    for name in ("gm_ac_create_categorical", "gm_ac_pack_categorical"):
        assert getattr(lib, name) is not None
    i32p = C.POINTER(C.c_int32)
    a, c = np.asarray([63, 64, A], np.int32), np.asarray([63, 64, 1], np.int32)
    off = (C.c_int64 * 2)()
    n = lib.gm_ac_pack_categorical(a.ctypes.data_as(i32p), 3, c.ctypes.data_as(i32p), 3, None, None, off)
    g = lib.gm_ac_pack(a.ctypes.data_as(i32p), 3, c.ctypes.data_as(i32p), 3, None, None, None)
    assert n > 0 and g == n + A and off[1] == n
    assert hasattr(gm, "DeviceCategoricalActorCritic")


def test_uniform_statistics(gm):
    """4096 ids: u in [0, 1) on the 2^-24 grid, mean and variance within 5 standard errors of
    U(0, 1)'s (var 1/12, se(var) = sqrt((mu4 - var^2) / n) with mu4 = 1/80), keyed by global id."""
    from gmx import ppo
    g = np.arange(4096)
    u = ppo.categorical_uniforms(1234, g, 3)
    n = u.size
    assert u.shape == (4096,) and u.dtype == np.float64
    assert u.min() >= 0.0 and u.max() < 1.0
    np.testing.assert_array_equal(u * 16777216.0, np.round(u * 16777216.0))
    assert abs(u.mean() - 0.5) < 5 * math.sqrt(1 / 12 / n)
    assert abs(u.var() - 1 / 12) < 5 * math.sqrt((1 / 80 - (1 / 12) ** 2) / n)
    np.testing.assert_array_equal(u[100:164], ppo.categorical_uniforms(1234, g[100:164], 3))
    assert not np.array_equal(u, ppo.categorical_uniforms(1235, g, 3))
    assert not np.array_equal(u, ppo.categorical_uniforms(1234, g, 4))
    # the draw is the Gaussian sampler's first counter of action 0: one stream, no new constants
    z_u1 = ((ppo._counters(1234, g, 3, 1, 1)[:, 0] >> np.uint64(40)).astype(np.float64)) / 16777216.0
    np.testing.assert_array_equal(u, z_u1)


def inverse_cdf(e, u):
    """ga_sample_cat's rule in float64: the first j whose running sum of e exceeds u * sum e,
    else the last j with e_j > 0.  e: [n, A], u: [n]."""
    run = np.cumsum(e, axis=1)
    t = u * run[:, -1]
    hit = run > t[:, None]
    first = hit.argmax(axis=1)
    last = e.shape[1] - 1 - (e[:, ::-1] > 0).argmax(axis=1)
    return np.where(hit.any(axis=1), first, last)


def test_inverse_cdf_reproduces_a_distribution(gm):
    """A fixed 8-way distribution (one class of probability 0) through the mirror's uniforms:
    each bin's count within 5 binomial standard errors."""
    from gmx import ppo
    p = np.array([0.30, 0.05, 0.0, 0.20, 0.10, 0.25, 0.02, 0.08])
    n = 4096
    u = ppo.categorical_uniforms(99, np.arange(n), 17)
    a = inverse_cdf(np.tile(p * 3.7, (n, 1)), u)          # unnormalised, as the device's e_j are
    counts = np.bincount(a, minlength=8)
    assert counts[2] == 0
    for j in range(8):
        assert abs(counts[j] - n * p[j]) <= 5 * math.sqrt(n * p[j] * (1 - p[j])), (j, counts[j], n * p[j])
