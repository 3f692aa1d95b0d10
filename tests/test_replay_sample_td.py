"""gm_replay_sample, gm_policy_td_target and gm_policy_set_params on the GPU, on a replay memory
filled from torch with crafted rows (random observations, end cycling 0 / 1 / 2: terminal and
truncated rows are present by construction).  No env-stepping.

The TD target's tolerance is that of tests/test_actor_critic_forward.py, measured and not chosen:
every expected value is computed on the CPU twice, in float32 and in float64, and the device must
agree with the float64 one within 8 x max|f32 - f64| of that quantity plus one f32 ulp of its
largest magnitude.  The maximum is taken over the 128-row batch, of which the smaller batches
are prefixes: it estimates the f32 evaluation error for these parameters and inputs, which one
row cannot (its |f32 - f64| may be 0).  For double DQN the action is the online net's argmax, which a rounding
difference may flip where the top two outputs are closer than that bound on them: such rows are
left out, and the parameter seed is chosen (on the CPU, with torch alone) so that at least 90 % of
the rows of every batch remain.  Measured worst |device - f64| / bound: see DESIGN.md."""
import numpy as np
import pytest

from conftest import gpu_available
from test_policy_rollout import make_env

pytestmark = pytest.mark.gpu

N_ENVS, CAP, GAMMA = 16, 677, 0.99
NETS = {"canonical": [63, 150, 100, 50, 8], "widest-narrowest": [63, 256, 3, 8]}


@pytest.fixture(scope="module")
def env(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    e = make_env(gm, n=N_ENVS)
    yield e
    e.close()


@pytest.fixture(scope="module")
def memory(env):
    """The crafted memory, made once and left unchanged: (ReplayBuffer, its rows as numpy)."""
    import torch
    from gmx import ReplayBuffer
    g = torch.Generator().manual_seed(11)
    rows = dict(state=torch.rand((CAP, env.n_obs), generator=g) * 2 - 1,
                action=torch.randint(0, env.n_actions, (CAP,), generator=g, dtype=torch.int32),
                next_state=torch.rand((CAP, env.n_obs), generator=g) * 2 - 1,
                reward=torch.randn((CAP,), generator=g),
                end=(torch.arange(CAP) % 3).to(torch.uint8))
    buf = ReplayBuffer(env, CAP)
    for k, v in rows.items():
        getattr(buf, k).copy_(v)
    torch.cuda.synchronize()
    return buf, {k: v.numpy() for k, v in rows.items()}


@pytest.mark.parametrize("size", [128, 677])
@pytest.mark.parametrize("batch", [1, 37, 128])
def test_sample_gathers_the_mirrors_rows(gm, memory, batch, size):
    from gmx.policy import replay_indices
    buf, rows = memory
    buf.pushed = size if size < CAP else 3 * CAP + 17           # len(buf) = min(pushed, capacity)
    assert len(buf) == size
    got = {k: v.cpu().numpy() for k, v in buf.sample(batch, seed=5, draw=batch + size).items()}
    idx = replay_indices(size, batch, 5, batch + size)
    np.testing.assert_array_equal(got["index"], idx)
    assert len(np.unique(got["index"])) == batch and got["index"].min() >= 0 and got["index"].max() < size
    for f in ("state", "action", "next_state", "reward", "end"):
        assert got[f].dtype == rows[f].dtype, f
        np.testing.assert_array_equal(got[f], rows[f][idx], err_msg=f)
    other = buf.sample(batch, seed=5, draw=batch + size + 1)["index"].cpu().numpy()
    assert batch == 1 or not np.array_equal(other, got["index"])
    with pytest.raises((RuntimeError, ValueError)):
        buf.sample(size + 1, seed=5, draw=0)


def torch_forward(sizes, params, x, dtype):
    """VariableNetwork.forward (Linear + ReLU per hidden layer, a final Linear, Softmax(dim=1)) of
    the flat parameters with torch on the CPU in `dtype`."""
    import torch
    p = torch.from_numpy(params).to(dtype)
    x = torch.from_numpy(x).to(dtype)
    pos = 0
    for l in range(len(sizes) - 1):
        fin, fout = sizes[l], sizes[l + 1]
        W = p[pos:pos + fout * fin].reshape(fout, fin)
        pos += fout * fin
        b = p[pos:pos + fout]
        pos += fout
        x = torch.nn.functional.linear(x, W, b)
        if l < len(sizes) - 2:
            x = torch.relu(x)
    return torch.softmax(x, dim=1)


def bound(x32, x64):
    """8 x max|f32 - f64| + one f32 ulp of the largest magnitude."""
    x64 = x64.numpy()
    return 8.0 * float(np.abs(x32.numpy().astype(np.float64) - x64).max()) + \
        float(np.spacing(np.float32(np.abs(x64).max())))


def clear_rows(sizes, params, x):
    """Rows whose top two online outputs differ by more than the bound on those outputs."""
    import torch
    q32, q64 = torch_forward(sizes, params, x, torch.float32), torch_forward(sizes, params, x, torch.float64)
    top = torch.topk(q64, 2, dim=1).values
    return ((top[:, 0] - top[:, 1]) > bound(q32, q64)).numpy()


def choose_seed(sizes, x, ns):
    """The first parameter seed (CPU, torch alone) that leaves >= 90 % clear rows in every prefix."""
    from gmx.policy import init_params
    for seed in range(64):
        ok = clear_rows(sizes, init_params(sizes, seed), x)
        if all(ok[:n].mean() >= 0.9 for n in ns):
            return seed
    raise AssertionError("no parameter seed below 64 separates the online net's top two outputs")


@pytest.mark.parametrize("net", sorted(NETS))
def test_td_target_matches_torch(gm, env, memory, net):
    import torch
    from gmx.policy import DevicePolicy, init_params
    sizes = NETS[net]
    assert sizes[0] == env.n_obs and sizes[-1] == env.n_actions
    buf, rows = memory
    buf.pushed = CAP
    ns = (1, 37, 128)
    full = buf.sample(128, seed=3, draw=7)                      # the smaller batches are its prefixes
    nxt = full["next_state"].cpu().numpy()
    rew, end = full["reward"].cpu().numpy(), full["end"].cpu().numpy()
    assert (end[:37] == 1).any() and (end[:37] == 2).any() and (end[:37] == 0).any()
    oseed = choose_seed(sizes, nxt, ns)
    online = DevicePolicy(env, sizes=sizes, seed=oseed)
    target = DevicePolicy(env, sizes=sizes, seed=oseed + 100)
    worst = {}
    try:
        ref = {}
        for dt in (torch.float32, torch.float64):
            qo = torch_forward(sizes, online.params, nxt, dt)
            qt = torch_forward(sizes, target.params, nxt, dt)
            a = qo.max(1)[1]
            r = torch.from_numpy(rew).to(dt)
            term = torch.from_numpy(end == 1)
            for double in (False, True):
                v = qt.gather(1, a[:, None])[:, 0] if double else qt.max(1)[0]
                for mask in (False, True):
                    vm = torch.where(term, torch.zeros_like(v), v) if mask else v
                    ref[dt, double, mask] = dict(v=vm, y=vm * GAMMA + r)
        clear = clear_rows(sizes, online.params, nxt)
        for n in ns:
            batch = {k: t[:n].contiguous() for k, t in full.items()}
            for double in (False, True):
                every = torch.from_numpy(clear if double else np.ones(len(clear), dtype=bool))
                keep = every[:n].numpy()
                assert keep.mean() >= 0.9, f"{net} n {n}: only {keep.mean():.2f} of the rows are clear"
                for mask in (False, True):
                    y, v = online.td_target(batch, GAMMA, target=target, double=double, mask_terminal=mask)
                    dev = dict(y=y.cpu().numpy(), v=v.cpu().numpy())
                    for q in ("v", "y"):
                        r32, r64 = ref[torch.float32, double, mask][q], ref[torch.float64, double, mask][q]
                        b = bound(r32[every], r64[every])
                        err = float(np.abs(dev[q].astype(np.float64) - r64[:n].numpy())[keep].max())
                        worst[q] = max(worst.get(q, 0.0), err / b)
                        print(f"{net} n {n} double {double} mask {mask} {q}: max |device - f64| {err:.3e}, "
                              f"bound {b:.3e}, ratio {err / b:.3f}, rows {int(keep.sum())}/{n}")
                        assert err <= b, f"{net} n {n} double {double} mask {mask} {q}: {err:.3e} > {b:.3e}"
                    if mask:
                        t = end[:n] == 1
                        np.testing.assert_array_equal(dev["y"][t], rew[:n][t])       # exactly the reward
                        assert (dev["v"][t] == 0).all() and (dev["v"][end[:n] == 2] > 0).all()
                    else:
                        assert (dev["v"] > 0).all()                                  # every row bootstraps
        # target defaults to the online net itself
        y_self, _ = online.td_target(full, GAMMA)
        y_same, _ = online.td_target(full, GAMMA, target=online)
        assert torch.equal(y_self, y_same)
        print(f"{net}: worst |device - f64| / bound {worst}")
    finally:
        online.close()
        target.close()


@pytest.mark.parametrize("net", sorted(NETS))
def test_set_params_equals_a_fresh_policy(gm, env, net):
    from gmx.policy import DevicePolicy, init_params
    sizes = NETS[net]
    new = init_params(sizes, seed=2)
    p = DevicePolicy(env, sizes=sizes, seed=1)
    fresh = DevicePolicy(env, sizes=sizes, params=new)
    try:
        p.act(eps=0.3, seed=4, decision=9)
        a_old, q_old = p.read()
        p.set_params(new)
        p.act(eps=0.3, seed=4, decision=9)
        a_new, q_new = p.read()
        fresh.act(eps=0.3, seed=4, decision=9)
        a_ref, q_ref = fresh.read()
        assert a_new.tobytes() == a_ref.tobytes() and q_new.tobytes() == q_ref.tobytes()
        assert not np.array_equal(q_old, q_new)
        with pytest.raises(ValueError):
            p.set_params(new[:-1])
    finally:
        p.close()
        fresh.close()
