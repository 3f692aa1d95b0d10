"""The forward-only half of Agent_SAC.optimise_model on the device: the draw of a batch from the
action replay memory (gm_sac_replay_sample), both critics (gm_sac_q) and compute_loss_q's soft
Bellman backup (gm_sac_target), against numpy gathers and a torch evaluation of the same f32
parameters.  Tolerances follow tests/test_sac_forward.py's measured rule: 8 x max|f32 - f64| plus
one f32 ulp of the largest magnitude, per quantity; whatever the device chose itself (a2, u2) is
the input of the quantities derived from it.  Measured worst ratios: see DESIGN.md."""
import numpy as np
import pytest

from conftest import gpu_available
from sac_model import module_from_flat, in_dtype, actor_head, logp_of, critics, check

pytestmark = pytest.mark.gpu

N, K, SEED, PSEED, TSEED = 96, 11, 41, 9, 77
GAMMA, ALPHA = 0.99, 0.2
HIDDEN = (256, 256)


@pytest.fixture(scope="module")
def filled(gm):
    """An env, an online and a target DeviceSAC (different weights) and a memory filled by one
    fused rollout of 11 env-steps of 96 envs (1056 transitions, 5-step episodes)."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from test_sac_rollout import make_env
    from gmx.sac import DeviceSAC, ActionReplayBuffer
    env = make_env(gm)
    online, target = DeviceSAC(env, hidden=HIDDEN, seed=3), DeviceSAC(env, hidden=HIDDEN, seed=4)
    buf = ActionReplayBuffer(env, K * N + 100)
    online.rollout(K, "sample", seed=PSEED, decision0=0, max_episode_steps=5, replay=buf)
    torch.cuda.synchronize()
    host = {f: getattr(buf, f).cpu().numpy().copy() for f in ("state", "action", "next_state", "reward", "end")}
    yield env, online, target, buf, host
    online.close()
    target.close()
    env.close()


@pytest.mark.parametrize("size,batch", [(1000, 128), (33, 33)])
def test_sample_gathers_the_drawn_rows(gm, filled, size, batch):
    from gmx.policy import replay_indices
    env, online, target, buf, host = filled
    assert buf.pushed == K * N and len(buf) == K * N
    pushed = buf.pushed
    try:
        buf.pushed = size
        out = {k: v.cpu().numpy() for k, v in buf.sample(batch, seed=5, draw=3).items()}
        with pytest.raises(ValueError):
            buf.sample(size + 1)
    finally:
        buf.pushed = pushed
    idx = replay_indices(size, batch, seed=5, draw=3)
    np.testing.assert_array_equal(out["index"], idx)
    assert len(np.unique(idx)) == batch and idx.max() < size
    for f in ("state", "action", "next_state", "reward", "end"):
        np.testing.assert_array_equal(out[f], host[f][idx], err_msg=f)
    assert out["action"].shape == (batch, env.n_actions) and np.abs(out["action"]).max() > 0
    assert len(np.unique(out["action"], axis=0)) == batch


@pytest.mark.parametrize("n", [33, 128])
def test_q_matches_torch(gm, filled, n):
    import torch
    env, online, target, buf, host = filled
    # independent device tensors, not views of one concatenated array
    state = buf.state[100:100 + n].clone()
    action = buf.action[200:200 + n].clone()
    q1, q2 = online.q(dict(state=state, action=action))
    mod = module_from_flat(env.n_obs, env.n_actions, HIDDEN, "relu", online.params)
    ref = {dt: critics(in_dtype(mod, dt), state.cpu().to(dt), action.cpu().to(dt)) for dt in (torch.float32, torch.float64)}
    ratios = {}
    check("q1", q1.cpu().numpy(), ref[torch.float32][0], ref[torch.float64][0], ratios, f"n {n}")
    check("q2", q2.cpu().numpy(), ref[torch.float32][1], ref[torch.float64][1], ratios, f"n {n}")
    assert max(ratios.values()) <= 1.0, ratios
    assert np.abs((q1 - q2).cpu().numpy()).max() > 1e-3 and len(np.unique(q1.cpu().numpy())) == n


def target_batch(filled, n=128):
    """A sampled batch whose end codes are written by hand: 0, 1 and 2 all present."""
    import torch
    env, online, target, buf, host = filled
    batch = buf.sample(n, seed=5, draw=8)
    end = np.arange(n) % 3
    batch["end"] = torch.from_numpy(end.astype(np.uint8)).to(batch["end"].device)
    return batch, end


def test_target_matches_torch(gm, filled):
    import torch
    from gmx.sac import normal_draws
    env, online, target, buf, host = filled
    n = 128
    batch, end = target_batch(filled, n)
    o2 = batch["next_state"].cpu()
    rew = batch["reward"].cpu().numpy()
    z = normal_draws(TSEED, np.arange(n), 21, env.n_actions)             # the batch row is the id
    mon = module_from_flat(env.n_obs, env.n_actions, HIDDEN, "relu", online.params)
    mtg = module_from_flat(env.n_obs, env.n_actions, HIDDEN, "relu", target.params)
    for boots_trunc in (False, True):
        y, d = target.target(batch, GAMMA, ALPHA, online=online, bootstrap_truncated=boots_trunc, seed=TSEED, draw=21,
                             debug=True)
        y = y.cpu().numpy()
        d = {k: v.cpu().numpy() for k, v in d.items()}
        ref = {}
        for dt in (torch.float32, torch.float64):
            mu, ls = actor_head(in_dtype(mon, dt), o2.to(dt))
            u_dev, a_dev = torch.from_numpy(d["u2"]).to(dt), torch.from_numpy(d["a2"]).to(dt)
            q1, q2 = critics(in_dtype(mtg, dt), o2.to(dt), a_dev)
            # y from the device's own qmin and logp2, in this dtype's arithmetic
            qm, lp = torch.from_numpy(d["qmin"]).to(dt), torch.from_numpy(d["logp2"]).to(dt)
            ref[dt] = dict(u2=mu + torch.exp(ls) * torch.from_numpy(z).to(dt), a2=torch.tanh(u_dev),
                           logp2=logp_of(u_dev, mu, ls), qmin=torch.min(q1, q2),
                           y=torch.from_numpy(rew).to(dt) + GAMMA * (qm - ALPHA * lp))
        boots = (end == 0) | ((end == 2) & boots_trunc)
        assert boots.any() and (~boots).any()
        ratios = {}
        for q in ("u2", "a2", "logp2", "qmin"):
            check(q, d[q], ref[torch.float32][q], ref[torch.float64][q], ratios, f"bootstrap_truncated {boots_trunc}")
        check("y", y[boots], ref[torch.float32]["y"][boots], ref[torch.float64]["y"][boots], ratios,
              f"bootstrap_truncated {boots_trunc}")
        assert max(ratios.values()) <= 1.0, ratios
        np.testing.assert_array_equal(y[~boots], rew[~boots])                  # y == reward bit for bit where masked
        assert (y[boots] != rew[boots]).all() and np.isfinite(y).all()


def test_target_draws_and_handles(gm, filled):
    env, online, target, buf, host = filled
    batch, _ = target_batch(filled)
    kw = dict(gamma=GAMMA, alpha=ALPHA, seed=TSEED, debug=True)

    def run(tgt, onl, draw):
        y, d = tgt.target(batch, online=onl, draw=draw, **kw)
        return y.cpu().numpy(), {k: v.cpu().numpy() for k, v in d.items()}
    y1, d1 = run(target, online, 21)
    y2, d2 = run(target, online, 21)
    y3, d3 = run(target, online, 22)
    np.testing.assert_array_equal(y1, y2)
    for k in d1:
        np.testing.assert_array_equal(d1[k], d2[k], err_msg=k)            # the same draw repeats bit for bit
    assert (d1["a2"] != d3["a2"]).any(axis=1).all()                        # another draw, other actions
    # a target handle with other weights changes qmin and leaves a2 (the online actor's) unchanged
    y4, d4 = run(online, online, 21)
    np.testing.assert_array_equal(d4["a2"], d1["a2"])
    np.testing.assert_array_equal(d4["logp2"], d1["logp2"])
    assert (d4["qmin"] != d1["qmin"]).all()
    # without the debug outputs: the same y
    np.testing.assert_array_equal(target.target(batch, GAMMA, ALPHA, online=online, seed=TSEED, draw=21).cpu().numpy(), y1)
