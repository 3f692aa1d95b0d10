"""gm_ac_rollout on a categorical handle: the fused launch (each env's own wave runs the actor,
ga_sample_cat and the critic between its env-steps and applies the index through the discrete-
action path) must equal, bit for bit, gm_ac_act -> gm_step -> gm_ac_record ->
gm_autoreset_episodes, then gm_ac_finish -- on the whole state record, observations, rewards,
done flags, every episode-end record and every array of the trajectory buffer (the helpers are
tests/test_ac_rollout.py's).  33 envs: two full tiles and a one-env tail in the batched kernel;
2-3-step episodes, so truncation, the bootstrap value and the in-launch reset occur."""
import os

import numpy as np
import pytest

from conftest import gpu_available
from test_ac_rollout import HANDOFF, FIELDS, snapshot, assert_same

pytestmark = pytest.mark.gpu

N, K, MAX_EP, SEED, PSEED, DEC0 = 33, 7, 3, 41, 9, 1000


def make_env(gm, env_vars=None, n=N, env_offset=0, termination=False, single=False):
    import bench
    s = gm.canonical_settings(noise=True, seed=SEED)
    s.continous_actions = 0
    s.use_termination_action = int(termination)
    if single:                                                  # one action in use: +- gripper_Z, the smallest softmax
        for name in ("base_X", "base_Y", "base_Z", "base_yaw", "gripper_prismatic_X", "gripper_revolute_Y"):
            getattr(s, name).in_use = 0
    old = {k: os.environ.get(k) for k in (env_vars or {})}
    os.environ.update(env_vars or {})
    try:
        env = gm.BatchedGripperEnv(n, object_set="set6_synthetic", settings=s, seed=SEED, env_offset=env_offset)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    env.set_scene_spawn(bench.mjenv_spawn_params(gm), max_tries=3)
    env.reset()
    return env


def per_step(env, ac, traj, records, k0, k1, max_ep=MAX_EP):
    import torch
    for k in range(k0, k1):
        ac.act(traj, k, sample=True, seed=PSEED, decision=DEC0 + k)
        env.lib.gm_step(env.ctx)
        ac.record(traj, k, max_episode_steps=max_ep)
        env.autoreset_device(0, None, max_episode_steps=max_ep, episodes_dev_ptr=records[k].data_ptr())
    torch.cuda.synchronize()


def both_ways(gm, k=K, max_ep=MAX_EP, env_vars=None, k0=0, hidden=(20, 20), **env_kw):
    """(per-step snapshot, fused snapshot, the fused env's dispatch info and chunk stats)."""
    import torch
    from gmx.ppo import DeviceCategoricalActorCritic, TrajectoryBuffer
    ra = torch.zeros((k, N, 3), dtype=torch.int32, device="cuda")
    rb = torch.zeros((k, N, 3), dtype=torch.int32, device="cuda")
    a, b = make_env(gm, **env_kw), make_env(gm, env_vars, **env_kw)
    pa, pb = (DeviceCategoricalActorCritic(e, hidden=hidden, seed=3) for e in (a, b))
    ta, tb = TrajectoryBuffer(a, k, act_dim=1), TrajectoryBuffer(b, k, act_dim=1)
    try:
        per_step(a, pa, ta, ra, 0, k, max_ep)
        pa.finish(ta)
        per_step(b, pb, tb, rb, 0, k0, max_ep)      # (the hand-off dispatch needs one env-step's dispatch costs)
        pb.rollout(tb, sample=True, seed=PSEED, decision0=DEC0 + k0, max_episode_steps=max_ep,
                   records_dev_ptr=rb[k0:].data_ptr(), k0=k0)
        sa, sb = snapshot(a, ta, ra), snapshot(b, tb, rb)
        return sa, sb, b.dispatch_info(), b.chunk_stats(), a.n_actions
    finally:
        pa.close()
        pb.close()
        a.close()
        b.close()


def not_vacuous(sa, n_actions, k):
    end, boot, act = sa["end"], sa["boot"], sa["act"]
    assert act.shape == (k, N, 1) and sa["mu"].shape == (k, N, n_actions)
    np.testing.assert_array_equal(act, np.round(act))
    assert act.min() >= 0 and act.max() < n_actions
    assert (end == 2).any() and set(np.unique(end)) <= {0, 1, 2}
    assert ((boot != 0) == (end == 2)).all()
    np.testing.assert_array_equal(sa["records"][..., 1] > 0, end != 0)
    assert np.isfinite(sa["logp"]).all() and (sa["logp"] < 0).all()
    assert (sa["last_val"] != 0).all() and (sa["val"] != 0).all()
    # logp is the taken class's log-softmax of the row's logits
    x = sa["mu"].astype(np.float64)
    lse = x.max(-1) + np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1))
    taken = np.take_along_axis(x, act.astype(np.int64), axis=-1)[..., 0]
    np.testing.assert_allclose(sa["logp"], taken - lse, rtol=0, atol=4e-6)


@pytest.mark.parametrize("dispatch", ["default", "handoff-heavy", "one-shot"])
def test_cat_rollout_equals_per_step(gm, dispatch):
    if not gpu_available():
        pytest.skip("no GPU")
    env_vars = {"handoff-heavy": HANDOFF, "one-shot": {"GM_CHUNK_SUBSTEPS": "0"}}.get(dispatch)
    sa, sb, info, stats, na = both_ways(gm, env_vars=env_vars, k0=1 if dispatch == "handoff-heavy" else 0)
    assert_same(gm, sa, sb)
    assert na == 8
    not_vacuous(sa, na, K)
    assert len(np.unique(sa["act"])) >= 6                          # sampled over the classes
    assert int(gm.env_state_view(sa["state"])["episode"].min()) >= 2
    if dispatch == "handoff-heavy":
        print("hand-off heavy:", stats)
        assert stats["yields"] > N, stats                          # envs changed waves mid env-step
    assert (info["chunk"] == 0) == (dispatch == "one-shot")


def test_cat_rollout_with_the_termination_action(gm):
    """use_termination_action on: 9 classes, and taking the last one lifts the base and adds
    substeps to that env-step (set_action_one), inside the launch as through gm_ac_act.  The
    widest and narrowest layers, as tests/test_ac_rollout.py has them for the Gaussian actor."""
    if not gpu_available():
        pytest.skip("no GPU")
    from gmx.ppo import DeviceCategoricalActorCritic          # noqa: F401
    sa, sb, info, _, na = both_ways(gm, k=5, max_ep=2, termination=True, hidden=(256, 3))
    assert_same(gm, sa, sb)
    assert na == 9 and info["chunk"] > 0
    not_vacuous(sa, na, 5)
    assert (sa["act"] == 8).any(), "no env took the termination action: the lift's substeps were not exercised"


def test_cat_rollout_with_one_action_in_use(gm):
    """One action in use: two classes (+-), the smallest softmax."""
    if not gpu_available():
        pytest.skip("no GPU")
    sa, sb, info, _, na = both_ways(gm, k=4, max_ep=2, single=True)
    assert_same(gm, sa, sb)
    assert na == 2 and info["chunk"] > 0
    not_vacuous(sa, na, 4)
    assert set(np.unique(sa["act"])) == {0.0, 1.0}


def test_cat_rollout_is_shard_independent(gm):
    """Contexts of 16 and 17 envs at env_offset 0 and 16 collect what one 33-env context collects."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.ppo import DeviceCategoricalActorCritic, TrajectoryBuffer
    k = 5
    whole = make_env(gm)
    halves = [make_env(gm, n=16, env_offset=0), make_env(gm, n=N - 16, env_offset=16)]
    acs, out = [], []
    try:
        for env in [whole] + halves:
            ac = DeviceCategoricalActorCritic(env, hidden=(20, 20), seed=3)
            acs.append(ac)
            t = TrajectoryBuffer(env, k, act_dim=1)
            ac.rollout(t, sample=True, seed=PSEED, decision0=DEC0, max_episode_steps=MAX_EP)
            torch.cuda.synchronize()
            out.append({f: getattr(t, f).cpu().numpy() for f in FIELDS})
        for f in FIELDS:
            ax = 0 if f == "last_val" else 1
            np.testing.assert_array_equal(out[0][f], np.concatenate([out[1][f], out[2][f]], axis=ax), err_msg=f)
        assert (out[0]["end"] == 2).any()
        assert not np.array_equal(out[1]["act"], out[2]["act"][:, :16])
    finally:
        for ac in acs:
            ac.close()
        whole.close()
        for e in halves:
            e.close()
