"""gm_sac_rollout: the SAC rollout fused into one persistent launch (each env's own wave runs the
squashed actor between its env-steps and pushes the transition) must equal, bit for bit, the
per-step sequence gm_sac_act (the batched MFMA kernel) -> gm_sac_push_begin -> gm_step ->
gm_sac_push_end -> gm_autoreset_episodes (include/gripper_mi355x.h).  Checked on the whole fp64
state record, observations, rewards, done flags, every episode-end record and every array of the
memory, with the ring wrapping inside the call, episodes short enough to be truncated and reset
inside the launch, and under the hand-off heavy dispatch.  Also: sharding leaves the memory
unchanged, and a launch without a memory leaves the state of one with."""
import hashlib
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

N, K, MAX_EP, SEED, PSEED, DEC0 = 96, 12, 5, 41, 9, 1000
FIELDS = ("state", "action", "next_state", "reward", "end")

HANDOFF = {"GM_CHUNK_SUBSTEPS": "1", "GM_CHUNK_MARGIN": "0", "GM_CHUNK_YIELDS": "60", "GM_CHUNK_CMARGIN": "0",
           "GM_CHUNK_GRID": "24"}


def make_env(gm, env_vars=None, n=N, env_offset=0):
    import bench
    s = gm.canonical_settings(noise=True, seed=SEED)           # the canonical continuous actions
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


def per_step(env, sac, buf, records, k0, k1, mode="sample", max_ep=MAX_EP, post=None, after=None):
    """Env-steps k0 .. k1 - 1 through the per-step API.  post / after: lists that receive each
    env-step's observation before / after the auto-reset."""
    import torch
    for k in range(k0, k1):
        sac.act(mode, seed=PSEED, decision=DEC0 + k)
        sac.push_begin(buf)
        env.lib.gm_step(env.ctx)
        if post is not None:
            post.append(env.observation())                     # the post-step observation
        sac.push_end(buf, max_episode_steps=max_ep)
        env.autoreset_device(0, None, max_episode_steps=max_ep, episodes_dev_ptr=records[k].data_ptr())
        if after is not None:
            after.append(env.observation())                    # the reset observation where the env was reset
    torch.cuda.synchronize()


def snapshot(env, buf, records):
    import torch
    torch.cuda.synchronize()
    st = env.env_states()
    rew, done = env.reward_done()
    out = dict(hash=hashlib.sha1(np.ascontiguousarray(st).tobytes()).hexdigest(), state_rec=st,
               observation=env.observation(), reward_now=rew, done=done, records=records.cpu().numpy())
    if buf is not None:
        out["pushed"] = buf.pushed
        for f in FIELDS:
            out[f] = getattr(buf, f).cpu().numpy()
    return out


def assert_same(gm, sa, sb, fields=FIELDS):
    va, vb = gm.env_state_view(sa["state_rec"]), gm.env_state_view(sb["state_rec"])
    for f in va.dtype.names:
        np.testing.assert_array_equal(va[f], vb[f], err_msg=f)
    assert sa["hash"] == sb["hash"]
    for f in ("observation", "reward_now", "done", "records") + tuple(fields):
        np.testing.assert_array_equal(sa[f], sb[f], err_msg=f)


def run_pair(gm, n, k, max_ep, hidden, env_vars=None, k0=0, post=None, after=None):
    """(per-step snapshot, fused snapshot, fused env's dispatch info and chunk stats, ring rows): a
    memory of capacity k n + 7 entered 50 rows before its end, so the ring wraps inside the call
    and no env-step starts at a multiple of n."""
    import torch
    from gmx.sac import DeviceSAC, ActionReplayBuffer
    from gmx.policy import ring_rows
    cap = k * n + 7
    row0 = cap - 50
    ra = torch.zeros((k, n, 3), dtype=torch.int32, device="cuda")
    rb = torch.zeros((k, n, 3), dtype=torch.int32, device="cuda")
    a, b = make_env(gm, n=n), make_env(gm, env_vars, n=n)
    pa, pb = DeviceSAC(a, hidden=hidden, seed=3), DeviceSAC(b, hidden=hidden, seed=3)
    ba, bb = ActionReplayBuffer(a, cap), ActionReplayBuffer(b, cap)
    ba.pushed = bb.pushed = row0
    try:
        per_step(a, pa, ba, ra, 0, k, max_ep=max_ep, post=post, after=after)
        # the hand-off dispatch needs the dispatch costs a context records from its first
        # env-step on: b takes that one through the per-step API too
        per_step(b, pb, bb, rb, 0, k0, max_ep=max_ep)
        pb.rollout(k - k0, "sample", seed=PSEED, decision0=DEC0 + k0, max_episode_steps=max_ep,
                   records_dev_ptr=rb[k0:].data_ptr(), replay=bb)
        sa, sb = snapshot(a, ba, ra), snapshot(b, bb, rb)
        info = dict(b.dispatch_info(), stats=b.chunk_stats() if env_vars is HANDOFF else None)
        return sa, sb, info, ring_rows(row0, k, n, cap)
    finally:
        pa.close()
        pb.close()
        a.close()
        b.close()


@pytest.mark.parametrize("dispatch", ["default", "handoff-heavy", "one-shot"])
def test_sac_rollout_equals_per_step(gm, dispatch):
    if not gpu_available():
        pytest.skip("no GPU")
    post, after = [], []
    sa, sb, info, rows = run_pair(gm, N, K, MAX_EP, (256, 256),
                                  {"handoff-heavy": HANDOFF, "one-shot": {"GM_CHUNK_SUBSTEPS": "0"}}.get(dispatch),
                                  k0=1 if dispatch == "handoff-heavy" else 0, post=post, after=after)
    assert_same(gm, sa, sb)
    assert sa["pushed"] == sb["pushed"] == K * N + 7 - 50 + K * N
    # -- what keeps the identity from holding vacuously (on the per-step side's data)
    assert rows.max() == K * N + 6 and rows.min() == 0 and (rows[:, 0] % N != 0).all()      # wrapped, unaligned
    end = sa["end"][rows]                                                                  # [K, N]
    n_term, n_trunc = int((end == 1).sum()), int((end == 2).sum())
    assert n_trunc > 0 and set(np.unique(end)) <= {0, 1, 2}, \
        f"end == 2 occurs {n_trunc} times, end == 1 {n_term} times (terminal ends are not required here)"
    np.testing.assert_array_equal(sa["records"][..., 1] > 0, end != 0)        # record length > 0 <=> an end
    for k in range(K):
        np.testing.assert_array_equal(sa["next_state"][rows[k]], post[k])     # the post-step observation ...
        ended = end[k] != 0
        assert (post[k][ended] != after[k][ended]).any(axis=1).all()          # ... which is not the reset one
        np.testing.assert_array_equal(post[k][~ended], after[k][~ended])
        if k + 1 < K:
            np.testing.assert_array_equal(sa["state"][rows[k + 1]], after[k])  # the next state row: after the reset
    act = sa["action"][rows]                                                   # [K, N, n_actions]
    assert np.abs(act).max() <= 1.0 and len(np.unique(act[0], axis=0)) == N and len(np.unique(act)) > N
    assert int(gm.env_state_view(sa["state_rec"])["episode"].min()) >= 2
    untouched = np.setdiff1d(np.arange(K * N + 7), rows.ravel())
    assert untouched.size == 7 and not sa["state"][untouched].any() and not sb["state"][untouched].any()
    if dispatch == "handoff-heavy":
        assert info["stats"]["yields"] > N and info["stats"]["steals"] > 0, info["stats"]
    assert (info["chunk"] == 0) == (dispatch == "one-shot")


@pytest.mark.parametrize("hidden", [(256, 3), (3, 256)])
def test_sac_rollout_equals_per_step_widest_and_narrowest_layers(gm, hidden):
    """The same identity where the shared forward's indexing is at its limits (width 256 and width
    3 in both positions), at 33 envs (two full 16-env tiles and a one-env tail in the batched
    kernel) with 2-step episodes, so truncation and the in-launch reset occur."""
    if not gpu_available():
        pytest.skip("no GPU")
    n, k = 33, 3
    sa, sb, info, rows = run_pair(gm, n, k, 2, hidden)
    assert_same(gm, sa, sb)
    assert info["chunk"] > 0                                   # the fused launch, not its fallback
    assert (sa["end"][rows] == 2).any() and len(np.unique(sa["action"][rows][0], axis=0)) == n


def test_sac_rollout_is_shard_independent(gm):
    """Two 48-env contexts at env_offset 0 and 48 collect what one 96-env context collects: the
    draws (actions, spawns) are keyed by the global env id."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.sac import DeviceSAC, ActionReplayBuffer
    k = 7
    whole = make_env(gm)
    halves = [make_env(gm, n=N // 2, env_offset=0), make_env(gm, n=N // 2, env_offset=N // 2)]
    sacs, out = [], []
    try:
        for env in [whole] + halves:
            sac = DeviceSAC(env, seed=3)
            sacs.append(sac)
            buf = ActionReplayBuffer(env, k * env.n_envs)
            sac.rollout(k, "sample", seed=PSEED, decision0=DEC0, max_episode_steps=MAX_EP, replay=buf)
            torch.cuda.synchronize()
            out.append({f: getattr(buf, f).cpu().numpy().reshape(k, env.n_envs, -1) for f in FIELDS})
        for f in FIELDS:
            np.testing.assert_array_equal(out[0][f], np.concatenate([out[1][f], out[2][f]], axis=1), err_msg=f)
        assert (out[0]["end"] == 2).any()
        assert not np.array_equal(out[1]["action"], out[2]["action"])
    finally:
        for sac in sacs:
            sac.close()
        whole.close()
        for e in halves:
            e.close()


def test_sac_rollout_without_a_memory(gm):
    """replay=None with GM_SAC_MEAN: state, observations and records equal the recording run's."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.sac import DeviceSAC, ActionReplayBuffer
    k = 6
    a, b = make_env(gm), make_env(gm)
    pa, pb = DeviceSAC(a, seed=3), DeviceSAC(b, seed=3)
    ra = torch.zeros((k, N, 3), dtype=torch.int32, device="cuda")
    rb = torch.zeros((k, N, 3), dtype=torch.int32, device="cuda")
    try:
        buf = ActionReplayBuffer(a, k * N)
        pa.rollout(k, "mean", seed=PSEED, decision0=DEC0, max_episode_steps=MAX_EP, records_dev_ptr=ra.data_ptr(),
                   replay=buf)
        pb.rollout(k, "mean", seed=PSEED, decision0=DEC0, max_episode_steps=MAX_EP, records_dev_ptr=rb.data_ptr())
        sa, sb = snapshot(a, buf, ra), snapshot(b, None, rb)
        assert_same(gm, sa, sb, fields=())
        assert buf.pushed == k * N and (sa["records"][..., 1] > 0).any() and sa["action"].any()
    finally:
        pa.close()
        pb.close()
        a.close()
        b.close()
