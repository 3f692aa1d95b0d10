"""The DQN replay memory filled on the device (include/gripper_mi355x.h, "DQN replay memory"):
gm_policy_push_begin / gm_policy_push_end around an env-step, and gm_policy_rollout_replay, the
fused rollout that records inside its one persistent launch.

  - the per-step pushes against the public getters, an independent reading: state is the
    observation before the env-step, action the policy's, next_state the observation after
    gm_step and before the auto-reset, reward reward_done()'s, end recomputed from done and
    num_action_steps -- with truncated rows present whose next_state is not the reset observation;
  - the fused launch equals the per-step sequence on every array byte for byte, under the default,
    the hand-off heavy and the one-shot dispatch, across a ring wrap in the middle of an env-step
    (capacity 96 * 7 + 5: the second 6-step call wraps inside its second env-step);
  - recording changes nothing: state, observations and records equal gm_policy_rollout's;
  - a call that would write a row twice is rejected with a message.
Shapes, episode length and eps schedule are tests/test_policy_rollout.py's."""
import numpy as np
import pytest

from conftest import gpu_available
from test_policy_rollout import DEC0, HANDOFF, K, MAX_EP, N, PSEED, eps_schedule, make_env, snapshot

pytestmark = pytest.mark.gpu

CAP = N * 7 + 5
ARRAYS = ("state", "action", "next_state", "reward", "end")
NETS = {"canonical": None, "widest-narrowest": [63, 256, 3, 8]}


def buffer_arrays(buf):
    import torch
    torch.cuda.synchronize()
    return {f: getattr(buf, f).cpu().numpy().copy() for f in ARRAYS}


def per_step(gm, env, pol, buf, records, k0, k1, max_ep=MAX_EP, seen=None):
    """Env-steps k0 .. k1 - 1 through the per-step API: act -> push_begin -> gm_step -> push_end
    -> auto-reset.  seen: a list that receives, per env-step, what the public getters show."""
    import torch
    for k in range(k0, k1):
        before = env.observation() if seen is not None else None
        pol.act(float(eps_schedule(k, k + 1)[0]), seed=PSEED, decision=DEC0 + k)
        pol.push_begin(buf)
        env.lib.gm_step(env.ctx)
        if seen is not None:
            rew, done = env.reward_done()
            steps = gm.env_state_view(env.env_states())["num_action_steps"].copy()
            seen.append(dict(pushed=buf.pushed, before=before, action=pol.read()[0], after=env.observation(), reward=rew,
                             done=done, steps=steps))
        pol.push_end(buf, max_episode_steps=max_ep)
        env.autoreset_device(0, None, max_episode_steps=max_ep, episodes_dev_ptr=records[k].data_ptr())
        if seen is not None:
            seen[-1]["reset"] = env.observation()
    torch.cuda.synchronize()


def test_per_step_pushes_hold_what_the_getters_show(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.policy import DevicePolicy
    from gmx import ReplayBuffer
    env = make_env(gm)
    pol = DevicePolicy(env, seed=3)
    rec = torch.zeros((K, N, 3), dtype=torch.int32, device="cuda")
    try:
        buf = ReplayBuffer(env, CAP)
        assert len(buf) == 0
        seen = []
        n_trunc = n_trunc_differs = 0
        for k in range(K):
            per_step(gm, env, pol, buf, rec, k, k + 1, seen=seen)
            s = seen[-1]
            assert buf.pushed == (k + 1) * N and len(buf) == min(buf.pushed, CAP)
            rows = (s["pushed"] + np.arange(N)) % CAP             # the ring rule, computed here
            got = buffer_arrays(buf)
            end = np.where(s["done"] != 0, 1, np.where(s["steps"] >= MAX_EP, 2, 0)).astype(np.uint8)
            np.testing.assert_array_equal(got["state"][rows], s["before"], err_msg=f"state, env-step {k}")
            np.testing.assert_array_equal(got["action"][rows], s["action"], err_msg=f"action, env-step {k}")
            np.testing.assert_array_equal(got["next_state"][rows], s["after"], err_msg=f"next_state, env-step {k}")
            np.testing.assert_array_equal(got["reward"][rows], s["reward"], err_msg=f"reward, env-step {k}")
            np.testing.assert_array_equal(got["end"][rows], end, err_msg=f"end, env-step {k}")
            trunc = end == 2
            n_trunc += int(trunc.sum())
            n_trunc_differs += int((got["next_state"][rows][trunc] != s["reset"][trunc]).any(axis=1).sum())
            # an env that was reset shows another observation afterwards; one that was not, the same
            np.testing.assert_array_equal(s["reset"][end == 0], s["after"][end == 0])
        assert K * N > CAP                                         # the ring wrapped on the way
        assert (buffer_arrays(buf)["end"] == 2).any(), "the buffer holds no truncated row"
        assert n_trunc > 0 and n_trunc_differs > 0, (n_trunc, n_trunc_differs)
        assert len(np.unique(np.concatenate([s["action"] for s in seen]))) >= 4
    finally:
        pol.close()
        env.close()


def fused_vs_per_step(gm, dispatch, sizes, n=N, k=K, max_ep=MAX_EP, cap=CAP):
    """Two 6-step (k / 2) calls on each side; returns both sides' snapshots and buffers."""
    import torch
    from gmx.policy import DevicePolicy
    from gmx import ReplayBuffer
    ra = torch.zeros((k, n, 3), dtype=torch.int32, device="cuda")
    rb = torch.zeros((k, n, 3), dtype=torch.int32, device="cuda")
    a = make_env(gm, n=n)
    b = make_env(gm, {"handoff-heavy": HANDOFF, "one-shot": {"GM_CHUNK_SUBSTEPS": "0"}}.get(dispatch), n=n)
    pa, pb = DevicePolicy(a, sizes=sizes, seed=3), DevicePolicy(b, sizes=sizes, seed=3)
    try:
        ba, bb = ReplayBuffer(a, cap), ReplayBuffer(b, cap)
        per_step(gm, a, pa, ba, ra, 0, k, max_ep=max_ep)
        # the hand-off dispatch needs the dispatch costs a context records from its first
        # env-step on: b takes that one through the per-step API too
        k0 = 1 if dispatch == "handoff-heavy" else 0
        per_step(gm, b, pb, bb, rb, 0, k0, max_ep=max_ep)
        half = k // 2
        for lo, hi in ((k0, half), (half, k)):
            pb.rollout(eps_schedule(lo, hi), seed=PSEED, decision0=DEC0 + lo, max_episode_steps=max_ep,
                       records_dev_ptr=rb[lo:].data_ptr(), replay=bb)
        assert ba.pushed == bb.pushed == k * n
        sa, sb = snapshot(a, ra), snapshot(b, rb)
        chunk = b.dispatch_info()["chunk"]
        stats = b.chunk_stats() if dispatch == "handoff-heavy" else None
        return sa, sb, buffer_arrays(ba), buffer_arrays(bb), chunk, stats
    finally:
        pa.close()
        pb.close()
        a.close()
        b.close()


def assert_same_rollout(gm, sa, sb):
    va, vb = gm.env_state_view(sa[1]), gm.env_state_view(sb[1])
    for f in va.dtype.names:
        np.testing.assert_array_equal(va[f], vb[f], err_msg=f)
    assert sa[0] == sb[0]
    for i in range(2, 6):
        np.testing.assert_array_equal(sa[i], sb[i])


@pytest.mark.parametrize("dispatch", ["default", "handoff-heavy", "one-shot"])
def test_fused_recording_equals_per_step(gm, dispatch):
    if not gpu_available():
        pytest.skip("no GPU")
    sa, sb, ba, bb, chunk, stats = fused_vs_per_step(gm, dispatch, None)
    assert_same_rollout(gm, sa, sb)
    for f in ARRAYS:
        assert ba[f].tobytes() == bb[f].tobytes(), f
    # -- what keeps the identity from holding vacuously
    # (a reset observation may be all zero: no sensor has read anything yet)
    assert (ba["end"] == 2).any() and (ba["state"] != 0).any(axis=1).mean() > 0.5 and (ba["next_state"] != 0).any(axis=1).all()
    assert len(np.unique(ba["action"])) >= 4 and len(np.unique(ba["reward"])) > 1
    assert K * N > CAP and (K // 2) * N < CAP < (K // 2 + 2) * N  # the second call wraps inside an env-step
    assert (chunk == 0) == (dispatch == "one-shot")
    if dispatch == "handoff-heavy":
        assert stats["yields"] > N and stats["steals"] > 0, stats


def test_fused_recording_equals_per_step_widest_and_narrowest_layers(gm):
    """Layers [63, 256, 3, 8] (tests/test_policy_rollout.py: the shared forward's indexing at its
    limits), 33 envs, 2-step episodes, a capacity that is no multiple of 33."""
    if not gpu_available():
        pytest.skip("no GPU")
    sa, sb, ba, bb, chunk, _ = fused_vs_per_step(gm, "default", NETS["widest-narrowest"], n=33, k=4, max_ep=2,
                                                 cap=33 * 3 + 7)
    assert_same_rollout(gm, sa, sb)
    for f in ARRAYS:
        assert ba[f].tobytes() == bb[f].tobytes(), f
    assert chunk > 0 and (ba["end"] == 2).any() and len(np.unique(ba["action"])) >= 2


@pytest.mark.parametrize("net", sorted(NETS))
def test_recording_does_not_change_the_rollout(gm, net):
    """rollout(replay=buf) leaves the state digest, observations and records of rollout()."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.policy import DevicePolicy
    from gmx import ReplayBuffer
    k = 6
    ra = torch.zeros((k, N, 3), dtype=torch.int32, device="cuda")
    rb = torch.zeros((k, N, 3), dtype=torch.int32, device="cuda")
    a, b = make_env(gm), make_env(gm)
    pa, pb = DevicePolicy(a, sizes=NETS[net], seed=3), DevicePolicy(b, sizes=NETS[net], seed=3)
    try:
        buf = ReplayBuffer(b, CAP)
        kw = dict(seed=PSEED, decision0=DEC0, max_episode_steps=MAX_EP)
        pa.rollout(eps_schedule(0, k), records_dev_ptr=ra.data_ptr(), **kw)
        pb.rollout(eps_schedule(0, k), records_dev_ptr=rb.data_ptr(), replay=buf, **kw)
        assert buf.pushed == k * N and len(buf) == k * N
        assert_same_rollout(gm, snapshot(a, ra), snapshot(b, rb))
        got = buffer_arrays(buf)
        assert (got["next_state"][:k * N] != 0).any(axis=1).all() and (got["end"] != 0).any()
        assert not got["next_state"][k * N:].any()                 # rows past the pushed ones untouched
    finally:
        pa.close()
        pb.close()
        a.close()
        b.close()


def test_a_call_that_would_write_a_row_twice_is_rejected(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    from gmx.policy import DevicePolicy
    from gmx import ReplayBuffer
    env = make_env(gm)
    pol = DevicePolicy(env, seed=3)
    try:
        buf = ReplayBuffer(env, CAP)
        before = env.env_states()
        with pytest.raises(RuntimeError, match="twice"):
            pol.rollout(eps_schedule(0, 8), seed=PSEED, max_episode_steps=MAX_EP, replay=buf)   # 768 > 677
        assert buf.pushed == 0
        np.testing.assert_array_equal(env.env_states(), before)    # nothing ran
        with pytest.raises(ValueError):
            ReplayBuffer(env, N - 1)                               # not even one env-step fits
    finally:
        pol.close()
        env.close()
