"""The chunked env-step dispatch (gm_rollout.h chunked_env_steps: a persistent work queue
whose envs yield to envs with more work left and resume on another wave of their XCD) must
give bit for bit the one-shot kernel's results: the same substeps on the same state in the
same order.  Each case steps two contexts of the same batch -- one-shot
(GM_CHUNK_SUBSTEPS=0) and chunked -- with the same actions and compares the full env
records, observations, rewards and done flags after every env-step; the hand-off heavy
setting (a preemption test every substep, no margins, up to 60 yields per env-step) makes
nearly every env change waves several times per env-step once there are more envs than
resident waves (2500 envs).  Batches of 1 and 37 envs leave most XCDs without a
workgroup (every env starts at once, nothing yields)."""
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gm():
    if not gpu_available():
        pytest.skip("no GPU")
    import gmx
    return gmx


def make(gm, n, env_vars):
    old = {k: os.environ.get(k) for k in env_vars}
    os.environ.update(env_vars)
    try:
        env = gm.BatchedGripperEnv(n, object_set="set6_synthetic", settings=gm.canonical_settings(seed=77), seed=77)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    env.reset()
    return env


CHUNKED = {
    "default": {},
    "handoff-heavy": {"GM_CHUNK_SUBSTEPS": "1", "GM_CHUNK_MARGIN": "0", "GM_CHUNK_YIELDS": "60",
                      "GM_CHUNK_CMARGIN": "0"},
}


@pytest.mark.parametrize("n", [1, 37, 2500])
@pytest.mark.parametrize("setting", sorted(CHUNKED))
def test_chunked_equals_one_shot(gm, n, setting):
    one = make(gm, n, {"GM_CHUNK_SUBSTEPS": "0"})
    chk = make(gm, n, CHUNKED[setting])
    assert np.array_equal(one.env_states(), chk.env_states())
    rng = np.random.default_rng(n)
    yields = 0
    for t in range(6):
        a = rng.uniform(-1, 1, size=(n, one.n_actions)).astype(np.float32)
        r1 = one.step(a)
        r2 = chk.step(a)
        for x, y in zip(r1, r2):
            assert np.array_equal(np.asarray(x), np.asarray(y)), f"env-step {t}"
        assert np.array_equal(one.env_states(), chk.env_states()), f"env-step {t}"
        st = chk.chunk_stats()
        assert st["every"] > 0 and st["started"] == n and st["finished"] == n
        assert st["resumes"] == st["yields"]
        assert one.chunk_stats()["every"] == 0
        yields += st["yields"]
    if setting == "handoff-heavy" and n > chk.chunk_stats()["workgroups"]:
        assert yields > n   # the hand-off path really ran (yields need more envs than waves)


def test_job_stats_account_for_the_launch(gm):
    """gm_chunk_job_stats (the per-job diagnostics of the last chunked launch): every job
    that ran has busy clocks, the jobs' yields add up to the queue's yield counter, and no
    job was busy for longer than the launch lasted (shader clocks / 64 at <= 2.6 GHz)."""
    n = 2500
    env = make(gm, n, CHUNKED["handoff-heavy"])
    rng = np.random.default_rng(5)
    for _ in range(2):
        env.step(rng.uniform(-1, 1, size=(n, env.n_actions)).astype(np.float32))
    st = env.chunk_stats()
    clk, yl = env.job_stats()
    assert clk.shape == (n,) and yl.shape == (n,)
    assert (clk > 0).all()
    assert (yl >= 0).all() and int(yl.sum()) == st["yields"]
    assert st["yields"] > 0
    busy_ms = clk.astype(np.float64) * 64 / 2.6e6
    assert busy_ms.max() <= st["span_ms"] * 1.05 + 0.05, (busy_ms.max(), st["span_ms"])
