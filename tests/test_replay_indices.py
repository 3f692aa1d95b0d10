"""gm_replay_indices, the replay memory's without-replacement draw, on the CPU: a keyed
bijection of [0, size) (4-round balanced Feistel network, cycle-walked), so a full draw is a
permutation; the library's host implementation equals the numpy mirror gmx.policy.replay_indices;
and the ring-row rule of gm_replay on plain integers."""
import ctypes as C

import numpy as np
import pytest

SIZES = [1, 2, 3, 250, 677, 10000]


def lib_indices(gm, size, batch, seed, draw):
    lib = gm.load_library()
    out = np.full(max(batch, 1), -1, dtype=np.int32)
    rc = lib.gm_replay_indices(size, batch, C.c_uint64(seed), C.c_uint64(draw), out.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out[:batch]


@pytest.mark.parametrize("size", SIZES)
def test_full_draw_is_a_permutation_and_equals_the_mirror(gm, size):
    from gmx.policy import replay_indices
    for seed, draw in ((0, 0), (7, 3), (2**63 + 11, 2**40 + 5)):
        rc, idx = lib_indices(gm, size, size, seed, draw)
        assert rc == 0
        np.testing.assert_array_equal(np.sort(idx), np.arange(size))
        np.testing.assert_array_equal(idx, replay_indices(size, size, seed, draw))


@pytest.mark.parametrize("size", SIZES)
def test_a_batch_is_the_prefix_of_the_full_draw(gm, size):
    """Index i depends on (size, seed, draw, i) alone: a smaller batch is a prefix."""
    from gmx.policy import replay_indices
    batch = max(1, size // 3)
    rc, idx = lib_indices(gm, size, batch, 5, 9)
    assert rc == 0
    np.testing.assert_array_equal(idx, lib_indices(gm, size, size, 5, 9)[1][:batch])
    np.testing.assert_array_equal(idx, replay_indices(size, batch, 5, 9))
    assert len(np.unique(idx)) == batch


@pytest.mark.parametrize("size", [s for s in SIZES if s >= 250])
def test_draw_and_seed_change_the_order(gm, size):
    base = lib_indices(gm, size, size, 5, 9)[1]
    other_draw = lib_indices(gm, size, size, 5, 10)[1]
    other_seed = lib_indices(gm, size, size, 6, 9)[1]
    for other in (other_draw, other_seed):
        assert (base != other).mean() > 0.9         # a random permutation keeps ~1 point in place
    assert (other_draw != other_seed).mean() > 0.9
    assert (base != np.arange(size)).mean() > 0.9   # and it is not the identity


def test_batch_larger_than_size_is_rejected(gm):
    from gmx.policy import replay_indices
    for size, batch in ((1, 2), (250, 251), (677, 10000)):
        rc, _ = lib_indices(gm, size, batch, 0, 0)
        assert rc != 0
        with pytest.raises(ValueError):
            replay_indices(size, batch, 0, 0)
    assert lib_indices(gm, 0, 0, 0, 0)[0] != 0        # an empty memory has nothing to draw from
    assert lib_indices(gm, 250, -1, 0, 0)[0] != 0


def test_ring_rows_wrap_in_the_middle_of_an_env_step():
    """Row of env e at env-step k of a call after `pushed` transitions: (pushed + k n_envs + e) %
    capacity -- the reference's deque with every env appended in env order each env-step."""
    from collections import deque
    from gmx.policy import ring_rows
    cap, n = 677, 96
    # the deque model: position in the ring of the t-th transition ever pushed
    ring, slot = deque([], maxlen=cap), {}
    pushed = 0
    for call_steps in (6, 6, 7, 1):
        rows = ring_rows(pushed, call_steps, n, cap)
        assert rows.shape == (call_steps, n)
        assert len(np.unique(rows)) == call_steps * n               # no row twice in one call
        for k in range(call_steps):
            for e in range(n):
                t = pushed + k * n + e
                assert rows[k, e] == t % cap
                ring.append(t)
        pushed += call_steps * n
        # what the deque holds is what the ring holds: the last `cap` transitions
        slot = {t % cap: t for t in range(max(0, pushed - cap), pushed)}
        assert sorted(ring) == sorted(slot.values())
    # the second 6-step call wraps inside env-step 1: envs 0..4 at the end of the ring, 5.. at its start
    rows = ring_rows(6 * n, 6, n, cap)
    assert rows[1, 4] == cap - 1 and rows[1, 5] == 0 and rows[1, 0] == cap - 5
    assert 7 * n < cap < 8 * n
    with pytest.raises(ValueError):
        ring_rows(0, 8, n, cap)                                      # 768 > 677: a row twice
