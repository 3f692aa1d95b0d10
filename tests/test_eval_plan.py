"""gmx.test_plan and gmx.test_performance: the host side of the batched evaluation
(MujocoTrainer.test's trial order and Trainer.get_test_performance's figures).  No GPU."""
import numpy as np
import pytest

import gmx
from gmx.eval import report_dtype, N_EVENTS, EVENT_NAMES


def test_plan_two_waves_with_one_inactive_env():
    """5 objects x 3 trials on 8 envs: trials 0..7 in wave 0, 8..14 in wave 1, whose env 7 is idle."""
    plan = gmx.test_plan(5, 3, 8)
    assert len(plan) == 2
    w0, w1 = plan
    np.testing.assert_array_equal(w0["trial"], [0, 1, 2, 3, 4, 5, 6, 7])
    np.testing.assert_array_equal(w0["obj_idx"], [0, 0, 0, 1, 1, 1, 2, 2])
    np.testing.assert_array_equal(w0["obj_trial"], [0, 1, 2, 0, 1, 2, 0, 1])
    np.testing.assert_array_equal(w0["active"], [True] * 8)
    np.testing.assert_array_equal(w1["trial"], [8, 9, 10, 11, 12, 13, 14, -1])
    np.testing.assert_array_equal(w1["obj_idx"], [2, 3, 3, 3, 4, 4, 4, -1])
    np.testing.assert_array_equal(w1["obj_trial"], [2, 0, 1, 2, 0, 1, 2, -1])
    np.testing.assert_array_equal(w1["active"], [True] * 7 + [False])
    assert int((~w1["active"]).sum()) == 1


def test_plan_one_wave():
    (w,) = gmx.test_plan(2, 2, 6)
    np.testing.assert_array_equal(w["trial"], [0, 1, 2, 3, -1, -1])
    np.testing.assert_array_equal(w["obj_idx"], [0, 0, 1, 1, -1, -1])
    np.testing.assert_array_equal(w["obj_trial"], [0, 1, 0, 1, -1, -1])
    np.testing.assert_array_equal(w["active"], [True, True, True, True, False, False])


def test_plan_trials_a_multiple_of_the_envs():
    """4 objects x 3 trials on 4 envs: three full waves, no idle env, every trial once and in order."""
    plan = gmx.test_plan(4, 3, 4)
    assert len(plan) == 3
    assert all(w["active"].all() for w in plan)
    trials = np.concatenate([w["trial"] for w in plan])
    np.testing.assert_array_equal(trials, np.arange(12))
    np.testing.assert_array_equal(np.concatenate([w["obj_idx"] for w in plan]), np.arange(12) // 3)
    np.testing.assert_array_equal(np.concatenate([w["obj_trial"] for w in plan]), np.arange(12) % 3)


def test_plan_rejects_empty_tests():
    for bad in ((0, 3, 8), (5, 0, 8), (5, 3, 0)):
        with pytest.raises(ValueError):
            gmx.test_plan(*bad)


def hand_written_report():
    """2 objects x 3 trials.  Object 0 (a sphere, type 2): success, failure, success; object 1 (a
    box, type 6): failure, a failure with a positive reward, success."""
    i_succ = EVENT_NAMES.index("successful_grasp")
    d = np.zeros(6, dtype=report_dtype())
    d["obj_idx"] = [0, 0, 0, 1, 1, 1]
    d["obj_trial"] = [0, 1, 2, 0, 1, 2]
    d["object_type"] = [2, 2, 2, 6, 6, 6]
    d["reward"] = [1.0, -0.5, 1.5, -1.0, 0.75, 1.25]
    d["length"] = [40, 250, 60, 250, 100, 80]
    d["end"] = [1, 2, 1, 2, 1, 1]
    d["abs"][:, i_succ] = [1, 0, 1, 0, 0, 2]
    return d


def test_performance_matches_hand_worked_numbers():
    d = hand_written_report()
    before = d.copy()
    p = gmx.test_performance(d)
    np.testing.assert_array_equal(d, before)                 # the records, in trial order, untouched
    assert p["trials"] == 6
    assert p["success_rate"] == pytest.approx(3 / 6)          # trial 4 has a reward of +0.75 and is no success
    assert p["mean_reward"] == pytest.approx((1.0 - 0.5 + 1.5 - 1.0 + 0.75 + 1.25) / 6)
    assert p["mean_steps"] == pytest.approx((40 + 250 + 60 + 250 + 100 + 80) / 6)
    assert list(p["per_object"]) == [0, 1]
    o0, o1 = p["per_object"][0], p["per_object"][1]
    assert (o0["trials"], o1["trials"]) == (3, 3)
    assert o0["success_rate"] == pytest.approx(2 / 3) and o1["success_rate"] == pytest.approx(1 / 3)
    assert o0["mean_reward"] == pytest.approx(2.0 / 3) and o1["mean_reward"] == pytest.approx(1.0 / 3)
    assert o0["mean_steps"] == pytest.approx(350 / 3) and o1["mean_steps"] == pytest.approx(430 / 3)
    assert list(p["per_object_type"]) == [2, 6]
    assert p["per_object_type"][2] == o0 and p["per_object_type"][6] == o1


def test_performance_counts_a_positive_reward_without_the_event_as_a_failure():
    d = hand_written_report()[4:5]
    assert d["reward"][0] > 0
    assert gmx.test_performance(d)["success_rate"] == 0.0


def test_performance_groups_objects_of_one_type():
    d = hand_written_report()
    d["object_type"] = 2
    p = gmx.test_performance(d)
    assert list(p["per_object_type"]) == [2]
    assert p["per_object_type"][2]["trials"] == 6
    assert p["per_object_type"][2]["success_rate"] == pytest.approx(0.5)
    with pytest.raises(ValueError):
        gmx.test_performance(d[:0])


def test_report_dtype_holds_every_event_column():
    dt = report_dtype()
    assert dt["rows"].shape == dt["abs"].shape == dt["last"].shape == (N_EVENTS,)
    assert N_EVENTS == len(gmx.BINARY_EVENTS) + len(gmx.LINEAR_EVENTS)
