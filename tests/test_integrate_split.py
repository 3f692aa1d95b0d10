"""The profiled env-step's split of the integrate stage (gm_integrate.h, gmx.env integrate_split).

The one-wave kernel's profiled instance marks the Euler damping factor and the Euler solve
inside integrate; their clocks travel in the upper halves of two counter columns (rows, line-search
evaluations).  step_profiled takes them out again, so the counters read as before, and the two
parts are positive and together less than the stage they are parts of.  DUO workgroups take the
factor from the helper wave and report no split.
"""
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu


def profiled(gm, duo):
    old = os.environ.get("GM_DUO")
    os.environ["GM_DUO"] = duo
    try:
        env = gm.BatchedGripperEnv(4, object_set="set6_synthetic", settings=gm.canonical_settings(noise=False, seed=7), seed=7)
    finally:
        if old is None:
            os.environ.pop("GM_DUO", None)
        else:
            os.environ["GM_DUO"] = old
    try:
        env.reset()
        env.set_action(np.zeros((4, env.n_actions), dtype=np.float32))
        ph = env.step_profiled()
        return env.dispatch_info()["waves_per_env"], ph, env.integrate_split.copy(), env.PHASES.index("integrate"), env
    finally:
        env.close()


def test_one_wave_split_is_inside_integrate_and_leaves_the_counters(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    waves, ph, split, ik, env = profiled(gm, "0")
    assert waves == 1
    print(f"\nintegrate {ph[:, ik].tolist()}, Euler factor / solve {split.tolist()}")
    assert (split > 0).all()
    assert (split.sum(axis=1) < ph[:, ik].astype(np.int64)).all()
    # the counters proper: 63 solves of at least one point each, rows and evaluations small numbers
    assert (ph[:, env.PH_NEWTON] >= 63).all() and (ph[:, env.PH_NEWTON] < 63 * 50).all()
    assert (ph[:, env.PH_NEFC] < 2 ** 20).all() and (ph[:, env.PH_LS] < 2 ** 20).all()


def test_duo_reports_no_split(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    waves, ph, split, _, env = profiled(gm, "1")
    assert waves == 2
    assert not split.any()
    assert (ph[:, env.PH_NEFC] < 2 ** 20).all() and (ph[:, env.PH_LS] < 2 ** 20).all()
