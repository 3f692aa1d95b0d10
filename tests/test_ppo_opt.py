"""ppo_opt on the CPU: Agent_PPO.Parameters' learner options under their own names, their defaults
(recorded in tests/golden/ppo_parameters.json), the library's gm_ppo_opt_default and the struct's
layout.  No GPU needed."""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_parameters.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)["defaults"]


def as_parameters(opt):
    """A gm_ppo_opt back under Parameters' names and value types."""
    d = opt.as_dict()
    d["optimiser"] = {0: "adam", 1: "adamW"}[d["optimiser"]]
    d["use_kl_penalty"] = bool(d["use_kl_penalty"])
    d["use_entropy_regularisation"] = bool(d["use_entropy_regularisation"])
    d["grad_clamp_value"] = None if d["grad_clamp_value"] <= 0 else d["grad_clamp_value"]
    return d


def test_defaults_are_the_references(gm):
    from gmx.ppo import ppo_opt, ppo_opt_default, PPO_DEFAULTS
    want = golden()
    assert PPO_DEFAULTS == want
    assert as_parameters(ppo_opt()) == want
    assert as_parameters(ppo_opt_default()) == want                 # the library's own defaults
    assert bytes(ppo_opt()) == bytes(ppo_opt_default())
    assert gm.load_library().gm_struct_size(9) == C.sizeof(ppo_opt())


def test_every_option_reaches_the_struct(gm):
    from gmx.ppo import ppo_opt
    changed = dict(learning_rate_pi=1e-4, learning_rate_vf=2e-4, gamma=0.999, clip_ratio=0.1, train_pi_iters=10,
                   train_vf_iters=11, lam=0.95, target_kl=0.02, max_kl_ratio=2.0, optimiser="adamW",
                   use_kl_penalty=True, use_entropy_regularisation=True, kl_penalty_coefficient=0.3,
                   entropy_coefficient=1e-3, adam_beta1=0.8, adam_beta2=0.99, grad_clamp_value=200)
    assert set(changed) == set(golden())
    assert as_parameters(ppo_opt(**changed)) == changed
    assert as_parameters(ppo_opt(optimiser="ADAM"))["optimiser"] == "adam"      # init() lower-cases the name


def test_unknown_keys_raise(gm):
    from gmx.ppo import ppo_opt
    with pytest.raises(ValueError, match="incorrect key"):
        ppo_opt(learning_rate=1e-3)
    with pytest.raises(ValueError, match="incorrect key"):
        ppo_opt(steps_per_epoch=4000)            # a Parameters field, but not a learner option
    with pytest.raises(ValueError, match="RMSprop"):
        ppo_opt(optimiser="RMSProp")


def test_no_clamp_by_default(gm):
    from gmx.ppo import ppo_opt
    assert ppo_opt(grad_clamp_value=None).grad_clamp_value == 0.0   # <= 0: the library clamps nothing
    assert ppo_opt().grad_clamp_value == 0.0
    assert ppo_opt(grad_clamp_value=5).grad_clamp_value == 5.0
