"""The host side of the SAC learner's options, no GPU needed: sac_opt's mapping of
Agent_SAC.Parameters' names onto gm_sac_learn_opt as Agent_SAC.init hands them to torch, its
errors, and the struct's size against the library's."""
import ctypes as C

import pytest


def test_defaults_are_the_parameters_learner_fields(gm):
    from gmx import sac
    from gmx._lib import OPT_ADAM
    o = sac.sac_opt()
    d = sac.SAC_DEFAULTS
    assert d["optimiser"] == "adam"
    assert (o.optimiser, o.amsgrad) == (OPT_ADAM, 0)
    assert (o.lr, o.beta1, o.beta2) == (d["learning_rate"], d["adam_beta1"], d["adam_beta2"])
    assert (o.eps, o.weight_decay) == (1e-8, 0.0)                  # torch.optim.Adam's own defaults
    assert o.as_dict() == sac.sac_opt_default().as_dict()          # and the library's


def test_adamw_is_amsgrad_with_torchs_decay(gm):
    from gmx import sac
    from gmx._lib import OPT_ADAMW
    for name in ("adamW", "adamw", "ADAMW"):
        o = sac.sac_opt(optimiser=name, learning_rate=3e-4, adam_beta1=0.8, adam_beta2=0.99)
        assert (o.optimiser, o.amsgrad, o.weight_decay) == (OPT_ADAMW, 1, 0.01)
        assert (o.lr, o.beta1, o.beta2) == (3e-4, 0.8, 0.99)
    o = sac.sac_opt(optimiser="adamW", weight_decay=0.0, amsgrad=False)
    assert (o.amsgrad, o.weight_decay) == (0, 0.0)
    # names that only train() reads are accepted and change nothing here
    assert sac.sac_opt(gamma=0.9, alpha=0.1, soft_target_tau=0.01, batch_size=64).as_dict() == sac.sac_opt().as_dict()


def test_unknown_names_and_rmsprop_raise(gm):
    from gmx import sac
    with pytest.raises(ValueError, match="incorrect key: polyak"):
        sac.sac_opt(polyak=0.995)
    with pytest.raises(ValueError, match="incorrect key: grad_clamp_value"):       # SAC has no clamp
        sac.sac_opt(grad_clamp_value=100)
    for name in ("rmsprop", "RMSProp", "sgd"):
        with pytest.raises(ValueError, match="RMSprop is not on the device"):
            sac.sac_opt(optimiser=name)


def test_struct_size_and_exports(gm):
    from gmx import sac
    from gmx._lib import SacLearnOpt
    lib = gm.load_library()
    assert lib.gm_sac_struct_size(4) == C.sizeof(SacLearnOpt) == 48
    assert gm.DeviceSACLearner is sac.DeviceSACLearner and gm.sac_opt is sac.sac_opt
    assert sac.LEARNER_MAX_BATCH == 256
