"""The DQN learner's options without a GPU: gm_dqn_opt_default against Agent_DQN.Parameters' values
as torch resolves them (rl/agents/DQN.py:68-92, 130-151), and gmx.dqn_opt's mapping of the
reference's option names onto gm_dqn_opt."""
import pytest


def test_library_defaults_are_the_agents(gm):
    from gmx._lib import OPT_ADAMW, LOSS_SMOOTH_L1
    d = gm.dqn_opt_default().as_dict()
    assert d == dict(optimiser=OPT_ADAMW, amsgrad=1, loss=LOSS_SMOOTH_L1, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                     weight_decay=0.01, grad_clamp=100.0)
    assert gm.dqn_opt().as_dict() == d                       # the Python mapping's defaults are the library's


def test_option_names_map_like_agent_init(gm):
    from gmx._lib import OPT_ADAM, OPT_ADAMW, LOSS_SMOOTH_L1, LOSS_MSE
    # "adam": torch.optim.Adam(lr, betas) -- no weight decay, no amsgrad (DQN.py:133-137)
    a = gm.dqn_opt(optimiser="Adam", learning_rate=3e-4, adam_beta1=0.8, adam_beta2=0.99).as_dict()
    assert (a["optimiser"], a["amsgrad"], a["weight_decay"]) == (OPT_ADAM, 0, 0.0)
    assert (a["lr"], a["beta1"], a["beta2"], a["eps"]) == (3e-4, 0.8, 0.99, 1e-8)
    # "adamW": torch.optim.AdamW(lr, betas, amsgrad=True) -- torch's weight_decay 0.01 (DQN.py:138-143)
    w = gm.dqn_opt(optimiser="adamw").as_dict()
    assert (w["optimiser"], w["amsgrad"], w["weight_decay"]) == (OPT_ADAMW, 1, 0.01)
    # explicit values win
    o = gm.dqn_opt(optimiser="adam", amsgrad=True, weight_decay=0.01).as_dict()
    assert (o["optimiser"], o["amsgrad"], o["weight_decay"]) == (OPT_ADAM, 1, 0.01)
    # the three criteria (DQN.py:146-151); Huber with delta 1 is smooth-L1 with beta 1
    assert gm.dqn_opt(loss_criterion="smoothL1Loss").loss == LOSS_SMOOTH_L1
    assert gm.dqn_opt(loss_criterion="Huber").loss == LOSS_SMOOTH_L1
    assert gm.dqn_opt(loss_criterion="MSELoss").loss == LOSS_MSE
    # grad_clamp_value None disables the clamp
    assert gm.dqn_opt(grad_clamp_value=None).grad_clamp == 0.0
    assert gm.dqn_opt(grad_clamp_value=2.5).grad_clamp == 2.5
    with pytest.raises(ValueError):
        gm.dqn_opt(optimiser="RMSProp")
    with pytest.raises(ValueError):
        gm.dqn_opt(loss_criterion="L1Loss")


def test_flat_and_packed_orders_round_trip_on_the_host(gm):
    """gm_policy_pack places every flat parameter once and pads with zeros: the map the learner's
    unpack inverts (gm_policy_get_params, gm_learner_read)."""
    import numpy as np
    from gmx.policy import pack
    for sizes in ([63, 150, 100, 50, 8], [63, 256, 3, 8], [5, 3, 2]):
        n = sum(sizes[i] * sizes[i + 1] + sizes[i + 1] for i in range(len(sizes) - 1))
        flat = np.arange(1, n + 1, dtype=np.float32)
        packed = pack(sizes, flat)
        ones = pack(sizes, np.ones(n, dtype=np.float32))
        assert int(ones.sum()) == n and set(np.unique(ones)) <= {0.0, 1.0}
        np.testing.assert_array_equal(np.sort(packed[ones == 1]), flat)
        assert (packed[ones == 0] == 0).all()
