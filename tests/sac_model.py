"""A small torch module with MLPActorCriticAC's parameter names (pi.net.{0,2,..}, pi.mu_layer,
pi.log_std_layer, q1.q.{0,2,..}, q2.q.{0,2,..}) and the float32 / float64 CPU evaluations the SAC
tests compare the device with.  Built here from the formulas in include/gripper_mi355x.h; shared by
tests/test_sac_host.py, test_sac_forward.py and test_sac_target.py."""
import copy
import math

import numpy as np

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0


def make_module(n_obs, n_actions, hidden, activation="relu", seed=0):
    import torch
    from torch import nn
    act = {"relu": nn.ReLU, "tanh": nn.Tanh}[activation]

    def mlp(sizes, last):
        layers = []
        for i in range(len(sizes) - 1):
            layers += [nn.Linear(sizes[i], sizes[i + 1]), (act if i < len(sizes) - 2 else last)()]
        return nn.Sequential(*layers)

    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            self.net = mlp([n_obs, *hidden], act)
            self.mu_layer = nn.Linear(hidden[-1], n_actions)
            self.log_std_layer = nn.Linear(hidden[-1], n_actions)

    class QFunction(nn.Module):
        def __init__(self):
            super().__init__()
            self.q = mlp([n_obs + n_actions, *hidden, 1], nn.Identity)

    class ActorCritic(nn.Module):
        def __init__(self):
            super().__init__()
            self.pi = Actor()
            self.q1 = QFunction()
            self.q2 = QFunction()

    torch.manual_seed(seed)
    return ActorCritic()


def module_from_flat(n_obs, n_actions, hidden, activation, flat):
    """The module holding the flat parameters (gmx.sac.init_params' order), float32."""
    import torch
    from gmx.sac import flat_to_state_dict, sizes
    mod = make_module(n_obs, n_actions, hidden, activation)
    sd = flat_to_state_dict(*sizes(n_obs, n_actions, hidden), flat)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return mod


def in_dtype(mod, dtype):
    import torch
    return copy.deepcopy(mod).double() if dtype == torch.float64 else mod


def actor_head(mod, obs):
    """(mu, clamped log_std) of the module's actor on obs (a tensor of the module's dtype)."""
    import torch
    with torch.no_grad():
        h = mod.pi.net(obs)
        return mod.pi.mu_layer(h), torch.clamp(mod.pi.log_std_layer(h), LOG_STD_MIN, LOG_STD_MAX)


def logp_of(u, mu, log_std):
    """The squashed Gaussian's log-probability of the pre-squash sample u."""
    import torch
    std = torch.exp(log_std)
    normal = (-((u - mu) ** 2) / (2 * std ** 2) - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
    return normal - (2 * (math.log(2) - u - torch.nn.functional.softplus(-2 * u))).sum(-1)


def critics(mod, state, action):
    import torch
    with torch.no_grad():
        x = torch.cat([state, action], dim=-1)
        return mod.q1.q(x)[:, 0], mod.q2.q(x)[:, 0]


def bound(x32, x64):
    """8 x max|f32 - f64| + one f32 ulp of the largest magnitude (tests/test_actor_critic_forward.py)."""
    x64 = x64.numpy()
    return 8.0 * float(np.abs(x32.numpy().astype(np.float64) - x64).max()) + \
        float(np.spacing(np.float32(np.abs(x64).max())))


def check(name, dev, x32, x64, ratios, label=""):
    """Record |device - f64| / bound of one quantity in ratios[name] and print the figures."""
    b = bound(x32, x64)
    err = float(np.abs(np.asarray(dev, dtype=np.float64) - x64.numpy()).max())
    ratios[name] = max(ratios.get(name, 0.0), err / b)
    print(f"{label} {name}: max |device - f64| {err:.3e}, bound {b:.3e}, ratio {err / b:.3f}")
