"""On-device PPO data collection for the batched env: a Gaussian actor and a critic evaluated
on the device, a device trajectory buffer and the GAE-lambda scan.

Mirrors the reference's policy-gradient rollout side:
  - MLPActorCriticPG.step (rl/agents/PolicyGradient.py:522-528): mu = mu_net(obs), a = mu +
    exp(log_std) z, logp = Normal(mu, std).log_prob(a).sum(-1), v = v_net(obs); both nets are
    mlp([...], Tanh) with an identity output layer (:47-55, 449-500);
  - Agent_PPO.select_action (:1348-1388): uniform exploration noise added after logp;
  - PPOBuffer (:301-409): finish_trajectory's GAE-lambda advantages and rewards-to-go, get()'s
    advantage normalisation;
and its learner, Agent_PPO.optimise_model (:1440-1522): DevicePPOLearner runs compute_loss_pi's
and compute_loss_v's backward, both Adam / AdamW optimisers and the KL stop on the device weights
the rollout reads, so a training loop is ac.rollout(traj) followed by learner.update(traj).

DeviceCategoricalActorCritic is the same for discrete actions: MLPActorCriticPG(continous_actions=
False)'s MLPCategoricalActor (:429-447), whose outputs are logits and which has no log_std.  The
buffer's action is then the chosen index as a float, TrajectoryBuffer(env, K, act_dim=1).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import load_library, PpoOpt, PpoBatch, PpoInfo, OPT_ADAM, OPT_ADAMW
from .policy import _M64, _mix, as_f32, linear_init, state_dict_net

DEFAULT_HIDDEN = (64, 64)          # MLPActorCriticPG's default hidden_sizes
LOG_STD_INIT = -0.5                # MLPGaussianActor


def _counters(seed, gids, decision, n_actions, j):
    """c_j of csrc/gm_ac_net.h for every (env, action): [len(gids), n_actions] uint64."""
    gids = np.atleast_1d(np.asarray(gids, dtype=np.uint64))
    with np.errstate(over="ignore"):
        h = _mix(np.uint64(int(seed) & _M64) ^ _mix(gids * np.uint64(0x100000001B3) + np.uint64(int(decision) & _M64)))
        i = np.arange(n_actions, dtype=np.uint64)
        return _mix(h[:, None] + np.uint64(3) * i[None, :] + np.uint64(j))


def normal_draws(seed, gids, decision, n_actions) -> np.ndarray:
    """The device sampler's standard normal draws z (float64) for global env ids `gids` at one
    decision index: Box-Muller on two 24-bit uniforms, the first in (0, 1]."""
    u1 = ((_counters(seed, gids, decision, n_actions, 1) >> np.uint64(40)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (_counters(seed, gids, decision, n_actions, 2) >> np.uint64(40)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def noise_draws(seed, gids, decision, n_actions, noise: float) -> np.ndarray:
    """The device's uniform exploration noise in [-noise, noise) (float64)."""
    u3 = (_counters(seed, gids, decision, n_actions, 3) >> np.uint64(40)).astype(np.float64) / 16777216.0
    return float(noise) * (2.0 * u3 - 1.0)


def categorical_uniforms(seed, gids, decision) -> np.ndarray:
    """The categorical sampler's one uniform u in [0, 1) per env (float64, exact: 24 bits) for
    global env ids `gids` at one decision index: csrc/gm_ac_net.h ga_sample_cat's (c >> 40) / 2^24
    with c = mix(h + 1), h the eps-greedy key.  The device takes the first j whose running sum of
    e_j = exp(x_j - max x) exceeds u * sum e."""
    return (_counters(seed, gids, decision, 1, 1)[:, 0] >> np.uint64(40)).astype(np.float64) / 16777216.0


def init_params(actor_sizes, critic_sizes, seed: int = 0, categorical: bool = False) -> np.ndarray:
    """nn.Linear's default init for both nets and log_std = -0.5, flattened: the actor's W0
    [out x in], b0, W1, b1, ..., the critic's likewise, then log_std (categorical: no log_std)."""
    rng = np.random.default_rng(seed)
    parts = linear_init(rng, actor_sizes) + linear_init(rng, critic_sizes)
    if not categorical:
        parts.append(np.full(actor_sizes[-1], LOG_STD_INIT, dtype=np.float32))
    return np.concatenate(parts).astype(np.float32)


def params_from_state_dict(state_dict):
    """(actor_sizes, critic_sizes, flat params) from an MLPActorCriticPG state dict: pi.log_std,
    pi.mu_net.{0,2,..}.weight / .bias, vf.v_net.{0,2,..}.weight / .bias; or a categorical one's
    pi.logits_net.{0,2,..}.weight / .bias and vf.v_net.*, which has no log_std."""
    def net(prefix):
        ws = sorted((k for k in state_dict if k.startswith(prefix) and k.endswith(".weight")),
                    key=lambda k: int(k[len(prefix):].split(".")[0]))
        if not ws:
            raise KeyError(f"no {prefix}*.weight in the state dict")
        return state_dict_net(state_dict, ws)
    categorical = any(k.startswith("pi.logits_net.") for k in state_dict)
    asz, ap = net("pi.logits_net." if categorical else "pi.mu_net.")
    csz, cp = net("vf.v_net.")
    tail = [] if categorical else [as_f32(state_dict["pi.log_std"]).ravel()]
    return asz, csz, np.concatenate(ap + cp + tail).astype(np.float32)


def n_params(actor_sizes, critic_sizes, categorical: bool = False) -> int:
    """Floats of the flat parameters (init_params' order) for these layer sizes."""
    return (sum(s[i + 1] * s[i] + s[i + 1] for s in (actor_sizes, critic_sizes) for i in range(len(s) - 1))
            + (0 if categorical else actor_sizes[-1]))


def pack(actor_sizes, critic_sizes, params, categorical: bool = False):
    """(packed blob, critic offset, log_std offset): the device layout (gm_ac_pack, or
    gm_ac_pack_categorical, whose log_std offset is the blob's end; testable without a GPU).
    Raises ValueError for unsupported sizes or a wrong parameter count."""
    lib = load_library()
    fn = lib.gm_ac_pack_categorical if categorical else lib.gm_ac_pack
    a = np.ascontiguousarray(actor_sizes, dtype=np.int32)
    c = np.ascontiguousarray(critic_sizes, dtype=np.int32)
    pr = np.ascontiguousarray(params, dtype=np.float32).ravel()
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    off = (C.c_int64 * 2)()
    n = fn(a.ctypes.data_as(i32p), len(a), c.ctypes.data_as(i32p), len(c), pr.ctypes.data_as(f32p), None, off)
    if n < 0:
        raise ValueError("unsupported network sizes")
    want = n_params([int(x) for x in a], [int(x) for x in c], categorical)
    if pr.size != want:
        raise ValueError(f"{want} parameters expected for these sizes, got {pr.size}")
    out = np.zeros(n, dtype=np.float32)
    fn(a.ctypes.data_as(i32p), len(a), c.ctypes.data_as(i32p), len(c), pr.ctypes.data_as(f32p),
       out.ctypes.data_as(f32p), off)
    return out, int(off[0]), int(off[1])


class AcTraj(C.Structure):
    """gm_ac_traj (include/gripper_mi355x.h)."""
    _fields_ = [("capacity", C.c_int32), ("pad", C.c_int32), ("obs", C.c_void_p), ("act", C.c_void_p),
                ("logp", C.c_void_p), ("val", C.c_void_p), ("rew", C.c_void_p), ("end", C.c_void_p),
                ("boot", C.c_void_p), ("last_val", C.c_void_p), ("mu", C.c_void_p)]


class TrajectoryBuffer:
    """K env-steps of every env, as torch tensors on the env's device in gm_ac_traj's layout
    (time-major: all envs of one env-step are contiguous).  act_dim: floats of one action, by
    default the env's n_actions; 1 for a DeviceCategoricalActorCritic, whose action is the chosen
    index (mu then holds the logits, [K, n_envs, n_actions] either way)."""

    def __init__(self, env, K: int, keep_mu: bool = True, act_dim: int | None = None):
        import torch
        self.env = env
        self.K = int(K)
        n, dev = env.n_envs, f"cuda:{env.device}"
        f = dict(dtype=torch.float32, device=dev)
        self.obs = torch.zeros((self.K, n, env.n_obs), **f)
        self.act = torch.zeros((self.K, n, env.n_actions if act_dim is None else int(act_dim)), **f)
        self.logp = torch.zeros((self.K, n), **f)
        self.val = torch.zeros((self.K, n), **f)
        self.rew = torch.zeros((self.K, n), **f)
        self.end = torch.zeros((self.K, n), dtype=torch.uint8, device=dev)
        self.boot = torch.zeros((self.K, n), **f)
        self.last_val = torch.zeros((n,), **f)
        self.mu = torch.zeros((self.K, n, env.n_actions), **f) if keep_mu else None
        self.adv = torch.zeros((self.K, n), **f)
        self.ret = torch.zeros((self.K, n), **f)
        torch.cuda.synchronize(dev)    # the zero fills, before the env's own stream writes

    def struct(self, k0: int = 0) -> AcTraj:
        """The gm_ac_traj of rows k0 .. K - 1 (row k0 is the struct's row 0)."""
        t = AcTraj()
        t.capacity = self.K - k0
        for name in ("obs", "act", "logp", "val", "rew", "end", "boot"):
            setattr(t, name, getattr(self, name)[k0:].data_ptr())
        t.last_val = self.last_val.data_ptr()
        t.mu = self.mu[k0:].data_ptr() if self.mu is not None else None
        return t

    def gae(self, gamma: float, lam: float, n_steps: int | None = None):
        """gm_ac_gae over the first n_steps rows: (adv, ret) device tensors [n_steps, n_envs]."""
        import torch
        k = self.K if n_steps is None else int(n_steps)
        t = self.struct()
        torch.cuda.synchronize(self.adv.device)     # torch-side writes to the buffers (tests)
        rc = self.env.lib.gm_ac_gae(self.env.ctx, C.byref(t), k, C.c_float(gamma), C.c_float(lam),
                                    C.c_void_p(self.adv.data_ptr()), C.c_void_p(self.ret.data_ptr()))
        if rc != 0:
            raise RuntimeError(self.env.lib.gm_last_error(self.env.ctx).decode() or f"gm_ac_gae failed ({rc})")
        torch.cuda.synchronize(self.adv.device)     # the env's stream, before torch reads the results
        return self.adv[:k], self.ret[:k]

    def get(self, gamma: float = 0.99, lam: float = 0.97, n_steps: int | None = None) -> dict:
        """PPOBuffer.get (PolicyGradient.py:384-409): obs, act, ret, adv, logp flattened to
        [n_steps * n_envs, ...], the advantages normalised with torch.std_mean (unbiased)."""
        import torch
        adv, ret = self.gae(gamma, lam, n_steps)
        k = adv.shape[0]
        std, mean = torch.std_mean(adv)
        return dict(obs=self.obs[:k].reshape(-1, self.obs.shape[-1]), act=self.act[:k].reshape(-1, self.act.shape[-1]),
                    ret=ret.reshape(-1), adv=((adv - mean) / std).reshape(-1), logp=self.logp[:k].reshape(-1))


def adv_normalise(env, adv):
    """gm_ac_adv_normalise in place on a contiguous float32 device tensor: adv <- (adv - mean) /
    std with torch.std_mean's unbiased std (PPOBuffer.get), the sums in double in a fixed order.
    Returns adv.  One element raises: its standard deviation is undefined."""
    import torch
    if adv.dtype != torch.float32 or not adv.is_cuda or not adv.is_contiguous():
        raise ValueError("a contiguous float32 device tensor expected")
    torch.cuda.synchronize(adv.device)     # torch-side writes to adv
    rc = env.lib.gm_ac_adv_normalise(env.ctx, C.c_void_p(adv.data_ptr()), int(adv.numel()))
    if rc != 0:
        raise RuntimeError(env.lib.gm_last_error(env.ctx).decode() or f"gm_ac_adv_normalise failed ({rc})")
    torch.cuda.synchronize(adv.device)     # the env's stream, before torch reads the result
    return adv


class DeviceActorCritic:
    """An MLPActorCriticPG (Gaussian actor, critic) bound to a BatchedGripperEnv with
    continuous actions."""

    categorical = False
    _create = "gm_ac_create"
    _actor_prefix = "pi.mu_net."

    def __init__(self, env, hidden=DEFAULT_HIDDEN, params=None, seed: int = 0, hidden_v=None,
                 actor_sizes=None, critic_sizes=None):
        self.env = env
        self.lib = env.lib
        hv = hidden if hidden_v is None else hidden_v
        self.actor_sizes = [int(x) for x in (actor_sizes or [env.n_obs, *hidden, env.n_actions])]
        self.critic_sizes = [int(x) for x in (critic_sizes or [env.n_obs, *hv, 1])]
        #: the last weights handed in from the host (the constructor's, set_params'); a
        #: DevicePPOLearner's steps do not reach it: get_params() returns the device's
        self.params = (init_params(self.actor_sizes, self.critic_sizes, seed, self.categorical) if params is None
                       else np.ascontiguousarray(params, np.float32).copy())
        self._p = C.c_void_p()
        if min(self.actor_sizes + self.critic_sizes) < 1 or len(self.actor_sizes) < 2 or len(self.critic_sizes) < 2:
            raise ValueError("layer sizes must be positive, with at least an input and an output")
        want = n_params(self.actor_sizes, self.critic_sizes, self.categorical)
        if self.params.ndim != 1 or self.params.size != want:      # (the library reads exactly this many)
            raise ValueError(f"{want} parameters expected for these sizes, got {self.params.size}")
        a = np.ascontiguousarray(self.actor_sizes, dtype=np.int32)
        c = np.ascontiguousarray(self.critic_sizes, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        rc = getattr(self.lib, self._create)(env.ctx, a.ctypes.data_as(i32p), len(a), c.ctypes.data_as(i32p), len(c),
                                             self.params.ctypes.data_as(C.POINTER(C.c_float)), C.byref(self._p))
        if rc != 0:
            raise RuntimeError(self.lib.gm_last_error(env.ctx).decode() or f"{self._create} failed ({rc})")

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(self.lib.gm_last_error(self.env.ctx).decode() or f"{what} failed ({rc})")

    def _traj_ok(self, traj, noise=0.0):
        """The buffer's action width is this actor's (the library sees pointers only: a narrower
        buffer would be read or written past its end)."""
        want = 1 if self.categorical else self.env.n_actions
        if traj.act.shape[-1] != want:
            raise ValueError(f"a TrajectoryBuffer with act_dim = {want} expected, got {traj.act.shape[-1]}")
        if self.categorical and noise != 0:
            raise ValueError("a categorical actor takes no exploration noise (noise must be 0)")

    def set_params(self, params):
        """New weights after a learner update (flat, init_params' order, or a state dict)."""
        if isinstance(params, dict):
            if any(k.startswith("pi.logits_net.") for k in params) != self.categorical:
                raise ValueError("state dict of the other actor class (pi.mu_net / pi.logits_net)")
            asz, csz, params = params_from_state_dict(params)
            if asz != self.actor_sizes or csz != self.critic_sizes:
                raise ValueError("state dict does not match the network sizes")
        p = np.ascontiguousarray(params, np.float32)
        if p.size != self.params.size:
            raise ValueError(f"{self.params.size} parameters expected, got {p.size}")
        self.params = p.copy()
        self._check(self.lib.gm_ac_set_params(self._p, self.params.ctypes.data_as(C.POINTER(C.c_float))), "gm_ac_set_params")

    def get_params(self) -> np.ndarray:
        """The device's weights in init_params' flat order (the inverse of set_params), as a
        DevicePPOLearner's steps left them.  self.params keeps the last weights handed in."""
        out = np.empty(self.params.size, dtype=np.float32)
        self._check(self.lib.gm_ac_get_params(self._p, out.ctypes.data_as(C.POINTER(C.c_float))), "gm_ac_get_params")
        return out

    def get_packed(self) -> np.ndarray:
        """The device's weights as stored (pack()'s layout, padding entries included)."""
        out = np.empty(pack(self.actor_sizes, self.critic_sizes, self.params, self.categorical)[0].size, dtype=np.float32)
        self._check(self.lib.gm_ac_get_packed(self._p, out.ctypes.data_as(C.POINTER(C.c_float))), "gm_ac_get_packed")
        return out

    def state_dict(self) -> dict:
        """The device's weights under MLPActorCriticPG's key names (pi.log_std, pi.mu_net.{0,2,..}
        .weight / .bias, vf.v_net.{0,2,..}.weight / .bias) as numpy arrays: what
        params_from_state_dict and set_params read."""
        flat, pos, out = self.get_params(), 0, {}
        for prefix, sizes in ((self._actor_prefix, self.actor_sizes), ("vf.v_net.", self.critic_sizes)):
            for l in range(len(sizes) - 1):
                fin, fout = sizes[l], sizes[l + 1]
                out[f"{prefix}{2 * l}.weight"] = flat[pos:pos + fout * fin].reshape(fout, fin).copy()
                pos += fout * fin
                out[f"{prefix}{2 * l}.bias"] = flat[pos:pos + fout].copy()
                pos += fout
        if not self.categorical:
            out["pi.log_std"] = flat[pos:].copy()
        return out

    def act(self, traj: TrajectoryBuffer, k: int, sample: bool = True, noise: float = 0.0, seed: int = 0,
            decision: int = 0):
        """select_action for every env from its current observation into row k, applied on the device."""
        self._traj_ok(traj, noise)
        t = traj.struct()
        self._check(self.lib.gm_ac_act(self._p, C.byref(t), int(k), int(bool(sample)), C.c_float(noise),
                                       C.c_uint64(seed), C.c_uint64(decision)), "gm_ac_act")

    def record(self, traj: TrajectoryBuffer, k: int, max_episode_steps: int | None = None):
        """After the env-step, before the auto-reset: reward, end code and bootstrap value of row k."""
        mx = self.env.max_episode_steps if max_episode_steps is None else max_episode_steps
        t = traj.struct()
        self._check(self.lib.gm_ac_record(self._p, C.byref(t), int(k), int(mx)), "gm_ac_record")

    def finish(self, traj: TrajectoryBuffer, k_last: int | None = None):
        t = traj.struct()
        self._check(self.lib.gm_ac_finish(self._p, C.byref(t), int(traj.K - 1 if k_last is None else k_last)),
                    "gm_ac_finish")

    def rollout(self, traj: TrajectoryBuffer, n_steps: int | None = None, sample: bool = True, noise: float = 0.0,
                seed: int = 0, decision0: int = 0, max_episode_steps: int | None = None,
                records_dev_ptr: int | None = None, k0: int = 0):
        """gm_ac_rollout into rows k0 .. k0 + n_steps - 1: act(decision0 + i) -> env step -> record
        -> auto-reset for each, then finish, fused into one persistent launch (bit for bit the
        per-step sequence).  records_dev_ptr: device [n_steps x n_envs] gm_episode_end records."""
        n = traj.K - k0 if n_steps is None else int(n_steps)
        mx = self.env.max_episode_steps if max_episode_steps is None else max_episode_steps
        self._traj_ok(traj, noise)
        t = traj.struct(k0)
        self._check(self.lib.gm_ac_rollout(self._p, C.byref(t), n, int(bool(sample)), C.c_float(noise), C.c_uint64(seed),
                                           C.c_uint64(decision0), int(mx), C.c_void_p(records_dev_ptr or 0)),
                    "gm_ac_rollout")

    def evaluate(self, sample: bool = True, seed: int = 0, decision0: int = 0, max_episode_steps: int | None = None,
                 active=None, out=None) -> dict:
        """gm_ac_evaluate: one episode per active env, each env retiring at its episode's end
        (sample=True: the reference's PPO test mode, which still samples; False: mean / argmax); the
        test report as device tensors (gmx.eval).  No TrajectoryBuffer is written.  Reset the env
        before reuse."""
        from .eval import ac_evaluate
        return ac_evaluate(self, sample, seed, decision0, max_episode_steps, active, out)

    def gae(self, traj: TrajectoryBuffer, gamma: float = 0.99, lam: float = 0.97, n_steps: int | None = None):
        return traj.gae(gamma, lam, n_steps)

    def close(self):
        if self._p:
            self.lib.gm_ac_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceCategoricalActorCritic(DeviceActorCritic):
    """An MLPActorCriticPG(continous_actions=False) (categorical actor, critic) bound to a
    BatchedGripperEnv with discrete actions: the actor's outputs are logits, there is no log_std,
    the state dict's actor keys are pi.logits_net.*, the buffer is TrajectoryBuffer(env, K,
    act_dim=1) (the chosen index as a float; mu holds the logits) and noise must be 0.  sample=False
    takes the argmax.  Everything else, DevicePPOLearner included, is DeviceActorCritic's."""

    categorical = True
    _create = "gm_ac_create_categorical"
    _actor_prefix = "pi.logits_net."


_OPTIMISERS = {"adam": OPT_ADAM, "adamw": OPT_ADAMW}
# Agent_PPO.Parameters' learner options (PolicyGradient.py:1196-1220) and their defaults
PPO_DEFAULTS = dict(learning_rate_pi=3e-4, learning_rate_vf=1e-3, gamma=0.99, clip_ratio=0.2, train_pi_iters=80,
                    train_vf_iters=80, lam=0.97, target_kl=0.01, max_kl_ratio=1.5, optimiser="adam",
                    use_kl_penalty=False, use_entropy_regularisation=False, kl_penalty_coefficient=0.2,
                    entropy_coefficient=1e-4, adam_beta1=0.9, adam_beta2=0.999, grad_clamp_value=None)


def ppo_opt(**options) -> PpoOpt:
    """Agent_PPO.Parameters' learner options under their own names (PPO_DEFAULTS) as a gm_ppo_opt:
    "adam" is torch.optim.Adam(lr, betas), "adamW" torch.optim.AdamW(lr, betas, amsgrad=True), as
    Agent_PPO.init builds them; grad_clamp_value None disables the clamp.  Unknown names raise, as
    Parameters.update does.  No GPU needed."""
    unknown = sorted(set(options) - set(PPO_DEFAULTS))
    if unknown:
        raise ValueError(f"incorrect key: {', '.join(unknown)}")
    v = dict(PPO_DEFAULTS, **options)
    name = str(v["optimiser"]).lower()
    if name not in _OPTIMISERS:
        raise ValueError(f"optimiser {v['optimiser']!r}: 'adam' or 'adamW' expected (RMSprop is not on the device)")
    o = PpoOpt()
    for k in ("learning_rate_pi", "learning_rate_vf", "gamma", "lam", "clip_ratio", "target_kl", "max_kl_ratio",
              "kl_penalty_coefficient", "entropy_coefficient", "adam_beta1", "adam_beta2"):
        setattr(o, k, float(v[k]))
    o.train_pi_iters, o.train_vf_iters = int(v["train_pi_iters"]), int(v["train_vf_iters"])
    o.optimiser = _OPTIMISERS[name]
    o.use_kl_penalty, o.use_entropy_regularisation = int(bool(v["use_kl_penalty"])), int(bool(v["use_entropy_regularisation"]))
    o.grad_clamp_value = 0.0 if v["grad_clamp_value"] is None else float(v["grad_clamp_value"])
    return o


def ppo_opt_default() -> PpoOpt:
    """gm_ppo_opt_default: the library's own defaults (equal to ppo_opt()'s)."""
    o = PpoOpt()
    load_library().gm_ppo_opt_default(C.byref(o))
    return o


SCALARS = ("loss_pi", "loss_v", "kl", "ent", "cf")      # gm_ppo_learner_read's order


class DevicePPOLearner:
    """Agent_PPO.optimise_model on the device weights of `ac`: compute_loss_pi's and
    compute_loss_v's backward, pi_optimiser (actor net and log_std) and vf_optimiser (critic), the
    KL stop.  Options are Agent_PPO.Parameters' names (ppo_opt); n_groups: workgroups per gradient
    launch (None: the library's default) -- results are bit for bit reproducible for one n_groups."""

    def __init__(self, ac: DeviceActorCritic, n_groups: int | None = None, **options):
        self.ac, self.env, self.lib = ac, ac.env, ac.lib
        self.opt = ppo_opt(**options)
        self._l = C.c_void_p()
        self._check(self.lib.gm_ppo_learner_create(ac._p, C.byref(self.opt), int(n_groups or 0), C.byref(self._l)),
                    "gm_ppo_learner_create")

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(self.lib.gm_last_error(self.env.ctx).decode() or f"{what} failed ({rc})")

    def _handle(self):
        if not self._l:
            raise RuntimeError("the learner is closed")
        return self._l

    def _batch(self, data: dict, keys) -> PpoBatch:
        """The gm_ppo_batch of TrajectoryBuffer.get()'s dict (or any dict of contiguous f32 device
        tensors under those keys); the tensors named in `keys` are checked and passed."""
        import torch
        n = int(data["obs"].shape[0])
        want = dict(obs=(n, self.env.n_obs), act=(n, 1 if self.ac.categorical else self.env.n_actions), logp=(n,), adv=(n,), ret=(n,))
        b = PpoBatch()
        b.n = n
        for k in keys:
            t = data[k]
            if tuple(t.shape) != want[k] or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{k}: a contiguous float32 device tensor of shape {want[k]} expected, "
                                 f"got {tuple(t.shape)} {t.dtype} on {t.device}")
            setattr(b, k, t.data_ptr())
        return b

    def _grad(self, fn, name, data, keys):
        import torch
        h = self._handle()
        b = self._batch(data, keys)
        dev = data["obs"].device
        torch.cuda.synchronize(dev)     # torch-side writes to the batch
        self._check(fn(h, C.byref(b)), name)
        torch.cuda.synchronize(dev)     # the env's stream, before torch reuses the tensors

    def grad_pi(self, data: dict):
        """compute_loss_pi(data).backward(): leaves the policy's raw gradient, loss_pi, kl, ent, cf."""
        self._grad(self.lib.gm_ppo_learner_grad_pi, "gm_ppo_learner_grad_pi", data, ("obs", "act", "logp", "adv"))

    def grad_vf(self, data: dict):
        """compute_loss_v(data).backward(): leaves the critic's raw gradient and loss_v."""
        self._grad(self.lib.gm_ppo_learner_grad_vf, "gm_ppo_learner_grad_vf", data, ("obs", "ret"))

    def step_pi(self):
        """clip_grad_value_ and pi_optimiser.step() on the held gradient, in place on the actor and log_std."""
        self._check(self.lib.gm_ppo_learner_step_pi(self._handle()), "gm_ppo_learner_step_pi")

    def step_vf(self):
        """clip_grad_value_ and vf_optimiser.step() on the held gradient, in place on the critic."""
        self._check(self.lib.gm_ppo_learner_step_vf(self._handle()), "gm_ppo_learner_step_vf")

    def read(self):
        """(held gradient in init_params' flat order, dict of loss_pi, loss_v, kl, ent, cf as float32)."""
        g = np.empty(self.ac.params.size, dtype=np.float32)
        sc = np.empty(len(SCALARS), dtype=np.float32)
        f32p = C.POINTER(C.c_float)
        self._check(self.lib.gm_ppo_learner_read(self._handle(), g.ctypes.data_as(f32p), sc.ctypes.data_as(f32p)),
                    "gm_ppo_learner_read")
        return g, dict(zip(SCALARS, sc))

    def state(self) -> dict:
        """Both optimisers' state in flat order (the policy's entries pi_optimiser's, the critic's
        vf_optimiser's): step_pi, step_vf, exp_avg, exp_avg_sq, max_exp_avg_sq."""
        f32p = C.POINTER(C.c_float)
        n = self.ac.params.size
        steps = (C.c_int64 * 2)()
        out = {k: np.empty(n, dtype=np.float32) for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")}
        self._check(self.lib.gm_ppo_learner_get_state(self._handle(), steps, *(out[k].ctypes.data_as(f32p) for k in out)),
                    "gm_ppo_learner_get_state")
        return dict(step_pi=int(steps[0]), step_vf=int(steps[1]), **out)

    def load_state(self, state: dict):
        f32p = C.POINTER(C.c_float)
        n = self.ac.params.size
        arrs = [np.ascontiguousarray(as_f32(state[k]), np.float32).ravel()
                for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")]
        if any(a.size != n for a in arrs):
            raise ValueError(f"{n} entries per moment expected")
        steps = (C.c_int64 * 2)(int(state["step_pi"]), int(state["step_vf"]))
        self._check(self.lib.gm_ppo_learner_set_state(self._handle(), steps, *(a.ctypes.data_as(f32p) for a in arrs)),
                    "gm_ppo_learner_set_state")

    def update(self, traj: TrajectoryBuffer, n_steps: int | None = None) -> dict:
        """optimise_model on the first n_steps rows of traj (default: all), enqueued with one host
        read at the end: GAE -> advantage normalisation -> the policy loop with its KL stop -> the
        value loop.  Returns pi_iters_done and the first and last loss_pi, loss_v, kl, ent, cf."""
        import torch
        h = self._handle()
        k = traj.K if n_steps is None else int(n_steps)
        self.ac._traj_ok(traj)
        t = traj.struct()
        info = PpoInfo()
        torch.cuda.synchronize(traj.obs.device)     # torch-side writes to the buffers (tests)
        self._check(self.lib.gm_ppo_learner_update(h, C.byref(t), k, C.byref(info)), "gm_ppo_learner_update")
        return dict(pi_iters_done=int(info.pi_iters_done),
                    first=dict(zip(SCALARS, np.array(info.first[:], dtype=np.float32))),
                    last=dict(zip(SCALARS, np.array(info.last[:], dtype=np.float32))))

    def close(self):
        if self._l:
            self.lib.gm_ppo_learner_destroy(self._l)
            self._l = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
