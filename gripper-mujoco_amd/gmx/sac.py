"""On-device SAC for the batched env: the squashed Gaussian actor, a replay memory with float
action rows, the twin critics, the soft Bellman backup and the learner.

Mirrors the reference's soft actor-critic (rl/agents/ActorCritic.py):
  - SquashedGaussianMLPActor: mlp([n_obs, *hidden], act, act), then mu_layer and log_std_layer;
    log_std clamped to [-20, 2]; u = mu + std z (or mu); logp = Normal.log_prob(u).sum() -
    sum(2 (log 2 - u - softplus(-2 u))); a = action_limit tanh(u);
  - MLPQFunction x 2: mlp([n_obs + n_actions, *hidden, 1], act) on cat(obs, act);
  - Agent_SAC.select_action: uniform actions 2 U[0, 1) - 1 during the random start, the actor after;
  - Agent_SAC.update_step's push of (state, action, next_state, reward, terminal) as
    ActionReplayBuffer, filled by DeviceSAC.push_begin / push_end around an env-step or inside the
    fused launch (rollout(replay=buf));
  - compute_loss_q's backup, under no_grad, as DeviceSAC.target;
  - Agent_SAC.optimise_model (the backward of loss_q and loss_pi, q_optimiser and pi_optimiser,
    the polyak update) as DeviceSACLearner, in place on the device weights the rollout reads.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import (load_library, SacOpt, SacReplay, SacBatch, SacLearnOpt, SAC_MEAN, SAC_SAMPLE, SAC_RANDOM, ACT_RELU,
                   ACT_TANH, OPT_ADAM, OPT_ADAMW)
from .policy import as_f32, linear_init, state_dict_net
from .ppo import _counters, normal_draws        # noqa: F401  (normal_draws: the sampler's z, re-exported)

DEFAULT_HIDDEN = (256, 256)        # MLPActorCriticAC's default hidden_sizes
MAX_ACTIONS = 40                   # GA_MAX_ACT
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0

MODES = {"mean": SAC_MEAN, "sample": SAC_SAMPLE, "random": SAC_RANDOM}
_ACTIVATIONS = {"relu": ACT_RELU, "tanh": ACT_TANH}

# Agent_SAC.Parameters' names and defaults
SAC_DEFAULTS = dict(learning_rate=1e-4, gamma=0.99, alpha=0.2, batch_size=128, update_after_steps=1000,
                    update_every_steps=50, random_start_episodes=1000, min_memory_replay=250, memory_replay=10_000,
                    optimiser="adam", adam_beta1=0.9, adam_beta2=0.999, soft_target_tau=0.05)


def sac_options(**options) -> dict:
    """Agent_SAC.Parameters under their own names (SAC_DEFAULTS) with `options` applied.  Unknown
    names raise, as Parameters.update does.  No GPU needed."""
    unknown = sorted(set(options) - set(SAC_DEFAULTS))
    if unknown:
        raise ValueError(f"incorrect key: {', '.join(unknown)}")
    return dict(SAC_DEFAULTS, **options)


_OPTIMISERS = {"adam": OPT_ADAM, "adamw": OPT_ADAMW}
LEARNER_MAX_BATCH = 256     # GM_LEARNER_MAX_BATCH


def sac_opt(eps: float = 1e-8, weight_decay=None, amsgrad=None, **options) -> SacLearnOpt:
    """Agent_SAC.Parameters (by their own names, as sac_options takes them) as Agent_SAC.init hands
    them to torch, as a gm_sac_learn_opt: "adam" is torch.optim.Adam(lr, betas) -- weight_decay 0,
    no amsgrad; "adamW" is torch.optim.AdamW(lr, betas, amsgrad=True) -- weight_decay 0.01, torch's
    default.  weight_decay / amsgrad, when given, override that.  Unknown names raise as
    Parameters.update does; RMSprop is not on the device.  No GPU needed."""
    o = sac_options(**options)
    name = str(o["optimiser"]).lower()
    if name not in _OPTIMISERS:
        raise ValueError(f"optimiser {o['optimiser']!r}: 'adam' or 'adamW' expected (RMSprop is not on the device)")
    out = SacLearnOpt()
    out.optimiser = _OPTIMISERS[name]
    out.amsgrad = int(name == "adamw" if amsgrad is None else bool(amsgrad))
    out.lr, out.beta1, out.beta2, out.eps = (float(o["learning_rate"]), float(o["adam_beta1"]), float(o["adam_beta2"]),
                                             float(eps))
    out.weight_decay = float((0.01 if name == "adamw" else 0.0) if weight_decay is None else weight_decay)
    return out


def sac_opt_default() -> SacLearnOpt:
    """gm_sac_learn_opt_default: the library's own defaults (equal to sac_opt()'s)."""
    o = SacLearnOpt()
    load_library().gm_sac_learn_opt_default(C.byref(o))
    return o


def _mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(MODES)} expected")
        return MODES[mode]
    if int(mode) not in MODES.values():
        raise ValueError(f"mode {mode!r}: 0 (mean), 1 (sample) or 2 (random) expected")
    return int(mode)


def uniform_action_draws(seed, gids, decision, n_actions) -> np.ndarray:
    """The device's random-start actions 2 u3 - 1 in [-1, 1) (float64; exactly representable in
    float32: u3 has 24 bits) for global env ids `gids` at one decision index."""
    u3 = (_counters(seed, gids, decision, n_actions, 3) >> np.uint64(40)).astype(np.float64) / 16777216.0
    return 2.0 * u3 - 1.0


def sizes(n_obs: int, n_actions: int, hidden=DEFAULT_HIDDEN):
    """(pi_sizes, q_sizes) of MLPActorCriticAC(n_obs, n_actions, hidden)."""
    return [int(n_obs), *map(int, hidden), int(n_actions)], [int(n_obs) + int(n_actions), *map(int, hidden), 1]


def n_params(pi_sizes, q_sizes) -> int:
    """Floats of the flat parameters (init_params' order): the actor's hidden layers, its two
    heads, and the two critics."""
    hidden = sum(pi_sizes[i + 1] * pi_sizes[i] + pi_sizes[i + 1] for i in range(len(pi_sizes) - 2))
    heads = 2 * (pi_sizes[-1] * pi_sizes[-2] + pi_sizes[-1])
    q = sum(q_sizes[i + 1] * q_sizes[i] + q_sizes[i + 1] for i in range(len(q_sizes) - 1))
    return hidden + heads + 2 * q


def init_params(pi_sizes, q_sizes, seed: int = 0) -> np.ndarray:
    """nn.Linear's default init for every layer, flattened in MLPActorCriticAC's parameters()
    order: pi hidden layers W [out x in], b, ..., mu_layer W, b, log_std_layer W, b, q1's layers,
    q2's layers."""
    rng = np.random.default_rng(seed)
    parts = linear_init(rng, pi_sizes[:-1]) if len(pi_sizes) > 2 else []
    parts += linear_init(rng, pi_sizes[-2:]) + linear_init(rng, pi_sizes[-2:])
    parts += linear_init(rng, q_sizes) + linear_init(rng, q_sizes)
    return np.concatenate(parts).astype(np.float32)


def _layer_keys(prefix, n_layers):
    return [f"{prefix}{2 * l}" for l in range(n_layers)]


def params_from_state_dict(state_dict):
    """(pi_sizes, q_sizes, flat params) from an MLPActorCriticAC state dict: pi.net.{0,2,..},
    pi.mu_layer, pi.log_std_layer, q1.q.{0,2,..}, q2.q.{0,2,..} (.weight / .bias each)."""
    def net(prefix):
        ws = sorted((k for k in state_dict if k.startswith(prefix) and k.endswith(".weight")),
                    key=lambda k: int(k[len(prefix):].split(".")[0]))
        if not ws:
            raise KeyError(f"no {prefix}*.weight in the state dict")
        return state_dict_net(state_dict, ws)
    hsz, hp = net("pi.net.")
    msz, mp = state_dict_net(state_dict, ["pi.mu_layer.weight"])
    lsz, lp = state_dict_net(state_dict, ["pi.log_std_layer.weight"])
    q1sz, q1p = net("q1.q.")
    q2sz, q2p = net("q2.q.")
    if msz != lsz or msz[0] != hsz[-1] or q1sz != q2sz:
        raise ValueError("the heads or the two critics have different sizes")
    return hsz + [msz[1]], q1sz, np.concatenate(hp + mp + lp + q1p + q2p).astype(np.float32)


def flat_to_state_dict(pi_sizes, q_sizes, flat) -> dict:
    """The inverse of params_from_state_dict: numpy arrays under MLPActorCriticAC's key names."""
    flat = np.asarray(flat, dtype=np.float32).ravel()
    if flat.size != n_params(pi_sizes, q_sizes):
        raise ValueError(f"{n_params(pi_sizes, q_sizes)} parameters expected for these sizes, got {flat.size}")
    out, pos = {}, 0

    def take(key, fin, fout):
        nonlocal pos
        out[key + ".weight"] = flat[pos:pos + fout * fin].reshape(fout, fin).copy()
        pos += fout * fin
        out[key + ".bias"] = flat[pos:pos + fout].copy()
        pos += fout
    for l, key in enumerate(_layer_keys("pi.net.", len(pi_sizes) - 2)):
        take(key, pi_sizes[l], pi_sizes[l + 1])
    take("pi.mu_layer", pi_sizes[-2], pi_sizes[-1])
    take("pi.log_std_layer", pi_sizes[-2], pi_sizes[-1])
    for q in ("q1.q.", "q2.q."):
        for l, key in enumerate(_layer_keys(q, len(q_sizes) - 1)):
            take(key, q_sizes[l], q_sizes[l + 1])
    return out


def pack(pi_sizes, q_sizes, params, activation="relu"):
    """(packed blob, q1 offset, q2 offset): the device layout [pi | q1 | q2] (gm_sac_pack; testable
    without a GPU); pi is one MLP whose output layer is mu_layer stacked over log_std_layer.
    Raises ValueError for unsupported sizes or a wrong parameter count."""
    lib = load_library()
    a = np.ascontiguousarray(pi_sizes, dtype=np.int32)
    c = np.ascontiguousarray(q_sizes, dtype=np.int32)
    pr = np.ascontiguousarray(params, dtype=np.float32).ravel()
    act = _ACTIVATIONS[activation] if isinstance(activation, str) else int(activation)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    off = (C.c_int64 * 2)()
    n = lib.gm_sac_pack(a.ctypes.data_as(i32p), len(a), c.ctypes.data_as(i32p), len(c), act, pr.ctypes.data_as(f32p),
                        None, off)
    if n < 0:
        raise ValueError("unsupported network sizes")
    want = n_params([int(x) for x in a], [int(x) for x in c])
    if pr.size != want:
        raise ValueError(f"{want} parameters expected for these sizes, got {pr.size}")
    out = np.zeros(n, dtype=np.float32)
    lib.gm_sac_pack(a.ctypes.data_as(i32p), len(a), c.ctypes.data_as(i32p), len(c), act, pr.ctypes.data_as(f32p),
                    out.ctypes.data_as(f32p), off)
    return out, int(off[0]), int(off[1])


def _batch_struct(batch: dict) -> SacBatch:
    b = SacBatch()
    for name, _ in SacBatch._fields_:
        t = batch.get(name)
        setattr(b, name, t.data_ptr() if t is not None else None)
    return b


class ActionReplayBuffer:
    """Agent_SAC's ReplayMemory as torch tensors on the env's device in gm_sac_replay's layout: a
    ring of `capacity` transitions whose action is a float row, `pushed` counting every transition
    ever written."""

    def __init__(self, env, capacity: int):
        import torch
        self.env = env
        self.capacity = int(capacity)
        if self.capacity < env.n_envs:
            raise ValueError(f"capacity {self.capacity} holds less than one env-step of {env.n_envs} envs")
        self.pushed = 0
        dev = f"cuda:{env.device}"
        f = dict(dtype=torch.float32, device=dev)
        self.state = torch.zeros((self.capacity, env.n_obs), **f)
        self.action = torch.zeros((self.capacity, env.n_actions), **f)
        self.next_state = torch.zeros((self.capacity, env.n_obs), **f)
        self.reward = torch.zeros((self.capacity,), **f)
        self.end = torch.zeros((self.capacity,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)    # the zero fills, before the env's own stream writes

    def __len__(self):
        return min(self.pushed, self.capacity)

    def struct(self) -> SacReplay:
        r = SacReplay()
        r.capacity = self.capacity
        for name in ("state", "action", "next_state", "reward", "end"):
            setattr(r, name, getattr(self, name).data_ptr())
        return r

    def sample(self, batch: int, seed: int = 0, draw: int = 0) -> dict:
        """ReplayMemory.batch: `batch` distinct stored transitions (gmx.policy.replay_indices(len(self),
        batch, seed, draw)) gathered on the device: a dict of tensors state, action, next_state,
        reward, end and index."""
        import torch
        batch = int(batch)
        if not 1 <= batch <= len(self):
            raise ValueError(f"batch {batch} of {len(self)} stored transitions")
        dev = self.state.device
        f = dict(dtype=torch.float32, device=dev)
        out = dict(state=torch.empty((batch, self.state.shape[1]), **f),
                   action=torch.empty((batch, self.action.shape[1]), **f),
                   next_state=torch.empty((batch, self.state.shape[1]), **f),
                   reward=torch.empty((batch,), **f),
                   end=torch.empty((batch,), dtype=torch.uint8, device=dev),
                   index=torch.empty((batch,), dtype=torch.int32, device=dev))
        r, b = self.struct(), _batch_struct(out)
        torch.cuda.synchronize(dev)     # torch-side writes to the rows (tests), the allocations
        rc = self.env.lib.gm_sac_replay_sample(self.env.ctx, C.byref(r), len(self), batch, C.c_uint64(seed),
                                               C.c_uint64(draw), C.byref(b))
        if rc != 0:
            raise RuntimeError(self.env.lib.gm_last_error(self.env.ctx).decode() or f"gm_sac_replay_sample failed ({rc})")
        torch.cuda.synchronize(dev)     # the env's stream, before torch reads the batch
        return out


class DeviceSAC:
    """An MLPActorCriticAC (squashed Gaussian actor, two Q critics) bound to a BatchedGripperEnv
    with continuous actions.  A target network is a second DeviceSAC built from the same params."""

    def __init__(self, env, hidden=DEFAULT_HIDDEN, params=None, seed: int = 0, activation="relu",
                 action_limit: float = 1.0, log_std_min: float = LOG_STD_MIN, log_std_max: float = LOG_STD_MAX):
        self.env = env
        self.lib = env.lib
        self._p = C.c_void_p()
        if str(activation).lower() not in _ACTIVATIONS:
            raise ValueError(f"activation {activation!r}: 'relu' or 'tanh' expected")
        self.activation = str(activation).lower()
        self.action_limit = float(action_limit)
        self.pi_sizes, self.q_sizes = sizes(env.n_obs, env.n_actions, hidden)
        if min(self.pi_sizes) < 1:
            raise ValueError("layer sizes must be positive")
        #: the last weights handed in from the host (the constructor's, set_params')
        self.params = (init_params(self.pi_sizes, self.q_sizes, seed) if params is None
                       else np.ascontiguousarray(as_f32(params), np.float32).ravel().copy())
        want = n_params(self.pi_sizes, self.q_sizes)
        if self.params.size != want:      # (the library reads exactly this many)
            raise ValueError(f"{want} parameters expected for these sizes, got {self.params.size}")
        self.opt = SacOpt(_ACTIVATIONS[self.activation], float(action_limit), float(log_std_min), float(log_std_max))
        a = np.ascontiguousarray(self.pi_sizes, dtype=np.int32)
        c = np.ascontiguousarray(self.q_sizes, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        rc = self.lib.gm_sac_create(env.ctx, a.ctypes.data_as(i32p), len(a), c.ctypes.data_as(i32p), len(c),
                                    C.byref(self.opt), self.params.ctypes.data_as(C.POINTER(C.c_float)),
                                    C.byref(self._p))
        if rc != 0:
            raise RuntimeError(self.lib.gm_last_error(env.ctx).decode() or f"gm_sac_create failed ({rc})")

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(self.lib.gm_last_error(self.env.ctx).decode() or f"{what} failed ({rc})")

    def set_params(self, params):
        """New weights (flat, init_params' order, or an MLPActorCriticAC state dict)."""
        if isinstance(params, dict):
            psz, qsz, params = params_from_state_dict(params)
            if psz != self.pi_sizes or qsz != self.q_sizes:
                raise ValueError("state dict does not match the network sizes")
        p = np.ascontiguousarray(as_f32(params), np.float32).ravel()
        if p.size != self.params.size:
            raise ValueError(f"{self.params.size} parameters expected, got {p.size}")
        self.params = p.copy()
        self._check(self.lib.gm_sac_set_params(self._p, self.params.ctypes.data_as(C.POINTER(C.c_float))),
                    "gm_sac_set_params")

    def get_params(self) -> np.ndarray:
        """The device's weights in init_params' flat order (the inverse of set_params)."""
        out = np.empty(self.params.size, dtype=np.float32)
        self._check(self.lib.gm_sac_get_params(self._p, out.ctypes.data_as(C.POINTER(C.c_float))), "gm_sac_get_params")
        return out

    def get_packed(self) -> np.ndarray:
        """The device's weights as stored (pack()'s layout, padding entries included)."""
        out = np.empty(pack(self.pi_sizes, self.q_sizes, self.params, self.activation)[0].size, dtype=np.float32)
        self._check(self.lib.gm_sac_get_packed(self._p, out.ctypes.data_as(C.POINTER(C.c_float))), "gm_sac_get_packed")
        return out

    def state_dict(self) -> dict:
        """The device's weights under MLPActorCriticAC's key names as numpy arrays: what
        params_from_state_dict and set_params read."""
        return flat_to_state_dict(self.pi_sizes, self.q_sizes, self.get_params())

    def act(self, mode="sample", seed: int = 0, decision: int = 0):
        """select_action for every env from its current observation, applied on the device.
        mode: "mean" (deterministic), "sample", or "random" (the random start: uniform actions, the
        net is not consulted)."""
        self._check(self.lib.gm_sac_act(self._p, _mode(mode), C.c_uint64(seed), C.c_uint64(decision)), "gm_sac_act")

    def read(self) -> dict:
        """What the last act() left: act, u, mu, log_std [n_envs, n_actions] and logp [n_envs]."""
        n, a = self.env.n_envs, self.env.n_actions
        out = {k: np.zeros((n, a), dtype=np.float32) for k in ("act", "u", "mu", "log_std")}
        out["logp"] = np.zeros(n, dtype=np.float32)
        f32p = C.POINTER(C.c_float)
        self._check(self.lib.gm_sac_read(self._p, *(out[k].ctypes.data_as(f32p) for k in ("act", "logp", "u", "mu", "log_std"))),
                    "gm_sac_read")
        return out

    def push_begin(self, buf: ActionReplayBuffer):
        """After act(): state and action row of every env into the ring rows from buf.pushed on."""
        r = buf.struct()
        self._check(self.lib.gm_sac_push_begin(self._p, C.byref(r), buf.pushed), "gm_sac_push_begin")

    def push_end(self, buf: ActionReplayBuffer, max_episode_steps: int | None = None):
        """After the env-step, before the auto-reset: next_state, reward and end code into the rows
        push_begin wrote; advances buf.pushed by n_envs."""
        mx = self.env.max_episode_steps if max_episode_steps is None else max_episode_steps
        r = buf.struct()
        self._check(self.lib.gm_sac_push_end(self._p, C.byref(r), buf.pushed, int(mx)), "gm_sac_push_end")
        buf.pushed += self.env.n_envs

    def rollout(self, n_steps: int, mode="sample", seed: int = 0, decision0: int = 0,
                max_episode_steps: int | None = None, records_dev_ptr: int | None = None,
                replay: ActionReplayBuffer | None = None):
        """gm_sac_rollout: n_steps rounds of act(mode, seed, decision0 + k) -> push_begin -> env step
        -> push_end -> auto-reset, fused into one persistent launch (bit for bit the per-step
        sequence).  records_dev_ptr: device [n_steps x n_envs] gm_episode_end records (or None).
        replay: the memory to push every transition into (advances replay.pushed), or None."""
        mx = self.env.max_episode_steps if max_episode_steps is None else max_episode_steps
        r = replay.struct() if replay is not None else None
        self._check(self.lib.gm_sac_rollout(self._p, int(n_steps), _mode(mode), C.c_uint64(seed), C.c_uint64(decision0),
                                            int(mx), C.c_void_p(records_dev_ptr or 0),
                                            C.byref(r) if r is not None else None,
                                            replay.pushed if replay is not None else 0), "gm_sac_rollout")
        if replay is not None:
            replay.pushed += int(n_steps) * self.env.n_envs

    def evaluate(self, mode="mean", seed: int = 0, decision0: int = 0, max_episode_steps: int | None = None,
                 active=None, out=None) -> dict:
        """gm_sac_evaluate: one episode per active env, each env retiring at its episode's end; the
        test report as device tensors (gmx.eval).  No memory is written.  Reset the env before reuse."""
        from .eval import sac_evaluate
        return sac_evaluate(self, mode, seed, decision0, max_episode_steps, active, out)

    @staticmethod
    def _f32_dev(t, shape, name):
        import torch
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{name}: a contiguous float32 device tensor of shape {shape} expected, "
                             f"got {tuple(t.shape)} {t.dtype} on {t.device}")

    def q(self, batch: dict):
        """(q1, q2) device tensors [n] of both critics on (batch["state"], batch["action"])."""
        import torch
        st, ac = batch["state"], batch["action"]
        n = int(st.shape[0])
        self._f32_dev(st, (n, self.env.n_obs), "state")
        self._f32_dev(ac, (n, self.env.n_actions), "action")
        q1 = torch.empty((n,), dtype=torch.float32, device=st.device)
        q2 = torch.empty((n,), dtype=torch.float32, device=st.device)
        torch.cuda.synchronize(st.device)     # torch-side writes to the batch, the allocations
        self._check(self.lib.gm_sac_q(self._p, C.c_void_p(st.data_ptr()), C.c_void_p(ac.data_ptr()), n,
                                      C.c_void_p(q1.data_ptr()), C.c_void_p(q2.data_ptr())), "gm_sac_q")
        torch.cuda.synchronize(st.device)     # the env's stream, before torch reads the results
        return q1, q2

    def target(self, batch: dict, gamma: float = SAC_DEFAULTS["gamma"], alpha: float = SAC_DEFAULTS["alpha"],
               online: "DeviceSAC | None" = None, bootstrap_truncated: bool = False, seed: int = 0, draw: int = 0,
               debug: bool = False):
        """compute_loss_q's backup for a sampled batch (next_state, reward and end are read), self
        being the target network and `online` (default: self) the one whose actor samples a2:
        y = reward + gamma (min(q1_targ, q2_targ)(next_state, a2) - alpha logp2) where the row
        bootstraps (end == 0, or end == 2 with bootstrap_truncated), y = reward where not.  Row i
        draws with (seed, i, draw): pass a seed other than the rollout's.  Returns y, a device
        tensor [n]; with debug, (y, dict of a2, u2, logp2, qmin)."""
        import torch
        onl = self if online is None else online
        n = int(batch["reward"].shape[0])
        dev = batch["reward"].device
        self._f32_dev(batch["next_state"], (n, self.env.n_obs), "next_state")
        f = dict(dtype=torch.float32, device=dev)
        y = torch.empty((n,), **f)
        dbg = {}
        if debug:
            dbg = dict(a2=torch.empty((n, self.env.n_actions), **f), u2=torch.empty((n, self.env.n_actions), **f),
                       logp2=torch.empty((n,), **f), qmin=torch.empty((n,), **f))
        b = _batch_struct(batch)
        ptr = {k: C.c_void_p(dbg[k].data_ptr()) if debug else None for k in ("a2", "u2", "logp2", "qmin")}
        torch.cuda.synchronize(dev)     # torch-side writes to the batch, the allocations
        self._check(self.lib.gm_sac_target(self._p, onl._p, C.byref(b), n, C.c_float(gamma), C.c_float(alpha),
                                           int(bool(bootstrap_truncated)), C.c_uint64(seed), C.c_uint64(draw),
                                           C.c_void_p(y.data_ptr()), ptr["a2"], ptr["u2"], ptr["logp2"], ptr["qmin"]),
                    "gm_sac_target")
        torch.cuda.synchronize(dev)     # the env's stream, before torch reads the results
        return (y, dbg) if debug else y

    def soft_update(self, online: "DeviceSAC", tau: float):
        """self <- tau online + (1 - tau) self over all three nets, on the device (optimise_model's
        polyak update, self being mlp_ac_targ); tau = 1 copies online bit for bit."""
        self._check(self.lib.gm_sac_soft_update(self._p, online._p, C.c_float(tau)), "gm_sac_soft_update")

    def close(self):
        if self._p:
            self.lib.gm_sac_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceSACLearner:
    """Agent_SAC.optimise_model on the device weights of `sac` (mlp_ac) and `target` (mlp_ac_targ):
    loss_q's backward and q_optimiser on [q1 | q2], loss_pi's backward through the frozen critics
    and pi_optimiser on [pi], the polyak update of all three nets.  Options are Agent_SAC.Parameters'
    names (sac_opt reads learning_rate, optimiser, adam_beta1, adam_beta2; train() reads gamma,
    alpha, batch_size and soft_target_tau) plus bootstrap_truncated (DeviceSAC.target's) and
    sac_opt's eps / weight_decay / amsgrad."""

    def __init__(self, sac: DeviceSAC, target: DeviceSAC | None = None, bootstrap_truncated: bool = False,
                 eps: float = 1e-8, weight_decay=None, amsgrad=None, **options):
        self.sac, self.target = sac, target
        self.env, self.lib = sac.env, sac.lib
        self.options = sac_options(**options)
        self.bootstrap_truncated = bool(bootstrap_truncated)
        self.opt = sac_opt(eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **options)
        self._l = C.c_void_p()
        self._check(self.lib.gm_sac_learner_create(sac._p, C.byref(self.opt), C.byref(self._l)), "gm_sac_learner_create")

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(self.lib.gm_last_error(self.env.ctx).decode() or f"{what} failed ({rc})")

    def grad_q(self, batch: dict, y):
        """loss_q.backward() for a sampled batch (state and action are read) and its backup y (a
        device tensor [n], DeviceSAC.target's): leaves the raw gradient of [q1 | q2] and loss_q on
        the device."""
        import torch
        n = int(y.shape[0])
        b = _batch_struct(batch)
        torch.cuda.synchronize(y.device)     # torch-side writes to the batch and y
        self._check(self.lib.gm_sac_learner_grad_q(self._l, C.byref(b), C.c_void_p(y.data_ptr()), n),
                    "gm_sac_learner_grad_q")
        torch.cuda.synchronize(y.device)     # the env's stream, before torch reuses the tensors

    def grad_pi(self, batch: dict, alpha: float | None = None, seed: int = 0, draw: int = 0, debug: bool = False):
        """loss_pi.backward() for a sampled batch (state is read) with the critics as they stand,
        row i drawing with (seed, i, draw): leaves the raw gradient of [pi] and loss_pi on the
        device.  With debug, returns a dict of device tensors z, u, a [n, n_actions] and logp, q1,
        q2 [n]: the draws, the pre-squash sample, the action, its log-probability and both critics."""
        import torch
        st = batch["state"]
        n, na = int(st.shape[0]), self.env.n_actions
        alpha = self.options["alpha"] if alpha is None else alpha
        f = dict(dtype=torch.float32, device=st.device)
        dbg = {}
        if debug:
            dbg = {k: torch.empty((n, na), **f) for k in ("z", "u", "a")}
            dbg.update({k: torch.empty((n,), **f) for k in ("logp", "q1", "q2")})
        ptr = [C.c_void_p(dbg[k].data_ptr()) if debug else None for k in ("z", "u", "a", "logp", "q1", "q2")]
        b = _batch_struct(batch)
        torch.cuda.synchronize(st.device)    # torch-side writes to the batch, the allocations
        self._check(self.lib.gm_sac_learner_grad_pi(self._l, C.byref(b), n, C.c_float(alpha), C.c_uint64(seed),
                                                    C.c_uint64(draw), *ptr), "gm_sac_learner_grad_pi")
        torch.cuda.synchronize(st.device)    # the env's stream, before torch reads the outputs
        return dbg if debug else None

    def step_q(self):
        """q_optimiser.step() on the held gradient, in place on [q1 | q2] of `sac`."""
        self._check(self.lib.gm_sac_learner_step_q(self._l), "gm_sac_learner_step_q")

    def step_pi(self):
        """pi_optimiser.step() on the held gradient, in place on [pi] of `sac`."""
        self._check(self.lib.gm_sac_learner_step_pi(self._l), "gm_sac_learner_step_pi")

    def read(self):
        """(both gradients as one array in init_params' flat order, loss_q, loss_pi) as the last
        grad_q() / grad_pi() / update left them."""
        g = np.empty(self.sac.params.size, dtype=np.float32)
        lq, lp = C.c_float(), C.c_float()
        self._check(self.lib.gm_sac_learner_read(self._l, g.ctypes.data_as(C.POINTER(C.c_float)), C.byref(lq),
                                                 C.byref(lp)), "gm_sac_learner_read")
        return g, float(lq.value), float(lp.value)

    def state(self) -> dict:
        """Both optimisers' state in flat order, like their state_dict()s' tensors: step_q, step_pi,
        exp_avg, exp_avg_sq, max_exp_avg_sq (one array each: the critics' part is q_optimiser's)."""
        f32p = C.POINTER(C.c_float)
        n = self.sac.params.size
        steps = (C.c_int64 * 2)()
        out = {k: np.empty(n, dtype=np.float32) for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")}
        self._check(self.lib.gm_sac_learner_get_state(self._l, steps, *(out[k].ctypes.data_as(f32p) for k in out)),
                    "gm_sac_learner_get_state")
        return dict(step_q=int(steps[0]), step_pi=int(steps[1]), **out)

    def load_state(self, state: dict):
        f32p = C.POINTER(C.c_float)
        n = self.sac.params.size
        arrs = [np.ascontiguousarray(as_f32(state[k]), np.float32).ravel()
                for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")]
        if any(a.size != n for a in arrs):
            raise ValueError(f"{n} entries per moment expected")
        steps = (C.c_int64 * 2)(int(state["step_q"]), int(state["step_pi"]))
        self._check(self.lib.gm_sac_learner_set_state(self._l, steps, *(a.ctypes.data_as(f32p) for a in arrs)),
                    "gm_sac_learner_set_state")

    def train(self, buf: ActionReplayBuffer, n_updates: int, batch_size: int | None = None, seed: int = 0,
              noise_seed: int = 1, draw0: int = 0, tau: float | None = None):
        """n_updates of optimise_model enqueued back to back: sample(draw0 + u) -> backup -> critic
        gradient and step -> actor gradient and step -> polyak update.  The backup's noise is keyed
        (noise_seed, 2 (draw0 + u)), the actor loss's (noise_seed, 2 (draw0 + u) + 1).  tau: the
        polyak factor (default soft_target_tau; 0 leaves the target alone).  Returns (loss_q,
        loss_pi) of every update as a device tensor [n_updates, 2]."""
        import torch
        if self.target is None:
            raise ValueError("train() needs the target handle")
        dev = buf.state.device
        o = self.options
        losses = torch.empty((int(n_updates), 2), dtype=torch.float32, device=dev)
        r = buf.struct()
        torch.cuda.synchronize(dev)     # torch-side writes to the memory (tests), the allocation
        self._check(self.lib.gm_sac_learner_train(
            self._l, self.target._p, C.byref(r), len(buf), int(o["batch_size"] if batch_size is None else batch_size),
            C.c_uint64(seed), C.c_uint64(noise_seed), C.c_uint64(draw0), int(n_updates), C.c_float(o["gamma"]),
            C.c_float(o["alpha"]), int(self.bootstrap_truncated), C.c_float(o["soft_target_tau"] if tau is None else tau),
            C.c_void_p(losses.data_ptr())), "gm_sac_learner_train")
        torch.cuda.synchronize(dev)     # the env's stream, before torch reads the losses
        return losses

    def close(self):
        if self._l:
            self.lib.gm_sac_learner_destroy(self._l)
            self._l = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
