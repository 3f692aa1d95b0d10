"""On-device DQN action selection for the batched env.

Mirrors the reference's policy side of the rollout:
  - VariableNetwork (rl/networks.py:7-41): Linear + ReLU per hidden layer, a final
    Linear, Softmax(dim=1); canonical layers [n_obs, 150, 100, 50, n_actions]
    (launch_training.py:850-857);
  - Agent_DQN.select_action (rl/agents/DQN.py:184-209): eps_threshold =
    eps_end + (eps_start - eps_end) exp(-decay_num / eps_decay); a uniform random
    action with that probability, otherwise the argmax of the network output.
The forward pass and the choice run in one HIP kernel (gm_policy_kernel, f32 MFMA) on
the env's device observations and the chosen actions are applied on the device.

The data plumbing of training sits next to it, on the device too:
  - ReplayMemory (DQN.py:11-62) as ReplayBuffer, pushed by DevicePolicy.push_begin / push_end
    around an env-step or inside the fused launch (rollout(replay=buf)), sampled without
    replacement by ReplayBuffer.sample;
  - optimise_model's TD target (DQN.py:294-315), plain or double, as DevicePolicy.td_target.
The learning step is here as well:
  - optimise_model from the loss on (DQN.py:317-327: smooth-L1 / MSE loss, backward,
    clip_grad_value_, Adam / AdamW step) as DeviceLearner.grad / step, on the packed device
    weights the rollout reads, and update_step's soft target update (DQN.py:352-360) as
    DevicePolicy.soft_update;
  - DeviceLearner.train enqueues whole updates (sample -> TD target -> gradient -> step -> soft
    update) with no host synchronisation between them, so a training loop is
    rollout(replay=buf) followed by learner.train(buf, n_updates) and no weight crosses the bus.
DevicePolicy.get_params() reads the device's weights back; set_params() remains for weights that
come from elsewhere (a checkpoint, a torch optimiser of the user's own).  RMSprop and
update_episode's hard-copy schedule are not here; a hard copy is soft_update(online, tau=1).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._lib import load_library, DqnOpt, OPT_ADAM, OPT_ADAMW, LOSS_SMOOTH_L1, LOSS_MSE

CANONICAL_HIDDEN = (150, 100, 50)

_M64 = (1 << 64) - 1


def _mix(z):
    """gp_mix (csrc/gm_policy_net.h): splitmix64's finaliser on uint64 arrays."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def replay_indices(size: int, batch: int, seed: int = 0, draw: int = 0) -> np.ndarray:
    """The numpy mirror of gm_replay_indices (csrc/gm_replay.h gr_index): `batch` distinct rows of
    [0, size) -- index i is the image of i under a 4-round balanced Feistel network over the
    smallest even bit count b with 2^b >= size, keyed by (seed, draw), cycle-walked into range."""
    size, batch = int(size), int(batch)
    if size < 1 or not 0 <= batch <= size:
        raise ValueError(f"0 <= batch <= size and size >= 1 expected, got batch {batch}, size {size}")
    h = 0
    while (1 << (2 * h)) < size:
        h += 1
    mask = np.uint64((1 << h) - 1)
    sh = np.uint64(h)
    key = _mix(np.uint64(int(seed) & _M64) ^ _mix(np.uint64(int(draw) & _M64)))
    x = np.arange(batch, dtype=np.uint64)
    walk = np.ones(batch, dtype=bool)
    while walk.any():
        L, R = x[walk] >> sh, x[walk] & mask
        for r in range(4):
            with np.errstate(over="ignore"):
                f = _mix(key + np.uint64(((r + 1) * 0xD1B54A32D192ED03) & _M64) + R) & mask
            L, R = R, L ^ f
        x[walk] = (L << sh) | R
        walk = x >= np.uint64(size)
    return x.astype(np.int32)


def ring_rows(row0: int, n_steps: int, n_envs: int, capacity: int) -> np.ndarray:
    """[n_steps, n_envs] ring rows a call writes that starts after row0 pushed transitions: env e
    at env-step k goes to (row0 + k * n_envs + e) % capacity (include/gripper_mi355x.h gm_replay)."""
    if n_steps * n_envs > capacity:
        raise ValueError("the call would write a row twice")
    return (int(row0) + np.arange(n_steps * n_envs, dtype=np.int64).reshape(n_steps, n_envs)) % int(capacity)


def eps_threshold(decay_num: int, eps_start: float = 0.9, eps_end: float = 0.05, eps_decay: int = 1000) -> float:
    """Agent_DQN.select_action's exploration threshold (DQN.py:195-198; defaults DQN.py:75-77)."""
    return eps_end + (eps_start - eps_end) * math.exp(-1.0 * decay_num / float(eps_decay))


def linear_init(rng, sizes) -> list:
    """nn.Linear's default init (kaiming-uniform weights, U(+-1/sqrt(fan_in)) biases) for
    every layer of one net, drawn from rng in state_dict order: [W0 [out x in], b0, W1, b1, ...]"""
    parts = []
    for i in range(len(sizes) - 1):
        fan_in, fan_out = sizes[i], sizes[i + 1]
        bound = 1.0 / math.sqrt(fan_in)
        parts.append(rng.uniform(-bound, bound, size=(fan_out, fan_in)).astype(np.float32).ravel())
        parts.append(rng.uniform(-bound, bound, size=fan_out).astype(np.float32))
    return parts


def init_params(sizes, seed: int = 0) -> np.ndarray:
    """linear_init for every layer, flattened: W0 [out x in], b0, W1, b1, ..."""
    return np.concatenate(linear_init(np.random.default_rng(seed), sizes)).astype(np.float32)


def as_f32(t) -> np.ndarray:
    """A torch tensor or array-like as a float32 numpy array."""
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)


def state_dict_net(state_dict, weight_keys) -> tuple[list[int], list]:
    """(sizes, [W0, b0, W1, b1, ...]) of one net from its *.weight keys in layer order."""
    sizes = [int(state_dict[weight_keys[0]].shape[1])]
    parts = []
    for k in weight_keys:
        w = as_f32(state_dict[k])
        sizes.append(int(w.shape[0]))
        parts += [w.ravel(), as_f32(state_dict[k[:-len("weight")] + "bias"]).ravel()]
    return sizes, parts


def params_from_state_dict(state_dict) -> tuple[list[int], np.ndarray]:
    """(sizes, flat params) from a VariableNetwork state_dict (linear.i.weight / .bias)."""
    ws = sorted((k for k in state_dict if k.endswith(".weight")), key=lambda k: int(k.split(".")[1]))
    sizes, parts = state_dict_net(state_dict, ws)
    return sizes, np.concatenate(parts).astype(np.float32)


def pack(sizes, params) -> np.ndarray:
    """The device layout of the parameters (gm_policy_pack; testable without a GPU)."""
    lib = load_library()
    sz = np.ascontiguousarray(sizes, dtype=np.int32)
    pr = np.ascontiguousarray(params, dtype=np.float32)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    n = lib.gm_policy_pack(sz.ctypes.data_as(i32p), len(sz), pr.ctypes.data_as(f32p), None)
    if n < 0:
        raise ValueError("unsupported network sizes")
    out = np.zeros(n, dtype=np.float32)
    lib.gm_policy_pack(sz.ctypes.data_as(i32p), len(sz), pr.ctypes.data_as(f32p), out.ctypes.data_as(f32p))
    return out


class Replay(C.Structure):
    """gm_replay (include/gripper_mi355x.h)."""
    _fields_ = [("capacity", C.c_int64), ("state", C.c_void_p), ("action", C.c_void_p), ("next_state", C.c_void_p),
                ("reward", C.c_void_p), ("end", C.c_void_p)]


class ReplayBatch(C.Structure):
    """gm_replay_batch (include/gripper_mi355x.h)."""
    _fields_ = [("state", C.c_void_p), ("action", C.c_void_p), ("next_state", C.c_void_p), ("reward", C.c_void_p),
                ("end", C.c_void_p), ("index", C.c_void_p)]


def _batch_struct(batch: dict) -> ReplayBatch:
    b = ReplayBatch()
    for name, _ in ReplayBatch._fields_:
        t = batch.get(name)
        setattr(b, name, t.data_ptr() if t is not None else None)
    return b


class ReplayBuffer:
    """ReplayMemory (rl/agents/DQN.py:11-62) as torch tensors on the env's device in gm_replay's
    layout: a ring of `capacity` transitions, `pushed` counting every transition ever written."""

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
        self.action = torch.zeros((self.capacity,), dtype=torch.int32, device=dev)
        self.next_state = torch.zeros((self.capacity, env.n_obs), **f)
        self.reward = torch.zeros((self.capacity,), **f)
        self.end = torch.zeros((self.capacity,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)    # the zero fills, before the env's own stream writes

    def __len__(self):
        return min(self.pushed, self.capacity)

    def struct(self) -> Replay:
        r = Replay()
        r.capacity = self.capacity
        for name in ("state", "action", "next_state", "reward", "end"):
            setattr(r, name, getattr(self, name).data_ptr())
        return r

    def sample(self, batch: int, seed: int = 0, draw: int = 0) -> dict:
        """ReplayMemory.batch: `batch` distinct stored transitions (replay_indices(len(self), batch,
        seed, draw)) gathered on the device: a dict of tensors state, action, next_state, reward,
        end and index."""
        import torch
        batch = int(batch)
        if not 1 <= batch <= len(self):
            raise ValueError(f"batch {batch} of {len(self)} stored transitions")
        dev = self.state.device
        out = dict(state=torch.empty((batch, self.state.shape[1]), dtype=torch.float32, device=dev),
                   action=torch.empty((batch,), dtype=torch.int32, device=dev),
                   next_state=torch.empty((batch, self.state.shape[1]), dtype=torch.float32, device=dev),
                   reward=torch.empty((batch,), dtype=torch.float32, device=dev),
                   end=torch.empty((batch,), dtype=torch.uint8, device=dev),
                   index=torch.empty((batch,), dtype=torch.int32, device=dev))
        r, b = self.struct(), _batch_struct(out)
        torch.cuda.synchronize(dev)     # torch-side writes to the rows (tests), the allocations
        rc = self.env.lib.gm_replay_sample(self.env.ctx, C.byref(r), len(self), batch, C.c_uint64(seed),
                                           C.c_uint64(draw), C.byref(b))
        if rc != 0:
            raise RuntimeError(self.env.lib.gm_last_error(self.env.ctx).decode() or f"gm_replay_sample failed ({rc})")
        torch.cuda.synchronize(dev)     # the env's stream, before torch reads the batch
        return out


class DevicePolicy:
    """A VariableNetwork DQN policy bound to a BatchedGripperEnv (discrete actions)."""

    def __init__(self, env, sizes=None, params=None, seed: int = 0):
        self.env = env
        self.lib = env.lib
        if sizes is None:
            sizes = [env.n_obs, *CANONICAL_HIDDEN, env.n_actions]
        self.sizes = [int(x) for x in sizes]
        self.params = init_params(self.sizes, seed) if params is None else np.ascontiguousarray(params, np.float32)
        sz = np.ascontiguousarray(self.sizes, dtype=np.int32)
        self._p = C.c_void_p()
        rc = self.lib.gm_policy_create(env.ctx, sz.ctypes.data_as(C.POINTER(C.c_int32)), len(sz),
                                       self.params.ctypes.data_as(C.POINTER(C.c_float)), C.byref(self._p))
        self._check(rc, "gm_policy_create")

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(self.lib.gm_last_error(self.env.ctx).decode() or f"{what} failed ({rc})")

    def act(self, eps: float = 0.0, seed: int = 0, decision: int = 0):
        """select_action for every env from its current observation, applied on the device."""
        self._check(self.lib.gm_policy_act(self._p, C.c_float(eps), C.c_uint64(seed), C.c_uint64(decision)),
                    "gm_policy_act")

    def set_params(self, params):
        """New weights after a learner update (flat, init_params' order, or a state dict)."""
        if isinstance(params, dict):
            sizes, params = params_from_state_dict(params)
            if sizes != self.sizes:
                raise ValueError("state dict does not match the network sizes")
        p = np.ascontiguousarray(as_f32(params), np.float32).ravel()
        if p.size != self.params.size:
            raise ValueError(f"{self.params.size} parameters expected, got {p.size}")
        self.params = p.copy()
        self._check(self.lib.gm_policy_set_params(self._p, self.params.ctypes.data_as(C.POINTER(C.c_float))),
                    "gm_policy_set_params")

    def push_begin(self, buf: ReplayBuffer):
        """After act(): state and action of every env into the ring rows from buf.pushed on."""
        r = buf.struct()
        self._check(self.lib.gm_policy_push_begin(self._p, C.byref(r), buf.pushed), "gm_policy_push_begin")

    def push_end(self, buf: ReplayBuffer, max_episode_steps: int | None = None):
        """After the env-step, before the auto-reset: next_state, reward and end code into the rows
        push_begin wrote; advances buf.pushed by n_envs."""
        mx = self.env.max_episode_steps if max_episode_steps is None else max_episode_steps
        r = buf.struct()
        self._check(self.lib.gm_policy_push_end(self._p, C.byref(r), buf.pushed, int(mx)), "gm_policy_push_end")
        buf.pushed += self.env.n_envs

    def rollout(self, eps, seed: int = 0, decision0: int = 0, max_episode_steps: int | None = None,
                records_dev_ptr: int | None = None, replay: ReplayBuffer | None = None):
        """gm_policy_rollout: len(eps) rounds of act(eps[k], seed, decision0 + k) -> env step ->
        auto-reset, fused into one persistent launch (bit for bit the per-step sequence).
        records_dev_ptr: device [len(eps) x n_envs] gm_episode_end records (or None).
        replay: gm_policy_rollout_replay -- the same launch also pushes every transition
        (push_begin / push_end around each env-step) and advances replay.pushed."""
        e = np.ascontiguousarray(np.atleast_1d(eps), dtype=np.float32)
        mx = self.env.max_episode_steps if max_episode_steps is None else max_episode_steps
        if replay is not None:
            r = replay.struct()
            self._check(self.lib.gm_policy_rollout_replay(
                self._p, len(e), e.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(seed), C.c_uint64(decision0),
                int(mx), C.c_void_p(records_dev_ptr or 0), C.byref(r), replay.pushed), "gm_policy_rollout_replay")
            replay.pushed += len(e) * self.env.n_envs
            return
        self._check(self.lib.gm_policy_rollout(self._p, len(e), e.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(seed),
                                               C.c_uint64(decision0), int(mx), C.c_void_p(records_dev_ptr or 0)),
                    "gm_policy_rollout")

    def evaluate(self, seed: int = 0, decision0: int = 0, max_episode_steps: int | None = None, active=None,
                 out=None) -> dict:
        """gm_policy_evaluate: one greedy episode per active env, each env retiring at its episode's
        end; the test report as device tensors (gmx.eval).  Reset the env before reuse."""
        from .eval import policy_evaluate
        return policy_evaluate(self, seed, decision0, max_episode_steps, active, out)

    def read(self):
        n, a = self.env.n_envs, self.env.n_actions
        acts = np.zeros(n, dtype=np.int32)
        q = np.zeros((n, a), dtype=np.float32)
        self._check(self.lib.gm_policy_read(self._p, acts.ctypes.data_as(C.POINTER(C.c_int32)),
                                            q.ctypes.data_as(C.POINTER(C.c_float))), "gm_policy_read")
        return acts, q

    def td_target(self, batch: dict, gamma: float, target: "DevicePolicy | None" = None, double: bool = False,
                  mask_terminal: bool = False):
        """optimise_model's expected_state_action_values for a sampled batch (ReplayBuffer.sample's
        dict; next_state, reward and end are read): (y, next_value) device tensors [batch].  self
        is the online net, target (default: self) the target net; double: the action from self,
        its value from target.  mask_terminal: no bootstrap where end == 1."""
        import torch
        tgt = self if target is None else target
        n = int(batch["reward"].shape[0])
        dev = batch["reward"].device
        y = torch.empty((n,), dtype=torch.float32, device=dev)
        v = torch.empty((n,), dtype=torch.float32, device=dev)
        b = _batch_struct(batch)
        torch.cuda.synchronize(dev)     # torch-side writes to the batch, the allocations
        self._check(self.lib.gm_policy_td_target(tgt._p, self._p if double else None, C.byref(b), n, C.c_float(gamma),
                                                 int(bool(mask_terminal)), C.c_void_p(y.data_ptr()),
                                                 C.c_void_p(v.data_ptr())), "gm_policy_td_target")
        torch.cuda.synchronize(dev)     # the env's stream, before torch reads the results
        return y, v

    def get_params(self) -> np.ndarray:
        """The device's weights in init_params' flat order (the inverse of set_params); also
        refreshes self.params, which a DeviceLearner's steps leave behind."""
        out = np.empty(self.params.size, dtype=np.float32)
        self._check(self.lib.gm_policy_get_params(self._p, out.ctypes.data_as(C.POINTER(C.c_float))),
                    "gm_policy_get_params")
        self.params = out
        return out.copy()

    def get_packed(self) -> np.ndarray:
        """The device's weights as stored (pack()'s layout, padding entries included)."""
        out = np.empty(pack(self.sizes, self.params).size, dtype=np.float32)
        self._check(self.lib.gm_policy_get_packed(self._p, out.ctypes.data_as(C.POINTER(C.c_float))),
                    "gm_policy_get_packed")
        return out

    def soft_update(self, online: "DevicePolicy", tau: float):
        """update_step's soft target update on the device: self <- tau online + (1 - tau) self.
        tau = 1 is the hard copy."""
        self._check(self.lib.gm_policy_soft_update(self._p, online._p, C.c_float(tau)), "gm_policy_soft_update")

    def close(self):
        if self._p:
            self.lib.gm_policy_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


LEARNER_MAX_BATCH = 256     # GM_LEARNER_MAX_BATCH

_OPTIMISERS = {"adam": OPT_ADAM, "adamw": OPT_ADAMW}
_LOSSES = {"smoothl1loss": LOSS_SMOOTH_L1, "huber": LOSS_SMOOTH_L1, "mseloss": LOSS_MSE}


def dqn_opt(learning_rate: float = 1e-4, adam_beta1: float = 0.9, adam_beta2: float = 0.999, optimiser: str = "adamW",
            grad_clamp_value=100, loss_criterion: str = "smoothL1Loss", eps: float = 1e-8, weight_decay=None,
            amsgrad=None) -> DqnOpt:
    """Agent_DQN.Parameters' optimiser and loss options (DQN.py:68-92) as Agent_DQN.init hands them
    to torch (:130-151), as a gm_dqn_opt: "adam" is torch.optim.Adam(lr, betas) -- weight_decay 0,
    no amsgrad; "adamW" is torch.optim.AdamW(lr, betas, amsgrad=True) -- weight_decay 0.01, torch's
    default.  weight_decay / amsgrad, when given, override that.  "Huber" (nn.HuberLoss(), delta 1)
    is "smoothL1Loss" (beta 1); grad_clamp_value None disables the clamp.  No GPU needed."""
    name = str(optimiser).lower()
    if name not in _OPTIMISERS:
        raise ValueError(f"optimiser {optimiser!r}: 'adam' or 'adamW' expected (RMSprop is not on the device)")
    if str(loss_criterion).lower() not in _LOSSES:
        raise ValueError(f"loss_criterion {loss_criterion!r}: 'smoothL1Loss', 'MSELoss' or 'Huber' expected")
    o = DqnOpt()
    o.optimiser = _OPTIMISERS[name]
    o.amsgrad = int(name == "adamw" if amsgrad is None else bool(amsgrad))
    o.loss = _LOSSES[str(loss_criterion).lower()]
    o.lr, o.beta1, o.beta2, o.eps = float(learning_rate), float(adam_beta1), float(adam_beta2), float(eps)
    o.weight_decay = float((0.01 if name == "adamw" else 0.0) if weight_decay is None else weight_decay)
    o.grad_clamp = 0.0 if grad_clamp_value is None else float(grad_clamp_value)
    return o


def dqn_opt_default() -> DqnOpt:
    """gm_dqn_opt_default: the library's own defaults (equal to dqn_opt()'s)."""
    o = DqnOpt()
    load_library().gm_dqn_opt_default(C.byref(o))
    return o


class DeviceLearner:
    """Agent_DQN.optimise_model from the loss on and the soft target update, on the device weights
    of `policy` (the online net) and `target`.  Options are Agent_DQN.Parameters' names
    (learning_rate, adam_beta1, adam_beta2, optimiser, grad_clamp_value, loss_criterion; see
    dqn_opt) plus soft_target_tau, gamma, use_double_dqn, soft_target_update and mask_terminal,
    which train() uses."""

    def __init__(self, policy: DevicePolicy, target: DevicePolicy | None = None, soft_target_tau: float = 0.05,
                 gamma: float = 0.99, use_double_dqn: bool = False, soft_target_update: bool = True,
                 mask_terminal: bool = False, **opts):
        self.policy, self.target = policy, target
        self.env, self.lib = policy.env, policy.lib
        self.tau, self.gamma = float(soft_target_tau), float(gamma)
        self.double, self.soft, self.mask_terminal = bool(use_double_dqn), bool(soft_target_update), bool(mask_terminal)
        self.opt = dqn_opt(**opts)
        self._l = C.c_void_p()
        self._check(self.lib.gm_learner_create(policy._p, C.byref(self.opt), C.byref(self._l)), "gm_learner_create")

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(self.lib.gm_last_error(self.env.ctx).decode() or f"{what} failed ({rc})")

    def grad(self, batch: dict, y):
        """loss.backward() for a sampled batch (state and action are read) and its TD targets y
        (a device tensor [batch]): leaves the raw gradient and the mean loss on the device."""
        import torch
        n = int(y.shape[0])
        b = _batch_struct(batch)
        torch.cuda.synchronize(y.device)     # torch-side writes to the batch and y
        self._check(self.lib.gm_learner_grad(self._l, C.byref(b), C.c_void_p(y.data_ptr()), n), "gm_learner_grad")
        torch.cuda.synchronize(y.device)     # the env's stream, before torch reuses the tensors

    def step(self):
        """clip_grad_value_ and optimiser.step() on the held gradient, in place on the policy."""
        self._check(self.lib.gm_learner_step(self._l), "gm_learner_step")

    def read(self):
        """(gradient in init_params' flat order, mean loss) of the last grad() / update."""
        g = np.empty(self.policy.params.size, dtype=np.float32)
        loss = C.c_float()
        self._check(self.lib.gm_learner_read(self._l, g.ctypes.data_as(C.POINTER(C.c_float)), C.byref(loss)),
                    "gm_learner_read")
        return g, float(loss.value)

    def state(self) -> dict:
        """The optimiser's state in flat order, like optimiser.state_dict()'s tensors: step,
        exp_avg, exp_avg_sq, max_exp_avg_sq."""
        f32p = C.POINTER(C.c_float)
        n = self.policy.params.size
        step = C.c_int64()
        out = {k: np.empty(n, dtype=np.float32) for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")}
        self._check(self.lib.gm_learner_get_state(self._l, C.byref(step), *(out[k].ctypes.data_as(f32p) for k in out)),
                    "gm_learner_get_state")
        return dict(step=int(step.value), **out)

    def load_state(self, state: dict):
        f32p = C.POINTER(C.c_float)
        n = self.policy.params.size
        arrs = [np.ascontiguousarray(as_f32(state[k]), np.float32).ravel()
                for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")]
        if any(a.size != n for a in arrs):
            raise ValueError(f"{n} entries per moment expected")
        step = C.c_int64(int(state["step"]))
        self._check(self.lib.gm_learner_set_state(self._l, C.byref(step), *(a.ctypes.data_as(f32p) for a in arrs)),
                    "gm_learner_set_state")

    def train(self, buf: ReplayBuffer, n_updates: int, batch_size: int = 128, seed: int = 0, draw0: int = 0):
        """n_updates of Agent_DQN.update_step's learning part, enqueued back to back: sample(draw0 + u)
        -> TD target -> gradient -> optimiser step -> soft target update.  Returns the mean loss of
        every update as a device tensor [n_updates]."""
        import torch
        dev = buf.state.device
        losses = torch.empty((int(n_updates),), dtype=torch.float32, device=dev)
        r = buf.struct()
        tau = self.tau if (self.soft and self.target is not None) else 0.0
        torch.cuda.synchronize(dev)     # torch-side writes to the memory (tests), the allocation
        self._check(self.lib.gm_learner_train(
            self._l, self.target._p if self.target is not None else None, C.byref(r), len(buf), int(batch_size),
            C.c_uint64(seed), C.c_uint64(draw0), int(n_updates), C.c_float(self.gamma), int(self.double),
            int(self.mask_terminal), C.c_float(tau), C.c_void_p(losses.data_ptr())), "gm_learner_train")
        torch.cuda.synchronize(dev)     # the env's stream, before torch reads the losses
        return losses

    def close(self):
        if self._l:
            self.lib.gm_learner_destroy(self._l)
            self._l = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
