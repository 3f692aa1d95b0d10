"""Batched evaluation: MujocoTrainer.test() (rl/Trainer.py:950-1015) for n_envs envs at once.

The reference's test runs test_objects x test_trials_per_object episodes, each on a chosen object
and exactly one episode long with the agent in its test mode, and keeps MjEnv._monitor_test's
test report of each (rl/env/MjEnv.py:1279-1326): the object, the cumulative reward and the event
track.  Here one evaluation launch (include/gripper_mi355x.h gm_evaluate and the like) runs one
episode in every active env and each env leaves the work queue when its episode ends, so the
launch ends with the last episode; a wave of such launches covers the test set:

  - `evaluate` methods on BatchedGripperEnv (the scripted drivers; action_mode 3, the grasp
    program, is Trainer.test(heuristic=True)), DevicePolicy (greedy), DeviceActorCritic /
    DeviceCategoricalActorCritic (sample=True is the reference's PPO test mode, which still
    samples; sample=False the mean / argmax) and DeviceSAC (mode "mean") return the report as
    torch tensors on the env's device;
  - test_plan assigns the trials to waves and envs in _monitor_test's order;
  - Evaluator resets every wave onto its chosen objects, launches, reads back, and returns one
    numpy record per trial; test_performance reduces them to the figures of
    Trainer.get_test_performance (success rate, mean reward, mean steps), overall, per object and
    per object type.

The reports are a deterministic function of the env states and the arguments at the call.  They
do depend on n_envs and env_offset: each env's RNG stream is keyed by its global id and persists
across episodes, so the same trial run in another env slot sees other sensor noise.  After an
evaluate() the env states are unspecified (the fused launch parks each env at its terminal state,
the per-step sequence leaves it in a later episode): reset before reuse.  Evaluator.run does.

The text report of create_test_report, saving, plotting and the curriculum are not here, nor are
EventTrack.calculate_percentage's percentages: apply 100 * abs / abs[step_num] to the abs rows.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import BINARY_EVENTS, LINEAR_EVENTS, RolloutParams
from .settings import MAX_EPISODE_STEPS

N_EVENTS = len(BINARY_EVENTS) + len(LINEAR_EVENTS)
EVENT_NAMES = tuple(BINARY_EVENTS) + tuple(LINEAR_EVENTS)
REPORT_FIELDS = ("ret", "length", "end", "rows", "abs", "last")


class EvalOut(C.Structure):
    """gm_eval_out (include/gripper_mi355x.h)."""
    _fields_ = [(name, C.c_void_p) for name in REPORT_FIELDS]


def new_report(env) -> dict:
    """Zeroed report tensors on the env's device in gm_eval_out's layout: ret [n] f32, length [n]
    i32, end [n] u8 and rows / abs / last [n, W] (i32, i32, f32), W the binary then the linear
    events (gm_get_event_rows' column order, EVENT_NAMES)."""
    import torch
    n, dev = env.n_envs, f"cuda:{env.device}"
    return dict(ret=torch.zeros((n,), dtype=torch.float32, device=dev),
                length=torch.zeros((n,), dtype=torch.int32, device=dev),
                end=torch.zeros((n,), dtype=torch.uint8, device=dev),
                rows=torch.zeros((n, N_EVENTS), dtype=torch.int32, device=dev),
                abs=torch.zeros((n, N_EVENTS), dtype=torch.int32, device=dev),
                last=torch.zeros((n, N_EVENTS), dtype=torch.float32, device=dev))


def report_struct(report: dict) -> EvalOut:
    o = EvalOut()
    for name in REPORT_FIELDS:
        t = report.get(name)
        setattr(o, name, t.data_ptr() if t is not None else None)
    return o


def active_tensor(env, active):
    """active (None: every env; a bool / uint8 tensor or array of n_envs) as a uint8 tensor on the
    env's device, or None."""
    import torch
    if active is None:
        return None
    t = torch.as_tensor(np.asarray(active.cpu() if hasattr(active, "cpu") else active).astype(np.uint8))
    if tuple(t.shape) != (env.n_envs,):
        raise ValueError(f"active: {env.n_envs} flags expected, got shape {tuple(t.shape)}")
    return t.to(f"cuda:{env.device}").contiguous()


def _launch(env, what, call, active, out):
    """One evaluation call: the report tensors (out, or new ones), the active bytes, the two
    synchronisations between torch's stream and the env's own."""
    import torch
    dev = f"cuda:{env.device}"
    rep = new_report(env) if out is None else out
    act = active_tensor(env, active)
    o = report_struct(rep)
    torch.cuda.synchronize(dev)     # the fills and copies above, before the env's own stream writes
    rc = call(C.c_void_p(act.data_ptr() if act is not None else 0), C.byref(o))
    if rc != 0:
        raise RuntimeError(env.lib.gm_last_error(env.ctx).decode() or f"{what} failed ({rc})")
    torch.cuda.synchronize(dev)     # the env's stream, before torch reads the report
    return rep


def _max_ep(env, max_episode_steps):
    return int(env.max_episode_steps if max_episode_steps is None else max_episode_steps)


def env_evaluate(env, action_mode: int = 3, seed: int = 1234, jitter: float = 0.2, max_episode_steps=None,
                 active=None, out=None) -> dict:
    """BatchedGripperEnv.evaluate (gm_evaluate): one episode per active env under a scripted driver
    (0 scripted mix, 1 random, 3 the grasp program, 4 the program / scripted mix)."""
    p = RolloutParams()
    p.action_mode, p.max_episode_steps, p.seed, p.jitter = (int(action_mode), _max_ep(env, max_episode_steps),
                                                            int(seed), float(jitter))
    return _launch(env, "gm_evaluate", lambda a, o: env.lib.gm_evaluate(env.ctx, C.byref(p), a, o), active, out)


def env_eval_record(env, active, out, max_episode_steps=None):
    """BatchedGripperEnv.eval_record (gm_eval_record), the per-step half: after an env-step, every
    env whose byte in `active` (a uint8 device tensor, updated in place) is set and whose episode
    has ended writes its report into `out` and clears its byte."""
    import torch
    o = report_struct(out)
    if active.dtype != torch.uint8 or not active.is_cuda or tuple(active.shape) != (env.n_envs,):
        raise ValueError("active: a uint8 device tensor of n_envs flags expected")
    torch.cuda.synchronize(active.device)
    rc = env.lib.gm_eval_record(env.ctx, _max_ep(env, max_episode_steps), C.c_void_p(active.data_ptr()), C.byref(o))
    if rc != 0:
        raise RuntimeError(env.lib.gm_last_error(env.ctx).decode() or f"gm_eval_record failed ({rc})")


def policy_evaluate(policy, seed: int = 0, decision0: int = 0, max_episode_steps=None, active=None, out=None) -> dict:
    """DevicePolicy.evaluate (gm_policy_evaluate): one greedy (eps = 0) episode per active env."""
    env = policy.env
    mx = _max_ep(env, max_episode_steps)
    return _launch(env, "gm_policy_evaluate",
                   lambda a, o: policy.lib.gm_policy_evaluate(policy._p, C.c_uint64(seed), C.c_uint64(decision0), mx, a, o),
                   active, out)


def ac_evaluate(ac, sample: bool = True, seed: int = 0, decision0: int = 0, max_episode_steps=None, active=None,
                out=None) -> dict:
    """DeviceActorCritic.evaluate (gm_ac_evaluate), both actor kinds: sample=True is the reference's
    PPO test mode (it still samples, without exploration noise), sample=False the mean / argmax.
    No trajectory buffer is involved."""
    env = ac.env
    mx = _max_ep(env, max_episode_steps)
    return _launch(env, "gm_ac_evaluate",
                   lambda a, o: ac.lib.gm_ac_evaluate(ac._p, int(bool(sample)), C.c_uint64(seed), C.c_uint64(decision0),
                                                      mx, a, o), active, out)


def sac_evaluate(sac, mode="mean", seed: int = 0, decision0: int = 0, max_episode_steps=None, active=None,
                 out=None) -> dict:
    """DeviceSAC.evaluate (gm_sac_evaluate): one episode per active env, by default with the
    deterministic mean action.  No replay memory is involved."""
    from .sac import _mode
    env = sac.env
    mx = _max_ep(env, max_episode_steps)
    return _launch(env, "gm_sac_evaluate",
                   lambda a, o: sac.lib.gm_sac_evaluate(sac._p, _mode(mode), C.c_uint64(seed), C.c_uint64(decision0), mx,
                                                        a, o), active, out)


# ------------------------------------------------------------------ the test set
def test_plan(n_test_objects: int, trials_per_object: int, n_envs: int) -> list:
    """The waves of a test of n_test_objects x trials_per_object episodes on n_envs envs.  Pure
    host code.  Trial t is (obj_idx = t // trials_per_object, obj_trial = t % trials_per_object),
    MjEnv._monitor_test's order; wave w runs trials [w n_envs, (w + 1) n_envs), env e of it trial
    w n_envs + e; the last wave's surplus envs are inactive.  Returns one dict per wave of int32
    arrays [n_envs] trial, obj_idx, obj_trial (-1 for an inactive env) and the bool array active."""
    n_obj, per, n = int(n_test_objects), int(trials_per_object), int(n_envs)
    if n_obj < 1 or per < 1 or n < 1:
        raise ValueError("n_test_objects, trials_per_object and n_envs must be positive")
    total = n_obj * per
    waves = []
    for w in range((total + n - 1) // n):
        t = w * n + np.arange(n, dtype=np.int32)
        active = t < total
        waves.append(dict(trial=np.where(active, t, -1).astype(np.int32),
                          obj_idx=np.where(active, t // per, -1).astype(np.int32),
                          obj_trial=np.where(active, t % per, -1).astype(np.int32),
                          active=active))
    return waves



def report_dtype():
    """One trial of Evaluator.run's result."""
    return np.dtype([("obj_idx", "i4"), ("obj_trial", "i4"), ("object_type", "i4"), ("reward", "f4"), ("length", "i4"),
                     ("end", "u1"), ("rows", "i4", N_EVENTS), ("abs", "i4", N_EVENTS), ("last", "f4", N_EVENTS)])


class Evaluator:
    """MujocoTrainer.test() on a BatchedGripperEnv.  test_objects: indices into the env's object
    set (None: every object), MjEnv's test_objects; trials_per_object: its test_trials_per_object."""

    def __init__(self, env, test_objects=None, trials_per_object: int = 3, max_episode_steps: int = MAX_EPISODE_STEPS):
        self.env = env
        n_set = len(env.objects)
        self.test_objects = np.arange(n_set, dtype=np.int32) if test_objects is None \
            else np.asarray(test_objects, dtype=np.int32).reshape(-1)
        if self.test_objects.size < 1 or self.test_objects.min() < 0 or self.test_objects.max() >= n_set:
            raise ValueError(f"test_objects must index the env's {n_set} objects")
        self.trials_per_object = int(trials_per_object)
        self.max_episode_steps = int(max_episode_steps)
        self.plan = test_plan(len(self.test_objects), self.trials_per_object, env.n_envs)

    def wave_objects(self, wave: dict) -> np.ndarray:
        """The object-set index every env of a wave is reset onto (an inactive env: the first test object)."""
        return self.test_objects[np.where(wave["active"], wave["obj_idx"], 0)]

    def run(self, agent=None, **mode) -> np.ndarray:
        """One episode per trial with `agent` in the given mode: anything with an evaluate() of this
        module (a DevicePolicy, DeviceActorCritic, DeviceCategoricalActorCritic or DeviceSAC bound
        to the env, or the env itself / None for its scripted drivers, e.g. action_mode=3).  Per
        wave: env.reset onto the wave's chosen objects (the pose is MjEnv._spawn_object's draw, and
        set_scene_spawn's search applies if the caller enabled it), one evaluation launch, one
        read-back.  Returns a numpy structured array (report_dtype) in trial order and leaves the
        env reset, so that a training rollout can follow."""
        env = self.env
        agent = env if agent is None else agent
        if agent is not env and getattr(agent, "env", None) is not env:
            raise ValueError("the agent is bound to another env")
        data = np.zeros(len(self.test_objects) * self.trials_per_object, dtype=report_dtype())
        for wave in self.plan:
            idx = self.wave_objects(wave)
            env.reset(spawn=env.make_spawn(idx=idx))
            rep = agent.evaluate(max_episode_steps=self.max_episode_steps, active=wave["active"], **mode)
            host = {k: v.cpu().numpy() for k, v in rep.items()}
            a = wave["active"]
            rows = data[wave["trial"][a]]
            rows["obj_idx"], rows["obj_trial"] = wave["obj_idx"][a], wave["obj_trial"][a]
            rows["object_type"] = [env.objects[int(i)].type for i in idx[a]]
            rows["reward"], rows["length"], rows["end"] = host["ret"][a], host["length"][a], host["end"][a]
            rows["rows"], rows["abs"], rows["last"] = host["rows"][a], host["abs"][a], host["last"][a]
            data[wave["trial"][a]] = rows
        env.reset()
        return data


def _performance(d) -> dict:
    succ = d["abs"][:, EVENT_NAMES.index("successful_grasp")] > 0
    return dict(trials=int(d.size), success_rate=float(succ.mean()), mean_reward=float(d["reward"].astype(np.float64).mean()),
                mean_steps=float(d["length"].astype(np.float64).mean()))


def test_performance(data) -> dict:
    """Trainer.get_test_performance's figures from Evaluator.run's records: trials, success_rate
    (the share of trials with abs[successful_grasp] > 0, MjEnv's metric), mean_reward and
    mean_steps; the same under per_object (keyed by obj_idx) and per_object_type (keyed by the
    geom type), both in order of first appearance."""
    d = np.asarray(data)
    if d.size < 1:
        raise ValueError("no trials")
    out = _performance(d)
    for key, field in (("per_object", "obj_idx"), ("per_object_type", "object_type")):
        seen = list(dict.fromkeys(int(v) for v in d[field]))
        out[key] = {v: _performance(d[d[field] == v]) for v in seen}
    return out

