#!/usr/bin/env python3
"""Cost of the on-device DQN replay memory ("DQN replay memory and TD target"): ms per
env-step at 4096 envs, canonical discrete settings, the canonical network, 10-env-step launches, for
  dqn_fused      gm_policy_rollout (one persistent launch, nothing recorded),
  replay_fused   gm_policy_rollout_replay (the same launch, recording every transition),
  replay_steps   the per-step sequence it fuses (gm_policy_act -> gm_policy_push_begin -> gm_step
                 -> gm_policy_push_end -> gm_autoreset_episodes),
and, per call at batch 128, gm_replay_sample and gm_policy_td_target (plain and double).  Times are
HIP events around the whole sequence on the context's stream, and gm_last_step_ms for the
persistent launches.  Every measurement runs in a child process under its own time limit; the
first failure stops the run.  Writes profiles/dqn_replay.json.

usage: python tools/dqn_replay_time.py [--out profiles/dqn_replay.json] [--reps 5]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gripper-mujoco_amd"))
sys.path.insert(0, REPO)

N, K, SEED, BATCH = 4096, 10, 1234, 128
CAPACITY = 4 * K * N
MAX_EP = None                 # the env's own max_episode_steps
CASES = ("dqn_fused", "replay_fused", "replay_steps", "sample", "td_target", "td_target_double")


def child(case: str, reps: int) -> dict:
    import numpy as np
    import torch
    import gmx
    import bench
    from gmx.policy import DevicePolicy, _batch_struct
    s = gmx.canonical_settings(noise=True, seed=SEED)
    s.continous_actions = 0
    env = gmx.BatchedGripperEnv(N, object_set="set6_synthetic", settings=s, seed=SEED)
    env.set_scene_spawn(bench.mjenv_spawn_params(gmx), max_tries=3)
    env.reset()
    stream = torch.cuda.Stream()                         # (a non-null stream: the context launches on it)
    env.set_stream(stream.cuda_stream)
    pol, tgt = DevicePolicy(env, seed=1), DevicePolicy(env, seed=2)
    buf = gmx.ReplayBuffer(env, CAPACITY)
    rec = torch.zeros((K, N, 3), dtype=torch.int32, device="cuda")
    eps = np.full(K, 0.2, dtype=np.float32)
    per_call = case in ("sample", "td_target", "td_target_double")
    batch = out = y = v = None
    if per_call:
        pol.rollout(eps, seed=SEED, max_episode_steps=MAX_EP, replay=buf)
        batch = buf.sample(BATCH, seed=SEED, draw=0)
        out, r = _batch_struct(batch), buf.struct()
        y, v = (torch.empty(BATCH, dtype=torch.float32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()

    def launch(i):
        if case == "dqn_fused":
            pol.rollout(eps, seed=SEED, decision0=i * K, max_episode_steps=MAX_EP, records_dev_ptr=rec.data_ptr())
        elif case == "replay_fused":
            pol.rollout(eps, seed=SEED, decision0=i * K, max_episode_steps=MAX_EP, records_dev_ptr=rec.data_ptr(),
                        replay=buf)
        elif case == "replay_steps":
            for k in range(K):
                pol.act(float(eps[k]), seed=SEED, decision=i * K + k)
                pol.push_begin(buf)
                env.action_step()
                pol.push_end(buf, max_episode_steps=MAX_EP)
                env.autoreset_device(0, None, max_episode_steps=MAX_EP, episodes_dev_ptr=rec[k].data_ptr())
        elif case == "sample":      # (the C calls: the Python wrappers synchronise around theirs)
            rc = env.lib.gm_replay_sample(env.ctx, C.byref(r), len(buf), BATCH, C.c_uint64(SEED), C.c_uint64(i), C.byref(out))
            assert rc == 0, rc
        else:
            rc = env.lib.gm_policy_td_target(tgt._p, pol._p if case == "td_target_double" else None, C.byref(out), BATCH,
                                             C.c_float(0.99), 0, C.c_void_p(y.data_ptr()), C.c_void_p(v.data_ptr()))
            assert rc == 0, rc

    for i in range(3):                                   # warm-up (dispatch costs, steady mix of episodes)
        launch(i)
    torch.cuda.synchronize()
    ev_ms, kern_ms = [], []
    for i in range(3, 3 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch(i)
        e1.record(stream)
        torch.cuda.synchronize()
        ev_ms.append(e0.elapsed_time(e1))
        if case in ("dqn_fused", "replay_fused"):
            kern_ms.append(env.last_step_ms())
    per = 1.0 if per_call else float(K)
    res = {"case": case, "n_envs": N, "env_steps_per_launch": K,
           "ms_per_call" if per_call else "ms_per_env_step": round(statistics.median(ev_ms) / per, 4),
           "event_ms_runs": [round(x / per, 4) for x in ev_ms]}
    if per_call:
        res["batch"] = BATCH
    if kern_ms:
        res["launch_ms_per_env_step"] = round(statistics.median(kern_ms) / K, 4)
        res["launch_ms_runs"] = [round(x / K, 4) for x in kern_ms]
    pol.close()
    tgt.close()
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dqn_replay.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per measurement")
    ap.add_argument("--child", choices=CASES)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.reps)))
        return 0
    res = {}
    for case in CASES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{case}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{case}: failed ({p.returncode}); stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1
        res[case] = json.loads(line[-1][len("RESULT "):])
        print(case, res[case])
    base = res["dqn_fused"]["event_ms_runs"]
    res["recording_price_ms_per_env_step"] = round(res["replay_fused"]["ms_per_env_step"] - res["dqn_fused"]["ms_per_env_step"], 4)
    res["dqn_fused_run_to_run_spread_ms"] = round(max(base) - min(base), 4)
    res["fused_no_slower_than_per_step"] = res["replay_fused"]["ms_per_env_step"] <= res["replay_steps"]["ms_per_env_step"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if res["fused_no_slower_than_per_step"] else 2


if __name__ == "__main__":
    sys.exit(main())
