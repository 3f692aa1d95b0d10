#!/usr/bin/env python3
"""Cost of the on-device PPO rollout ("PPO actor-critic rollout"): ms per env-step at
4096 envs, canonical continuous settings, (64, 64) nets, 10-env-step launches, for
  random     gm_rollout action_mode 1 (uniform random actions: the rollout without a policy),
  ac_fused   gm_ac_rollout (one persistent launch),
  ac_steps   the per-step sequence it fuses (gm_ac_act -> gm_step -> gm_ac_record ->
             gm_autoreset_episodes, then gm_ac_finish),
and gm_ac_gae for K = 10.  Times are HIP events: gm_last_step_ms for the persistent launches,
and events around the whole sequence on the context's stream for all of them (the per-step
sequence is several launches per env-step).  Every measurement runs in a child process under
its own time limit; the first failure stops the run.  Writes profiles/ac_rollout.json.

usage: python tools/ac_rollout_time.py [--out profiles/ac_rollout.json] [--reps 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gripper-mujoco_amd"))
sys.path.insert(0, REPO)

N, K, SEED = 4096, 10, 1234
MAX_EP = None                 # the env's own max_episode_steps
CASES = ("random", "ac_fused", "ac_steps", "gae")


def child(case: str, reps: int) -> dict:
    import torch
    import gmx
    import bench
    from gmx.ppo import DeviceActorCritic, TrajectoryBuffer
    env = gmx.BatchedGripperEnv(N, object_set="set6_synthetic", settings=gmx.canonical_settings(noise=True, seed=SEED),
                                seed=SEED)
    env.set_scene_spawn(bench.mjenv_spawn_params(gmx), max_tries=3)
    env.reset()
    stream = torch.cuda.Stream()                         # (a non-null stream: the context launches on it)
    env.set_stream(stream.cuda_stream)
    ac = DeviceActorCritic(env, hidden=(64, 64), seed=1)
    traj = TrajectoryBuffer(env, K)
    rec = torch.zeros((K, N, 3), dtype=torch.int32, device="cuda")

    def launch(i):
        if case == "random":
            env.rollout(K, action_mode=1, seed=SEED + i, max_episode_steps=MAX_EP, records_dev_ptr=rec.data_ptr())
        elif case == "ac_fused":
            ac.rollout(traj, sample=True, noise=0.05, seed=SEED, decision0=i * K, max_episode_steps=MAX_EP,
                       records_dev_ptr=rec.data_ptr())
        elif case == "ac_steps":
            for k in range(K):
                ac.act(traj, k, sample=True, noise=0.05, seed=SEED, decision=i * K + k)
                env.action_step()
                ac.record(traj, k, max_episode_steps=MAX_EP)
                env.autoreset_device(0, None, max_episode_steps=MAX_EP, episodes_dev_ptr=rec[k].data_ptr())
            ac.finish(traj)
        else:
            import ctypes as C
            t = traj.struct()
            rc = env.lib.gm_ac_gae(env.ctx, C.byref(t), K, C.c_float(0.99), C.c_float(0.97),
                                   C.c_void_p(traj.adv.data_ptr()), C.c_void_p(traj.ret.data_ptr()))
            assert rc == 0, rc

    if case == "gae":
        ac.rollout(traj, sample=True, noise=0.05, seed=SEED, max_episode_steps=MAX_EP)
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
        if case in ("random", "ac_fused"):
            kern_ms.append(env.last_step_ms())
    per = 1.0 if case == "gae" else float(K)
    out = {"case": case, "n_envs": N, "env_steps_per_launch": K,
           "ms_per_env_step" if case != "gae" else "ms_per_call": round(statistics.median(ev_ms) / per, 4),
           "event_ms_runs": [round(x / per, 4) for x in ev_ms]}
    if kern_ms:
        out["launch_ms_per_env_step"] = round(statistics.median(kern_ms) / K, 4)
        out["launch_ms_runs"] = [round(x / K, 4) for x in kern_ms]
    ac.close()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ac_rollout.json"))
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
    res["policy_price_ms_per_env_step"] = round(res["ac_fused"]["ms_per_env_step"] - res["random"]["ms_per_env_step"], 4)
    res["fused_no_slower_than_per_step"] = res["ac_fused"]["ms_per_env_step"] <= res["ac_steps"]["ms_per_env_step"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if res["fused_no_slower_than_per_step"] else 2


if __name__ == "__main__":
    sys.exit(main())
