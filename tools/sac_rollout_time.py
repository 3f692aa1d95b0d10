#!/usr/bin/env python3
"""Cost of the on-device SAC rollout ("SAC rollout"): ms per env-step at 4096 envs,
canonical continuous settings, (256, 256) nets, 10-env-step launches, for
  random      gm_rollout action_mode 1 (uniform random actions: the rollout without a policy),
  sac_fused   gm_sac_rollout with the replay memory (one persistent launch),
  sac_steps   the per-step sequence it fuses (gm_sac_act -> gm_sac_push_begin -> gm_step ->
              gm_sac_push_end -> gm_autoreset_episodes),
and, per call at batch 128, gm_sac_replay_sample + gm_sac_target ("target").  Times are HIP events:
gm_last_step_ms for the persistent launches, and events around the whole sequence on the context's
stream for all of them (the per-step sequence is several launches per env-step).  Every
measurement runs in a child process under its own time limit; the first failure stops the run.
Writes profiles/sac_rollout.json.

usage: python tools/sac_rollout_time.py [--out profiles/sac_rollout.json] [--reps 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gripper-mujoco_amd"))
sys.path.insert(0, REPO)

N, K, SEED, BATCH = 4096, 10, 1234, 128
MAX_EP = None                 # the env's own max_episode_steps
CASES = ("random", "sac_fused", "sac_steps", "target")
TARGET_CALLS = 20             # sample + target pairs per timed run


def child(case: str, reps: int) -> dict:
    import ctypes as C
    import torch
    import gmx
    import bench
    from gmx.sac import DeviceSAC, ActionReplayBuffer, _batch_struct
    env = gmx.BatchedGripperEnv(N, object_set="set6_synthetic", settings=gmx.canonical_settings(noise=True, seed=SEED),
                                seed=SEED)
    env.set_scene_spawn(bench.mjenv_spawn_params(gmx), max_tries=3)
    env.reset()
    stream = torch.cuda.Stream()                         # (a non-null stream: the context launches on it)
    env.set_stream(stream.cuda_stream)
    sac = DeviceSAC(env, hidden=(256, 256), seed=1)
    targ = DeviceSAC(env, hidden=(256, 256), seed=1)
    buf = ActionReplayBuffer(env, 4 * K * N)
    rec = torch.zeros((K, N, 3), dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    batch = dict(state=torch.empty((BATCH, env.n_obs), **f32), action=torch.empty((BATCH, env.n_actions), **f32),
                 next_state=torch.empty((BATCH, env.n_obs), **f32), reward=torch.empty((BATCH,), **f32),
                 end=torch.empty((BATCH,), dtype=torch.uint8, device="cuda"),
                 index=torch.empty((BATCH,), dtype=torch.int32, device="cuda"))
    y = torch.empty((BATCH,), **f32)
    torch.cuda.synchronize()

    def launch(i):
        if case == "random":
            env.rollout(K, action_mode=1, seed=SEED + i, max_episode_steps=MAX_EP, records_dev_ptr=rec.data_ptr())
        elif case == "sac_fused":
            sac.rollout(K, "sample", seed=SEED, decision0=i * K, max_episode_steps=MAX_EP,
                        records_dev_ptr=rec.data_ptr(), replay=buf)
        elif case == "sac_steps":
            for k in range(K):
                sac.act("sample", seed=SEED, decision=i * K + k)
                sac.push_begin(buf)
                env.action_step()
                sac.push_end(buf, max_episode_steps=MAX_EP)
                env.autoreset_device(0, None, max_episode_steps=MAX_EP, episodes_dev_ptr=rec[k].data_ptr())
        else:
            # the two calls as a training loop issues them: no host synchronisation in between
            r, b = buf.struct(), _batch_struct(batch)
            for u in range(TARGET_CALLS):
                rc = env.lib.gm_sac_replay_sample(env.ctx, C.byref(r), len(buf), BATCH, C.c_uint64(SEED + 1),
                                                  C.c_uint64(i * TARGET_CALLS + u), C.byref(b))
                assert rc == 0, rc
                rc = env.lib.gm_sac_target(targ._p, sac._p, C.byref(b), BATCH, C.c_float(0.99), C.c_float(0.2), 0,
                                           C.c_uint64(SEED + 2), C.c_uint64(i * TARGET_CALLS + u),
                                           C.c_void_p(y.data_ptr()), None, None, None, None)
                assert rc == 0, rc

    if case == "target":
        sac.rollout(K, "sample", seed=SEED, max_episode_steps=MAX_EP, replay=buf)
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
        if case in ("random", "sac_fused"):
            kern_ms.append(env.last_step_ms())
    per = float(TARGET_CALLS) if case == "target" else float(K)
    out = {"case": case, "n_envs": N, "env_steps_per_launch": K, "hidden": [256, 256],
           "ms_per_env_step" if case != "target" else "ms_per_sample_and_target": round(statistics.median(ev_ms) / per, 4),
           "event_ms_runs": [round(x / per, 4) for x in ev_ms]}
    if case == "target":
        out["batch"] = BATCH
    if kern_ms:
        out["launch_ms_per_env_step"] = round(statistics.median(kern_ms) / K, 4)
        out["launch_ms_runs"] = [round(x / K, 4) for x in kern_ms]
    sac.close()
    targ.close()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sac_rollout.json"))
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
    res["policy_price_ms_per_env_step"] = round(res["sac_fused"]["ms_per_env_step"] - res["random"]["ms_per_env_step"], 4)
    res["fused_over_per_step"] = round(res["sac_fused"]["ms_per_env_step"] / res["sac_steps"]["ms_per_env_step"], 4)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
