#!/usr/bin/env python3
"""What retiring buys ("Evaluation launch"): one evaluation launch against the only
other way to run the same episodes in a batch, a fixed-length rollout of max_episode_steps
env-steps with auto-reset.  4096 envs, the C3 workload's settings (set6_synthetic, canonical
settings, MjEnv's scene spawn), max_ep = MAX_EPISODE_STEPS, from a fresh reset, for
  eval_program / rollout_program   the grasp program (action_mode 3),
  eval_dqn / rollout_dqn           a random-weight DevicePolicy, greedy.
The rollout cases use nothing the evaluation added, so --rollout-tree can point them at another
checkout of this repository (its parent commit, built) and the cases then alternate between the
two trees, round by round, in one run.  Times are gm_last_step_ms (the launch's HIP events) and
events around the call; each measurement runs in a child process under its own time limit and
the first failure stops the run.  With the evaluation cases come the distribution of episode
lengths, the env-steps the launch ran and its tail from chunk_timeline().
Writes profiles/eval_time.json.

usage: python tools/eval_time.py [--rounds 3] [--rollout-tree DIR] [--out profiles/eval_time.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SEED = 4096, 1234
CASES = ("rollout_program", "eval_program", "rollout_dqn", "eval_dqn")


def child(case: str, tree: str) -> dict:
    sys.path.insert(0, os.path.join(tree, "gripper-mujoco_amd"))
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import gmx
    import bench
    from gmx.policy import DevicePolicy
    kind, driver = case.split("_")
    s = gmx.canonical_settings(noise=True, seed=SEED)
    if driver == "dqn":
        s.continous_actions = 0
    env = gmx.BatchedGripperEnv(N, object_set="set6_synthetic", settings=s, seed=SEED)
    env.set_scene_spawn(bench.mjenv_spawn_params(gmx), max_tries=3)
    mx = int(gmx.MAX_EPISODE_STEPS)
    stream = torch.cuda.Stream()                         # (a non-null stream: the context launches on it)
    env.set_stream(stream.cuda_stream)
    pol = DevicePolicy(env, seed=1) if driver == "dqn" else None
    rep = None

    def launch():
        nonlocal rep
        if kind == "eval":
            rep = (pol.evaluate(seed=SEED, max_episode_steps=mx) if pol is not None
                   else env.evaluate(action_mode=3, seed=SEED, max_episode_steps=mx))
        elif pol is not None:
            pol.rollout(np.zeros(mx, dtype=np.float32), seed=SEED, max_episode_steps=mx)
        else:
            env.rollout(mx, action_mode=3, seed=SEED, max_episode_steps=mx)

    out = {"case": case, "tree": "this tree" if os.path.abspath(tree) == REPO else "parent commit", "n_envs": N,
           "max_episode_steps": mx}
    for timed in (False, True):                          # one warm launch (dispatch costs), one timed
        env.reset()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        torch.cuda.synchronize()
        if timed:
            out["event_ms"] = round(e0.elapsed_time(e1), 3)
            out["launch_ms"] = round(env.last_step_ms(), 3)
    if kind == "eval":
        length = rep["length"].cpu().numpy().astype(np.int64)
        end = rep["end"].cpu().numpy()
        succ = rep["abs"].cpu().numpy()[:, list(gmx.EVENT_NAMES).index("successful_grasp")] > 0
        q = [0, 5, 25, 50, 75, 95, 100]
        out["episode_length_percentiles"] = {str(p): float(np.percentile(length, p)) for p in q}
        out["episode_length_mean"] = round(float(length.mean()), 2)
        out["env_steps_run"] = int(length.sum())
        out["env_steps_of_a_fixed_rollout"] = N * mx
        out["ended_done"], out["ended_truncated"] = int((end == 1).sum()), int((end == 2).sum())
        out["success_rate"] = round(float(succ.mean()), 4)
    ends, _, ev = env.chunk_timeline()
    fin = np.sort(ev[:, 1])
    span = float(fin[-1])
    out["timeline"] = {"span_ms": round(span, 3),
                       "envs_finished_by_ms": {str(p): round(float(np.percentile(fin, p)), 3) for p in (50, 90, 99)},
                       "tail_after_99pct_ms": round(span - float(np.percentile(fin, 99)), 3),
                       "mean_workgroup_idle_at_end_ms": round(float((span - ends).mean()), 3)}
    if pol is not None:
        pol.close()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_time.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="seconds per measurement")
    ap.add_argument("--rollout-tree", default=REPO, help="the checkout the rollout cases run in (default: this one)")
    ap.add_argument("--child", choices=CASES)
    ap.add_argument("--tree", default=REPO)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.tree)))
        return 0
    runs = {c: [] for c in CASES}
    for r in range(a.rounds):
        for case in CASES:
            tree = os.path.abspath(a.rollout_tree) if case.startswith("rollout") else REPO
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--tree", tree],
                                   capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f"{case}: no result within {a.limit} s; stopping", file=sys.stderr)
                return 1
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"{case}: failed ({p.returncode}); stopping\n{p.stderr[-2000:]}", file=sys.stderr)
                return 1
            runs[case].append(json.loads(line[-1][len("RESULT "):]))
            print(r, case, runs[case][-1]["launch_ms"], flush=True)
    res = {"rollout_tree": "this tree" if os.path.abspath(a.rollout_tree) == REPO else "parent commit", "rounds": a.rounds}
    for case in CASES:
        last = dict(runs[case][-1])
        last["launch_ms_runs"] = [x["launch_ms"] for x in runs[case]]
        last["event_ms_runs"] = [x["event_ms"] for x in runs[case]]
        last["launch_ms"] = statistics.median(last["launch_ms_runs"])
        last["event_ms"] = statistics.median(last["event_ms_runs"])
        res[case] = last
    for d in ("program", "dqn"):
        res[f"{d}_eval_over_rollout"] = round(res[f"eval_{d}"]["launch_ms"] / res[f"rollout_{d}"]["launch_ms"], 4)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
