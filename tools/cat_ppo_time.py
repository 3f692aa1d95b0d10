#!/usr/bin/env python3
"""Cost of the on-device categorical PPO ("Categorical PPO"), 4096 envs, canonical
settings with discrete actions (8 classes).

Rollout, ms per env-step over 10-env-step launches, (20, 20) and (64, 64) nets:
  fused      gm_ac_rollout on a categorical handle (one persistent launch),
  steps      the per-step sequence it fuses (gm_ac_act -> gm_step -> gm_ac_record ->
             gm_autoreset_episodes, then gm_ac_finish).
Update, ms per optimise_model at 4096 x 10 = 40,960 rows, (64, 64) nets, train_pi_iters =
train_vf_iters = 80, the KL stop disabled:
  update     gm_ppo_learner_update,
  calls      the same device sequence made call by call through the C ABI,
  torch      the sequence it replaces on the same GPU: TrajectoryBuffer.get() -> the reference's two
             loops in torch (Categorical(logits).log_prob of act.squeeze(-1).long(), kl.item() every
             iteration) -> set_params.
update and calls alternate in one process on one learner (update, calls, update, ...), so that both
see the same allocations and clocks.
Times are HIP events on the context's stream, median of `--reps` runs after warm-up.  Every
measurement runs in a child process under its own time limit; the first failure stops the run.
Gates: fused <= steps for both nets; update <= calls + the calls measurement's own spread
(max - min of its runs).  Writes profiles/cat_ppo.json; exits 2 when a gate fails.

usage: python tools/cat_ppo_time.py [--out profiles/cat_ppo.json] [--reps 5]"""
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

N, K, ITERS, SEED = 4096, 10, 80, 1234
NETS = {"20": (20, 20), "64": (64, 64)}
CASES = ("fused_20", "steps_20", "fused_64", "steps_64", "update_calls", "torch")
OPTS = dict(train_pi_iters=ITERS, train_vf_iters=ITERS, target_kl=1e30)


def make(hidden):
    import torch
    import gmx
    import bench
    from gmx.ppo import DeviceCategoricalActorCritic, TrajectoryBuffer
    s = gmx.canonical_settings(noise=True, seed=SEED)
    s.continous_actions = 0
    env = gmx.BatchedGripperEnv(N, object_set="set6_synthetic", settings=s, seed=SEED)
    env.set_scene_spawn(bench.mjenv_spawn_params(gmx), max_tries=3)
    env.reset()
    stream = torch.cuda.Stream()                         # (a non-null stream: the context launches on it)
    env.set_stream(stream.cuda_stream)
    ac = DeviceCategoricalActorCritic(env, hidden=hidden, seed=1)
    return env, stream, ac, TrajectoryBuffer(env, K, act_dim=1)


def rollout_case(case: str, reps: int) -> dict:
    import torch
    kind, net = case.split("_")
    env, stream, ac, traj = make(NETS[net])
    rec = torch.zeros((K, N, 3), dtype=torch.int32, device="cuda")

    def launch(i):
        if kind == "fused":
            ac.rollout(traj, sample=True, seed=SEED, decision0=i * K, records_dev_ptr=rec.data_ptr())
        else:
            for k in range(K):
                ac.act(traj, k, sample=True, seed=SEED, decision=i * K + k)
                env.action_step()
                ac.record(traj, k)
                env.autoreset_device(0, None, max_episode_steps=None, episodes_dev_ptr=rec[k].data_ptr())
            ac.finish(traj)
    for i in range(3):                                   # warm-up (dispatch costs, steady mix of episodes)
        launch(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(3, 3 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch(i)
        e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / K)
    counts = torch.bincount(traj.act.reshape(-1).long(), minlength=env.n_actions).cpu().tolist()
    ac.close()
    env.close()
    return {"case": case, "hidden": list(NETS[net]), "n_envs": N, "env_steps_per_launch": K,
            "ms_per_env_step": round(statistics.median(ms), 4), "ms_per_env_step_runs": [round(x, 4) for x in ms],
            "last_launch_action_counts": counts}


def update_case(case: str, reps: int) -> dict:
    import torch
    from gmx.ppo import DevicePPOLearner
    from gmx._lib import PpoBatch
    env, stream, ac, traj = make(NETS["64"])
    lib = env.lib
    ac.rollout(traj, sample=True, seed=SEED, decision0=0, max_episode_steps=5)
    torch.cuda.synchronize()
    start = ac.get_params()
    learner = DevicePPOLearner(ac, **OPTS)
    t = traj.struct()
    n = K * N

    def timed(fns, before):
        """Milliseconds of each of fns per round, the functions taking turns; the first round is the warm-up."""
        ms = [[] for _ in fns]
        for i in range(reps + 1):
            for j, fn in enumerate(fns):
                before()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                torch.cuda.synchronize()
                ms[j].append(e0.elapsed_time(e1))
        return [m[1:] for m in ms]

    def restart():
        ac.set_params(start)

    out = {"case": case, "rows": n, "iters": ITERS, "hidden": list(NETS["64"])}
    if case == "update_calls":
        b = PpoBatch()
        b.n = n
        for k in ("obs", "act", "logp", "adv", "ret"):
            setattr(b, k, getattr(traj, k).data_ptr())

        def run():
            assert lib.gm_ac_gae(env.ctx, C.byref(t), K, C.c_float(0.99), C.c_float(0.97), C.c_void_p(traj.adv.data_ptr()),
                                 C.c_void_p(traj.ret.data_ptr())) == 0
            assert lib.gm_ac_adv_normalise(env.ctx, C.c_void_p(traj.adv.data_ptr()), n) == 0
            for _ in range(ITERS):
                assert lib.gm_ppo_learner_grad_pi(learner._l, C.byref(b)) == 0
                assert lib.gm_ppo_learner_step_pi(learner._l) == 0
            for _ in range(ITERS):
                assert lib.gm_ppo_learner_grad_vf(learner._l, C.byref(b)) == 0
                assert lib.gm_ppo_learner_step_vf(learner._l) == 0
        for name, ms in zip(("update", "calls"), timed([lambda: learner.update(traj), run], restart)):
            out[name] = {"ms_per_update": round(statistics.median(ms), 3), "ms_per_update_runs": [round(x, 3) for x in ms]}
    else:
        from torch import nn

        def mlp(sizes):
            layers = []
            for i in range(len(sizes) - 1):
                layers += [nn.Linear(sizes[i], sizes[i + 1]), nn.Tanh() if i < len(sizes) - 2 else nn.Identity()]
            return nn.Sequential(*layers).cuda()
        logits_net, v_net = mlp(ac.actor_sizes), mlp(ac.critic_sizes)
        prms = list(logits_net.parameters()) + list(v_net.parameters())
        pi_opt = torch.optim.Adam(logits_net.parameters(), lr=3e-4)
        vf_opt = torch.optim.Adam(v_net.parameters(), lr=1e-3)

        def load():
            flat, pos = torch.from_numpy(start).cuda(), 0
            with torch.no_grad():
                for p in prms:
                    p.copy_(flat[pos:pos + p.numel()].reshape(p.shape))
                    pos += p.numel()

        def run():
            with torch.cuda.stream(stream):
                data = traj.get(0.99, 0.97)
                act = data["act"].squeeze(-1).long()
                for _ in range(ITERS):
                    pi_opt.zero_grad()
                    logp = torch.distributions.Categorical(logits=logits_net(data["obs"])).log_prob(act)
                    ratio = torch.exp(logp - data["logp"])
                    loss = -torch.min(ratio * data["adv"], torch.clamp(ratio, 0.8, 1.2) * data["adv"]).mean()
                    kl = (data["logp"] - logp).mean().item()       # optimise_model reads kl every iteration
                    if kl > 1e30:
                        break
                    loss.backward()
                    pi_opt.step()
                for _ in range(ITERS):
                    vf_opt.zero_grad()
                    loss = ((v_net(data["obs"])[:, 0] - data["ret"]) ** 2).mean()
                    loss.backward()
                    vf_opt.step()
                ac.set_params(torch.cat([p.detach().reshape(-1) for p in prms]).cpu().numpy())
        ms, = timed([run], load)
        out.update(ms_per_update=round(statistics.median(ms), 3), ms_per_update_runs=[round(x, 3) for x in ms])
    learner.close()
    ac.close()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cat_ppo.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=150, help="seconds per measurement")
    ap.add_argument("--child", choices=CASES)
    a = ap.parse_args()
    if a.child:
        fn = update_case if a.child in ("update_calls", "torch") else rollout_case
        print("RESULT " + json.dumps(fn(a.child, a.reps)))
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
        print(case, res[case], flush=True)
    res["update"], res["calls"] = res["update_calls"].pop("update"), res["update_calls"].pop("calls")
    gates = {f"fused_no_slower_than_per_step_{n}": res[f"fused_{n}"]["ms_per_env_step"] <= res[f"steps_{n}"]["ms_per_env_step"]
             for n in NETS}
    runs = res["calls"]["ms_per_update_runs"]
    res["calls_run_to_run_spread_ms"] = round(max(runs) - min(runs), 3)
    gates["update_no_slower_than_calls_plus_spread"] = \
        res["update"]["ms_per_update"] <= res["calls"]["ms_per_update"] + res["calls_run_to_run_spread_ms"]
    res["update_vs_torch_speedup"] = round(res["torch"]["ms_per_update"] / res["update"]["ms_per_update"], 2)
    res["gates"] = gates
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if all(gates.values()) else 2


if __name__ == "__main__":
    sys.exit(main())
