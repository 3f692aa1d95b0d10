#!/usr/bin/env python3
"""Cost of one PPO update on the device ("PPO learner"): milliseconds per optimise_model,
default (64, 64) nets, 4096 envs x 10 env-steps = 40,960 rows collected by gm_ac_rollout,
train_pi_iters = train_vf_iters = 80 with the KL stop disabled, for
  update       gm_ppo_learner_update: GAE -> advantage normalisation -> 80 x (policy gradient, reduce,
               Adam step) -> 80 x (value gradient, reduce, Adam step), one host read at the end,
  calls        the same device sequence made call by call through the C ABI,
  torch        the sequence it replaces on the same GPU: TrajectoryBuffer.get() -> the reference's two
               loops in torch (compute_loss_pi / backward / Adam step with kl.item() every iteration,
               compute_loss_v / backward / Adam step) -> DeviceActorCritic.set_params,
and two more measurements:
  groups       the policy gradient (gradient + reduce kernels) alone for n_groups in 128, 256, 512,
               1024: the sweep the library's default n_groups comes from,
  split        each launch group of an update alone: GAE + normalisation, policy gradient + reduce,
               policy step, value gradient + reduce, value step (microseconds each).
Times are HIP events on the context's stream (which torch shares here), median of `--reps` runs
after a warm-up run.  Every measurement runs in a child process under its own time limit; the first
failure stops the run.  Writes profiles/ppo_learn.json.

usage: python tools/ppo_learn_time.py [--out profiles/ppo_learn.json] [--reps 5]"""
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

N_ENVS, K, ITERS, SEED = 4096, 10, 80, 1234
GROUPS = (128, 256, 512, 1024)
CASES = ("update", "calls", "torch", "groups", "split")
OPTS = dict(train_pi_iters=ITERS, train_vf_iters=ITERS, target_kl=1e30)


def child(case: str, reps: int) -> dict:
    import torch
    import gmx
    from gmx.ppo import DeviceActorCritic, DevicePPOLearner, TrajectoryBuffer
    from gmx._lib import PpoBatch
    env = gmx.BatchedGripperEnv(N_ENVS, object_set="set6_synthetic", settings=gmx.canonical_settings(noise=True, seed=SEED),
                                seed=SEED)
    env.reset()
    stream = torch.cuda.Stream()                         # (a non-null stream: the context launches on it)
    env.set_stream(stream.cuda_stream)
    lib = env.lib
    ac = DeviceActorCritic(env, seed=1)
    traj = TrajectoryBuffer(env, K)
    ac.rollout(traj, sample=True, noise=0.0, seed=SEED, decision0=0, max_episode_steps=5)
    torch.cuda.synchronize()
    start = ac.get_params()
    learner = DevicePPOLearner(ac, **OPTS)
    t = traj.struct()
    n = K * N_ENVS

    def batch():
        b = PpoBatch()
        b.n = n
        for k in ("obs", "act", "logp", "adv", "ret"):
            setattr(b, k, getattr(traj, k).data_ptr())
        return b

    def gae_and_normalise():
        assert lib.gm_ac_gae(env.ctx, C.byref(t), K, C.c_float(0.99), C.c_float(0.97), C.c_void_p(traj.adv.data_ptr()),
                             C.c_void_p(traj.ret.data_ptr())) == 0
        assert lib.gm_ac_adv_normalise(env.ctx, C.c_void_p(traj.adv.data_ptr()), n) == 0

    def timed(fn, before=None):
        """Milliseconds of fn() per run, after one warm-up run; before() runs ahead of each, untimed."""
        ms = []
        for i in range(reps + 1):
            if before:
                before()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms[1:]

    def restart():
        ac.set_params(start)

    res = {"case": case, "rows": n, "iters": ITERS}
    if case == "update":
        ms = timed(lambda: learner.update(traj), restart)
        res.update(ms_per_update=round(statistics.median(ms), 3), ms_per_update_runs=[round(x, 3) for x in ms],
                   n_groups="default")
    elif case == "calls":
        b = batch()

        def run():
            gae_and_normalise()
            for _ in range(ITERS):
                assert lib.gm_ppo_learner_grad_pi(learner._l, C.byref(b)) == 0
                assert lib.gm_ppo_learner_step_pi(learner._l) == 0
            for _ in range(ITERS):
                assert lib.gm_ppo_learner_grad_vf(learner._l, C.byref(b)) == 0
                assert lib.gm_ppo_learner_step_vf(learner._l) == 0
        ms = timed(run, restart)
        res.update(ms_per_update=round(statistics.median(ms), 3), ms_per_update_runs=[round(x, 3) for x in ms])
    elif case == "torch":
        from torch import nn

        def mlp(sizes):
            layers = []
            for i in range(len(sizes) - 1):
                layers += [nn.Linear(sizes[i], sizes[i + 1]), nn.Tanh() if i < len(sizes) - 2 else nn.Identity()]
            return nn.Sequential(*layers).cuda()
        mu_net, v_net = mlp(ac.actor_sizes), mlp(ac.critic_sizes)
        log_std = nn.Parameter(torch.zeros(env.n_actions, device="cuda"))
        prms = list(mu_net.parameters()) + list(v_net.parameters()) + [log_std]
        pi_opt = torch.optim.Adam(list(mu_net.parameters()) + [log_std], lr=3e-4)
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
                for _ in range(ITERS):
                    pi_opt.zero_grad()
                    pi = torch.distributions.Normal(mu_net(data["obs"]), torch.exp(log_std))
                    logp = pi.log_prob(data["act"]).sum(-1)
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
                # the hand-back: the new weights to the device through the host
                ac.set_params(torch.cat([p.detach().reshape(-1) for p in prms]).cpu().numpy())
        ms = timed(run, load)
        res.update(ms_per_update=round(statistics.median(ms), 3), ms_per_update_runs=[round(x, 3) for x in ms])
    elif case == "groups":
        gae_and_normalise()
        b = batch()
        sweep = {}
        for g in GROUPS:
            l = DevicePPOLearner(ac, n_groups=g, **OPTS)

            def run():
                for _ in range(20):
                    assert lib.gm_ppo_learner_grad_pi(l._l, C.byref(b)) == 0
            ms = timed(run)
            sweep[str(g)] = dict(us_per_gradient=round(1000.0 * statistics.median(ms) / 20, 2),
                                 us_per_gradient_runs=[round(1000.0 * x / 20, 2) for x in ms])
            l.close()
        res.update(policy_gradient_and_reduce=sweep, fastest=min(sweep, key=lambda g: sweep[g]["us_per_gradient"]))
    else:
        gae_and_normalise()
        b = batch()
        parts = {"gae_and_normalise": (gae_and_normalise, 1),
                 "policy_gradient_and_reduce": (lambda: lib.gm_ppo_learner_grad_pi(learner._l, C.byref(b)), 20),
                 "policy_step": (lambda: lib.gm_ppo_learner_step_pi(learner._l), 20),
                 "value_gradient_and_reduce": (lambda: lib.gm_ppo_learner_grad_vf(learner._l, C.byref(b)), 20),
                 "value_step": (lambda: lib.gm_ppo_learner_step_vf(learner._l), 20)}
        split = {}
        for name, (fn, rep) in parts.items():
            def run():
                for _ in range(rep):
                    fn()
            ms = timed(run)
            split[name] = round(1000.0 * statistics.median(ms) / rep, 2)
        res.update(us_per_launch_group=split)
    learner.close()
    ac.close()
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ppo_learn.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=150, help="seconds per measurement")
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
    res["update_vs_torch_speedup"] = round(res["torch"]["ms_per_update"] / res["update"]["ms_per_update"], 2)
    res["update_faster_than_torch"] = res["update"]["ms_per_update"] < res["torch"]["ms_per_update"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
