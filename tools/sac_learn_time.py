#!/usr/bin/env python3
"""Cost of one SAC update on the device ("SAC learner"): microseconds per update, canonical
continuous settings, (256, 256) nets, batch 128, 50 updates in a row (update_every_steps), a 16-env
context and a crafted action replay memory of 10 000 rows, for
  train        gm_sac_learner_train with the 50 updates enqueued in one call (sample -> backup ->
               critic gradient and step -> actor gradient and step -> polyak, no host
               synchronisation between them),
  calls        the same device sequence made call by call through the C ABI (gm_sac_replay_sample,
               gm_sac_target, gm_sac_learner_grad_q, _step_q, _grad_pi, _step_pi, gm_sac_soft_update),
  torch        the sequence it replaces on the same GPU: gm_sac_replay_sample -> gm_sac_target ->
               Agent_SAC.optimise_model's body in torch (loss_q, backward, Adam step, the critics
               frozen, loss_pi, backward, Adam step, polyak over a torch target module) -> two
               gm_sac_set_params (online and target).
Times are HIP events around the 50 updates on the context's stream (which torch shares here), median
of `--reps` runs after a warm-up run.  Every measurement runs in a child process under its own time
limit; the first failure stops the run.  Gate: train's median must not exceed calls' median plus
calls' own min-max spread (they are the same kernels); torch is reported, not gated.  Writes
profiles/sac_learn.json and exits 1 when the gate fails.

usage: python tools/sac_learn_time.py [--out profiles/sac_learn.json] [--reps 5]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gripper-mujoco_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

N_ENVS, ROWS, BATCH, UPDATES, SEED, NOISE_SEED = 16, 10_000, 128, 50, 1234, 99
GAMMA, ALPHA, TAU, HIDDEN = 0.99, 0.2, 0.05, (256, 256)
CASES = ("train", "calls", "torch")


def child(case: str, reps: int) -> dict:
    import torch
    import gmx
    from gmx.sac import DeviceSAC, DeviceSACLearner, ActionReplayBuffer, _batch_struct
    s = gmx.canonical_settings(noise=True, seed=SEED)           # the canonical continuous actions
    env = gmx.BatchedGripperEnv(N_ENVS, object_set="set6_synthetic", settings=s, seed=SEED)
    env.reset()
    stream = torch.cuda.Stream()                         # (a non-null stream: the context launches on it)
    env.set_stream(stream.cuda_stream)
    lib = env.lib
    g = torch.Generator().manual_seed(11)
    buf = ActionReplayBuffer(env, ROWS)
    buf.state.copy_(torch.rand((ROWS, env.n_obs), generator=g) * 2 - 1)
    buf.action.copy_(torch.rand((ROWS, env.n_actions), generator=g) * 2 - 1)
    buf.next_state.copy_(torch.rand((ROWS, env.n_obs), generator=g) * 2 - 1)
    buf.reward.copy_(torch.randn((ROWS,), generator=g))
    buf.pushed = ROWS
    onl, tgt = DeviceSAC(env, hidden=HIDDEN, seed=1), DeviceSAC(env, hidden=HIDDEN, seed=2)
    learner = DeviceSACLearner(onl, tgt, soft_target_tau=TAU, gamma=GAMMA, alpha=ALPHA)
    batch = buf.sample(BATCH, seed=SEED, draw=0)
    out, r = _batch_struct(batch), buf.struct()
    y = torch.empty(BATCH, dtype=torch.float32, device="cuda")
    losses = torch.empty((UPDATES, 2), dtype=torch.float32, device="cuda")
    f32p = C.POINTER(C.c_float)

    mod = tmod = q_opt = pi_opt = q_params = None
    if case == "torch":
        from sac_model import module_from_flat, logp_of
        mod = module_from_flat(env.n_obs, env.n_actions, HIDDEN, "relu", onl.params).cuda()
        tmod = module_from_flat(env.n_obs, env.n_actions, HIDDEN, "relu", tgt.params).cuda()
        q_params = list(mod.q1.parameters()) + list(mod.q2.parameters())
        q_opt = torch.optim.Adam(q_params, lr=1e-4, betas=(0.9, 0.999))
        pi_opt = torch.optim.Adam(mod.pi.parameters(), lr=1e-4, betas=(0.9, 0.999))

    def flat(m):
        return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()

    def sample_and_target(d):
        rc = lib.gm_sac_replay_sample(env.ctx, C.byref(r), len(buf), BATCH, C.c_uint64(SEED), C.c_uint64(d), C.byref(out))
        assert rc == 0, rc
        rc = lib.gm_sac_target(tgt._p, onl._p, C.byref(out), BATCH, C.c_float(GAMMA), C.c_float(ALPHA), 0,
                               C.c_uint64(NOISE_SEED), C.c_uint64(2 * d), C.c_void_p(y.data_ptr()), None, None, None, None)
        assert rc == 0, rc

    def run(i):
        if case == "train":
            rc = lib.gm_sac_learner_train(learner._l, tgt._p, C.byref(r), len(buf), BATCH, C.c_uint64(SEED),
                                          C.c_uint64(NOISE_SEED), C.c_uint64(i * UPDATES), UPDATES, C.c_float(GAMMA),
                                          C.c_float(ALPHA), 0, C.c_float(TAU), C.c_void_p(losses.data_ptr()))
            assert rc == 0, rc
        elif case == "calls":
            for u in range(UPDATES):
                d = i * UPDATES + u
                sample_and_target(d)
                assert lib.gm_sac_learner_grad_q(learner._l, C.byref(out), C.c_void_p(y.data_ptr()), BATCH) == 0
                assert lib.gm_sac_learner_step_q(learner._l) == 0
                assert lib.gm_sac_learner_grad_pi(learner._l, C.byref(out), BATCH, C.c_float(ALPHA), C.c_uint64(NOISE_SEED),
                                                  C.c_uint64(2 * d + 1), None, None, None, None, None, None) == 0
                assert lib.gm_sac_learner_step_pi(learner._l) == 0
                assert lib.gm_sac_soft_update(tgt._p, onl._p, C.c_float(TAU)) == 0
        else:
            with torch.cuda.stream(stream):
                for u in range(UPDATES):
                    sample_and_target(i * UPDATES + u)
                    o, a = batch["state"], batch["action"]
                    x = torch.cat([o, a], dim=-1)
                    q_opt.zero_grad()
                    loss_q = ((mod.q1.q(x)[:, 0] - y) ** 2).mean() + ((mod.q2.q(x)[:, 0] - y) ** 2).mean()
                    loss_q.backward()
                    q_opt.step()
                    for p in q_params:
                        p.requires_grad = False
                    pi_opt.zero_grad()
                    h = mod.pi.net(o)
                    mu, ls = mod.pi.mu_layer(h), torch.clamp(mod.pi.log_std_layer(h), -20.0, 2.0)
                    uu = mu + torch.exp(ls) * torch.randn_like(mu)
                    xp = torch.cat([o, torch.tanh(uu)], dim=-1)
                    loss_pi = (ALPHA * logp_of(uu, mu, ls) - torch.min(mod.q1.q(xp)[:, 0], mod.q2.q(xp)[:, 0])).mean()
                    loss_pi.backward()
                    pi_opt.step()
                    for p in q_params:
                        p.requires_grad = True
                    with torch.no_grad():
                        for pt, po in zip(tmod.parameters(), mod.parameters()):
                            pt.mul_(1 - TAU)
                            pt.add_(TAU * po)
                    # the hand-back: both modules' new weights to the device handles through the host
                    for p, m in ((onl, mod), (tgt, tmod)):
                        w = flat(m)
                        assert lib.gm_sac_set_params(p._p, w.ctypes.data_as(f32p)) == 0

    run(0)                                               # warm-up
    torch.cuda.synchronize()
    us = []
    for i in range(1, 1 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        run(i)
        e1.record(stream)
        torch.cuda.synchronize()
        us.append(1000.0 * e0.elapsed_time(e1) / UPDATES)
    res = {"case": case, "batch": BATCH, "hidden": list(HIDDEN), "updates_per_run": UPDATES,
           "us_per_update": round(statistics.median(us), 2), "us_per_update_runs": [round(x, 2) for x in us]}
    learner.close()
    onl.close()
    tgt.close()
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sac_learn.json"))
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
    calls = res["calls"]["us_per_update_runs"]
    res["gate_train_le_calls_plus_spread"] = res["train"]["us_per_update"] <= res["calls"]["us_per_update"] + (max(calls) - min(calls))
    res["calls_spread_us"] = round(max(calls) - min(calls), 2)
    res["train_vs_torch_speedup"] = round(res["torch"]["us_per_update"] / res["train"]["us_per_update"], 2)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if res["gate_train_le_calls_plus_spread"] else 1


if __name__ == "__main__":
    sys.exit(main())
