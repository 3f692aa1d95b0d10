#!/usr/bin/env python3
"""Cost of one DQN update on the device ("DQN learner"): microseconds per update, canonical
network [63, 150, 100, 50, 8], batch 128, a 16-env context and a crafted replay memory of 10 000 rows, for
  train        gm_learner_train with 100 updates enqueued in one call (sample -> TD target ->
               gradient -> AdamW step -> soft update, no host synchronisation between them),
  calls        the same device sequence made call by call through the C ABI (gm_replay_sample,
               gm_policy_td_target, gm_learner_grad, gm_learner_step, gm_policy_soft_update),
  torch        the sequence it replaces on the same GPU: gm_replay_sample -> gm_policy_td_target ->
               torch forward / smooth-L1 loss / backward / clip_grad_value_ / AdamW(amsgrad) step /
               soft update of a torch target net -> two gm_policy_set_params (online and target).
Times are HIP events around 100 updates on the context's stream (which torch shares here), median of
`--reps` runs after a warm-up run.  Every measurement runs in a child process under its own time
limit; the first failure stops the run.  Writes profiles/dqn_learn.json.

usage: python tools/dqn_learn_time.py [--out profiles/dqn_learn.json] [--reps 5]"""
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

N_ENVS, ROWS, BATCH, UPDATES, SEED = 16, 10_000, 128, 100, 1234
GAMMA, TAU = 0.99, 0.05
CASES = ("train", "calls", "torch")


def child(case: str, reps: int) -> dict:
    import torch
    import gmx
    from gmx.policy import DevicePolicy, DeviceLearner, _batch_struct
    s = gmx.canonical_settings(noise=True, seed=SEED)
    s.continous_actions = 0
    env = gmx.BatchedGripperEnv(N_ENVS, object_set="set6_synthetic", settings=s, seed=SEED)
    env.reset()
    stream = torch.cuda.Stream()                         # (a non-null stream: the context launches on it)
    env.set_stream(stream.cuda_stream)
    lib = env.lib
    g = torch.Generator().manual_seed(11)
    buf = gmx.ReplayBuffer(env, ROWS)
    buf.state.copy_(torch.rand((ROWS, env.n_obs), generator=g) * 2 - 1)
    buf.action.copy_(torch.randint(0, env.n_actions, (ROWS,), generator=g, dtype=torch.int32))
    buf.next_state.copy_(torch.rand((ROWS, env.n_obs), generator=g) * 2 - 1)
    buf.reward.copy_(torch.randn((ROWS,), generator=g))
    buf.pushed = ROWS
    pol, tgt = DevicePolicy(env, seed=1), DevicePolicy(env, seed=2)
    learner = DeviceLearner(pol, tgt, soft_target_tau=TAU, gamma=GAMMA)
    batch = buf.sample(BATCH, seed=SEED, draw=0)
    out, r = _batch_struct(batch), buf.struct()
    y = torch.empty(BATCH, dtype=torch.float32, device="cuda")
    losses = torch.empty(UPDATES, dtype=torch.float32, device="cuda")
    f32p = C.POINTER(C.c_float)

    net = opt = tnet = None
    if case == "torch":
        sizes = pol.sizes

        def make(params):
            layers, pos = [], 0
            for i in range(len(sizes) - 1):
                lin = torch.nn.Linear(sizes[i], sizes[i + 1])
                n = sizes[i] * sizes[i + 1]
                lin.weight.data.copy_(torch.from_numpy(params[pos:pos + n].reshape(sizes[i + 1], sizes[i])))
                lin.bias.data.copy_(torch.from_numpy(params[pos + n:pos + n + sizes[i + 1]]))
                pos += n + sizes[i + 1]
                layers += [lin] + ([torch.nn.ReLU()] if i < len(sizes) - 2 else [torch.nn.Softmax(dim=1)])
            return torch.nn.Sequential(*layers).cuda()
        net, tnet = make(pol.params), make(tgt.params)
        opt = torch.optim.AdamW(net.parameters(), lr=1e-4, betas=(0.9, 0.999), amsgrad=True)
        crit = torch.nn.SmoothL1Loss()

    def flat(m):
        return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()

    def sample_and_target(u):
        rc = lib.gm_replay_sample(env.ctx, C.byref(r), len(buf), BATCH, C.c_uint64(SEED), C.c_uint64(u), C.byref(out))
        assert rc == 0, rc
        rc = lib.gm_policy_td_target(tgt._p, None, C.byref(out), BATCH, C.c_float(GAMMA), 0, C.c_void_p(y.data_ptr()), None)
        assert rc == 0, rc

    def run(i):
        if case == "train":
            rc = lib.gm_learner_train(learner._l, tgt._p, C.byref(r), len(buf), BATCH, C.c_uint64(SEED),
                                      C.c_uint64(i * UPDATES), UPDATES, C.c_float(GAMMA), 0, 0, C.c_float(TAU),
                                      C.c_void_p(losses.data_ptr()))
            assert rc == 0, rc
        elif case == "calls":
            for u in range(UPDATES):
                sample_and_target(i * UPDATES + u)
                assert lib.gm_learner_grad(learner._l, C.byref(out), C.c_void_p(y.data_ptr()), BATCH) == 0
                assert lib.gm_learner_step(learner._l) == 0
                assert lib.gm_policy_soft_update(tgt._p, pol._p, C.c_float(TAU)) == 0
        else:
            with torch.cuda.stream(stream):
                for u in range(UPDATES):
                    sample_and_target(i * UPDATES + u)
                    q = net(batch["state"]).gather(1, batch["action"].long()[:, None])
                    loss = crit(q, y[:, None])
                    opt.zero_grad()
                    loss.backward()
                    torch.nn.utils.clip_grad_value_(net.parameters(), 100)
                    opt.step()
                    with torch.no_grad():
                        for pt, po in zip(tnet.parameters(), net.parameters()):
                            pt.copy_(po * TAU + pt * (1 - TAU))
                    # the hand-back: both nets' new weights to the device policies through the host
                    for p, m in ((pol, net), (tgt, tnet)):
                        w = flat(m)
                        assert lib.gm_policy_set_params(p._p, w.ctypes.data_as(f32p)) == 0

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
    res = {"case": case, "batch": BATCH, "updates_per_run": UPDATES, "us_per_update": round(statistics.median(us), 2),
           "us_per_update_runs": [round(x, 2) for x in us]}
    learner.close()
    pol.close()
    tgt.close()
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dqn_learn.json"))
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
    res["train_vs_torch_speedup"] = round(res["torch"]["us_per_update"] / res["train"]["us_per_update"], 2)
    res["train_faster_than_torch"] = res["train"]["us_per_update"] < res["torch"]["us_per_update"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
