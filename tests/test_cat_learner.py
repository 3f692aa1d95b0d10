"""The on-device PPO learner on a categorical actor-critic (gm_ppo_grad_pi_cat_kernel and the shared
reduce / step kernels) against torch autograd and torch.optim on the CPU, on crafted batches.

The model: pi = Categorical(logits = logits_net(obs)); the buffer's action is [n, 1] float, read
as act.squeeze(-1).long(), so logp = pi.log_prob(that) has shape [n] (the section's
deviations).  Losses are Agent_PPO.compute_loss_pi's with ent = pi.entropy().mean().

Tolerances are tests/test_ppo_learner.py's, through its own check_scalar and check_grads: every
expected value is computed in float32 and in float64, and the device must agree with the float64
one within 8 x max|f32 - f64| + one f32 ulp of the largest magnitude, per parameter tensor; for a
scalar, over the crafted batch's per-row values.

The critic's kernel and sizes are the Gaussian learner's, so its gradients are checked on
test_ppo_learner.py's own crafted critic parameters, observations and returns, behind this file's
categorical actor in the [actor | critic] blob.  The output bias's gradient is one number, and a
one-number tensor's bound is 8 x whatever torch's f32 value of it happens to differ from the f64
one: on that file's rows the bound is known to cover an f32 evaluation of the sum (ratio 0.58 at
worst); this file's own returns give no such assurance, and nothing about the critic is new here
but the blob around it.

Crafted data: obs uniform in [-1, 1] with columns 0 and 1 zero; "old" parameters and "new" = old
+ a perturbation; act ~ Categorical(old logits); logp_old from the old parameters in float64,
rounded to f32; adv and ret standard normal.  The parameter seed is the first below 64 for which
every row's r is further from 1 -+ eps than the bound on r and all five clip branches occur
(test_ppo_learner.py's clear_of_edges guard, on this model).  Rows 5, 6, 7 are switched by
columns 0 / 1 through one saturated unit per hidden layer (weights 20, the same in old and new):
  row 5: logits += (60, -60, 0, ...): a spread of ~120, e_1 = expf(-120) == 0 in f32; takes class 0
  row 6: the same logits, takes class 1: the taken class has e == 0, p == 0, logp ~ -120
  row 7: logits += (16, 0, ...), takes class 3: its probability is below 1e-6
A class with e_j == 0 must add exactly 0 to the row's entropy (0 x a finite logp_j): a NaN or inf
there would reach ent and the gradient, which are compared within the bound (and asserted finite).
Measured worst |device - f64| / bound: see DESIGN.md, "Categorical PPO"."""

import ctypes as C

import numpy as np
import pytest

from conftest import gpu_available
from test_replay_sample_td import bound
from test_dqn_learner import tensors, split
import test_ppo_learner as gauss
from test_ppo_learner import (mlp, branches, device_batch, check_scalar, check_grads, vf_indices, same_learner_bytes,
                              same_info, EPS, ROWS, NS, NO_STOP, MODES)

pytestmark = pytest.mark.gpu

N_ENVS, N_OBS, N_ACT = 16, 63, 8
HIDDEN = {"20-20": (20, 20), "64-64": (64, 64), "spill": (256, 256, 200)}
PERTURB = {"20-20": 0.10, "64-64": 0.05, "spill": 0.03}     # std of new - old: r lands on both sides of 1 -+ eps
CRAFTED_ROWS = (5, 6, 7)
SWITCH = 20.0
LIFT = (np.array([60, -60, 0, 0, 0, 0, 0, 0], np.float32), np.array([16, 0, 0, 0, 0, 0, 0, 0], np.float32))


def sizes_of(net):
    return [N_OBS, *HIDDEN[net], N_ACT], [N_OBS, *HIDDEN[net], 1]


def parts(asz, csz, flat):
    na = sum(asz[i] * asz[i + 1] + asz[i + 1] for i in range(len(asz) - 1))
    assert flat.size == na + sum(csz[i] * csz[i + 1] + csz[i + 1] for i in range(len(csz) - 1))
    return flat[:na], flat[na:]


def names(asz, csz):
    return [f"pi.{'W' if i % 2 == 0 else 'b'}{i // 2}" for i in range(2 * (len(asz) - 1))] + \
        [f"vf.{'W' if i % 2 == 0 else 'b'}{i // 2}" for i in range(2 * (len(csz) - 1))]


def split_all(asz, csz, flat):
    a, c = parts(asz, csz, flat)
    return split(asz, a) + split(csz, c)


def switches(asz, flat):
    """Impose the two switch paths on the actor's part of flat parameters (in place): obs column
    s -> unit s of every hidden layer with weight SWITCH and nothing else into that unit, then
    LIFT[s] on the logits."""
    ts = split(asz, flat)
    for s in (0, 1):
        for l in range(len(asz) - 2):
            W = ts[2 * l].reshape(asz[l + 1], asz[l])
            W[s, :] = 0.0
            W[s, s] = SWITCH
            ts[2 * l + 1][s] = 0.0
        ts[-2].reshape(N_ACT, asz[-2])[:, s] = LIFT[s]


def craft(net, seed, rows=ROWS):
    """(new flat parameters, batch as f32 numpy) of the module docstring for one parameter seed."""
    import torch
    from gmx.ppo import init_params
    asz, csz = sizes_of(net)
    g = torch.Generator().manual_seed(1000 + seed)
    old = init_params(asz, csz, seed, categorical=True)
    new = (old.astype(np.float64) + PERTURB[net] * torch.randn(old.size, generator=g, dtype=torch.float64).numpy()).astype(np.float32)
    switches(asz, old)
    switches(asz, new)
    obs = (torch.rand((rows, N_OBS), generator=g) * 2 - 1).numpy()
    obs[:, :2] = 0.0
    obs[5, 0] = obs[6, 0] = obs[7, 1] = 1.0
    with torch.no_grad():
        logits = mlp(tensors(asz, parts(asz, csz, old)[0], torch.float64), torch.from_numpy(obs).double())
        lsm = torch.log_softmax(logits, dim=-1)
        act = torch.multinomial(torch.exp(lsm), 1, generator=g)[:, 0]
        act[5], act[6], act[7] = 0, 1, 3
        logp = lsm.gather(1, act[:, None])[:, 0].float()
    batch = dict(obs=obs, act=act.float().numpy()[:, None].copy(), logp=logp.numpy(),
                 adv=torch.randn(rows, generator=g).numpy(), ret=torch.randn(rows, generator=g).numpy())
    return new, batch


def loss_pi(asz, csz, flat, batch, n, dtype, opts, grad=True, rows=None):
    """compute_loss_pi in torch on the CPU (rows: an index list instead of the prefix n)."""
    import torch
    sel = slice(0, n) if rows is None else list(rows)
    ts = tensors(asz, parts(asz, csz, flat)[0], dtype, grad=grad)
    obs, adv, lold = (torch.from_numpy(batch[k][sel]).to(dtype) for k in ("obs", "adv", "logp"))
    act = torch.from_numpy(batch["act"][sel]).squeeze(-1).long()             # the stated reading
    logits = mlp(ts, obs)
    pi = torch.distributions.Categorical(logits=logits)
    logp = pi.log_prob(act)
    ratio = torch.exp(logp - lold)
    beta = opts.get("kl_penalty_coefficient", 0.2)
    if opts.get("use_kl_penalty"):
        per_row = -(ratio * adv) + beta * (lold - logp)
        loss = -(ratio * adv).mean() + beta * (lold - logp).mean()
    else:
        per_row = -torch.min(ratio * adv, torch.clamp(ratio, 1 - EPS, 1 + EPS) * adv)
        loss = per_row.mean()
    ent_rows = pi.entropy()
    if opts.get("use_entropy_regularisation"):
        loss = loss - opts["entropy_coefficient"] * ent_rows.mean()
    if grad:
        loss.backward()
    clipped = ratio.gt(1 + EPS) | ratio.lt(1 - EPS)
    return dict(loss=loss.detach(), rows=per_row.detach(), r=ratio.detach(), kl_rows=(lold - logp).detach(),
                kl=(lold - logp).mean().detach(), ent_rows=ent_rows.detach(), ent=ent_rows.mean().detach(),
                clipped=int(clipped.sum()), logits=logits.detach(), probs=pi.probs.detach(),
                grads=[t.grad for t in ts] if grad else None)


def clear_of_edges(net, flat, batch):
    """Every row's r beyond the bound on r from 1 - eps and 1 + eps, and all five branches present."""
    import torch
    asz, csz = sizes_of(net)
    r32 = loss_pi(asz, csz, flat, batch, ROWS, torch.float32, {}, grad=False)["r"]
    r64 = loss_pi(asz, csz, flat, batch, ROWS, torch.float64, {}, grad=False)["r"]
    edge = float(torch.minimum((r64 - (1 - EPS)).abs(), (r64 - (1 + EPS)).abs()).min())
    br = branches(r64.numpy(), batch["adv"].astype(np.float64))
    return edge > bound(r32, r64) and min(br) > 0, (edge, bound(r32, r64), br)


_CRAFTED = {}


def crafted(net):
    """(seed, new parameters, batch, figures): computed once per net and left unchanged."""
    if net not in _CRAFTED:
        for seed in range(64):
            flat, batch = craft(net, seed)
            ok, fig = clear_of_edges(net, flat, batch)
            if ok:
                _CRAFTED[net] = (seed, flat, batch, fig)
                break
        else:
            raise AssertionError("no parameter seed below 64 keeps every row clear of the clip edges with all branches")
    return _CRAFTED[net]


def make_discrete_env(gm, n):
    s = gm.canonical_settings(noise=True, seed=17)
    s.continous_actions = 0
    e = gm.BatchedGripperEnv(n, object_set="set6_synthetic", settings=s, seed=17)
    e.reset()
    return e


@pytest.fixture(scope="module")
def env(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    e = make_discrete_env(gm, N_ENVS)
    assert (e.n_obs, e.n_actions) == (N_OBS, N_ACT)
    yield e
    e.close()


def make_ac(env, net, flat):
    from gmx.ppo import DeviceCategoricalActorCritic
    asz, csz = sizes_of(net)
    return DeviceCategoricalActorCritic(env, actor_sizes=asz, critic_sizes=csz, params=flat)


def pi_indices(asz, csz):
    return list(range(2 * (len(asz) - 1)))


def check_pi(tag, learner, net, flat, batch, n, opts, worst):
    import torch
    asz, csz = sizes_of(net)
    learner.grad_pi(device_batch(batch, n))
    g_dev, sc = learner.read()
    r32 = loss_pi(asz, csz, flat, batch, n, torch.float32, opts)
    r64 = loss_pi(asz, csz, flat, batch, n, torch.float64, opts)
    f32, f64 = (loss_pi(asz, csz, flat, batch, ROWS, dt, opts, grad=False) for dt in (torch.float32, torch.float64))
    assert all(np.isfinite(sc[k]) for k in ("loss_pi", "kl", "ent", "cf")), (tag, sc)
    check_scalar(tag, sc["loss_pi"], r32["loss"], r64["loss"], f32["rows"], f64["rows"], worst, "loss_pi")
    check_scalar(tag, sc["kl"], r32["kl"], r64["kl"], f32["kl_rows"], f64["kl_rows"], worst, "kl")
    check_scalar(tag, sc["ent"], r32["ent"], r64["ent"], f32["ent_rows"], f64["ent_rows"], worst, "ent")
    assert r32["clipped"] == r64["clipped"]
    assert sc["cf"] == np.float32(r64["clipped"]) / np.float32(n), (tag, sc["cf"], r64["clipped"], n)
    assert np.isfinite(g_dev).all(), tag
    check_grads(tag, asz, csz, g_dev, pi_indices(asz, csz), r32["grads"], r64["grads"], worst)


def critic_case(net):
    """(flat parameters of this file's actor and test_ppo_learner.py's crafted critic, that file's
    sizes, parameters and batch): the critic's sizes are the same in both files."""
    asz, csz = sizes_of(net)
    gasz, gcsz = gauss.sizes_of(net)
    assert gcsz == csz
    _, gflat, gbatch, _ = gauss.crafted(net)
    flat = np.concatenate([parts(asz, csz, crafted(net)[1])[0], gauss.parts(gasz, gcsz, gflat)[1]])
    return flat, (gasz, gcsz, gflat, gbatch)


def check_vf(tag, learner, net, case, n, worst):
    """test_ppo_learner.check_vf's comparisons, with the device's gradient in this blob's flat order."""
    import torch
    asz, csz = sizes_of(net)
    gasz, gcsz, gflat, gbatch = case
    learner.grad_vf(device_batch(gbatch, n))
    g_dev, sc = learner.read()
    r32, r64 = (gauss.loss_v(gasz, gcsz, gflat, gbatch, n, dt) for dt in (torch.float32, torch.float64))
    f32, f64 = (gauss.loss_v(gasz, gcsz, gflat, gbatch, ROWS, dt) for dt in (torch.float32, torch.float64))
    check_scalar(tag, sc["loss_v"], r32["loss"], r64["loss"], f32["rows"], f64["rows"], worst, "loss_v")
    check_grads(tag, asz, csz, g_dev, vf_indices(asz, csz), r32["grads"], r64["grads"], worst)


def test_crafted_rows_are_what_they_claim(gm):
    """CPU only (torch): the spread, the exact zeros and the rare action of rows 5 - 7, and the
    five clip branches, on the float32 and float64 models."""
    import torch
    for net in sorted(HIDDEN):
        asz, csz = sizes_of(net)
        seed, flat, batch, fig = crafted(net)
        ok, fig = clear_of_edges(net, flat, batch)
        assert ok and min(fig[2]) > 0, f"a row on a clip edge or a branch missing: {fig}"
        print(f"{net}: seed {seed}, nearest clip edge {fig[0]:.2e} vs bound on r {fig[1]:.2e}, rows per branch {fig[2]}")
        r = loss_pi(asz, csz, flat, batch, ROWS, torch.float64, {}, grad=False)
        x = r["logits"].numpy()
        assert (x[[5, 6]].max(1) - x[[5, 6]].min(1) > 100).all()
        x32 = x[[5, 6]].astype(np.float32)
        e32 = np.exp(x32 - x32.max(1, keepdims=True))
        assert (e32[:, 1] == 0).all() and (e32[:, 0] == 1).all()              # e_1 underflows to exactly 0 in f32
        p = r["probs"].numpy()
        assert p[6, 1] < 1e-40 and 0 < p[7, 3] < 1e-6 and p[5, 0] > 0.999
        assert batch["act"][5, 0] == 0 and batch["act"][6, 0] == 1 and batch["act"][7, 0] == 3
        assert np.isfinite(batch["logp"]).all() and batch["logp"][6] < -100
        assert np.abs(x[8:]).max() < 20                                       # the other rows are ordinary


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("net", sorted(HIDDEN))
def test_actor_gradients_match_autograd(gm, env, net, mode):
    from gmx.ppo import DevicePPOLearner
    seed, flat, batch, fig = crafted(net)
    opts = MODES[mode]
    ac = make_ac(env, net, flat)
    learner, three = DevicePPOLearner(ac, **opts), DevicePPOLearner(ac, n_groups=3, **opts)
    worst = {}
    try:
        for n in NS:
            check_pi(f"{net} {mode} n {n}", learner, net, flat, batch, n, opts, worst)
        # 8 tiles over 3 workgroups, unevenly, the last tile partial: a workgroup adds several tiles up
        check_pi(f"{net} {mode} n {ROWS} G 3", three, net, flat, batch, ROWS, opts, worst)
        print(f"{net} {mode}: worst |device - f64| / bound {worst}")
    finally:
        learner.close()
        three.close()
        ac.close()


@pytest.mark.parametrize("mode", ["clip-entropy", "kl"])
def test_crafted_rows_alone(gm, env, mode):
    """Rows 5 - 7 as a batch of their own (n = 3): nothing averages their terms away."""
    import torch
    from gmx.ppo import DevicePPOLearner
    net = "20-20"
    asz, csz = sizes_of(net)
    _, flat, batch, _ = crafted(net)
    opts = MODES[mode]
    sub = {k: np.ascontiguousarray(v[list(CRAFTED_ROWS)]) for k, v in batch.items()}
    ac = make_ac(env, net, flat)
    learner = DevicePPOLearner(ac, **opts)
    worst = {}
    try:
        learner.grad_pi(device_batch(sub, 3))
        g_dev, sc = learner.read()
        r32, r64 = (loss_pi(asz, csz, flat, batch, 0, dt, opts, rows=CRAFTED_ROWS) for dt in (torch.float32, torch.float64))
        assert np.isfinite(g_dev).all() and all(np.isfinite(v) for v in sc.values()), sc
        for key, rows in (("loss_pi", "rows"), ("kl", "kl_rows"), ("ent", "ent_rows")):
            check_scalar(f"crafted {mode}", sc[key], r32["loss" if key == "loss_pi" else key],
                         r64["loss" if key == "loss_pi" else key], r32[rows], r64[rows], worst, key)
        check_grads(f"crafted {mode}", asz, csz, g_dev, pi_indices(asz, csz), r32["grads"], r64["grads"], worst)
        print(f"crafted rows {mode}: worst |device - f64| / bound {worst}")
    finally:
        learner.close()
        ac.close()


@pytest.mark.parametrize("net", sorted(HIDDEN))
def test_critic_gradients_match_autograd(gm, env, net):
    from gmx.ppo import DevicePPOLearner
    flat, case = critic_case(net)
    ac = make_ac(env, net, flat)
    learner, three = DevicePPOLearner(ac), DevicePPOLearner(ac, n_groups=3)
    worst = {}
    try:
        for n in NS:
            check_vf(f"{net} n {n}", learner, net, case, n, worst)
        check_vf(f"{net} n {ROWS} G 3", three, net, case, ROWS, worst)
        print(f"{net} critic: worst |device - f64| / bound {worst}")
    finally:
        learner.close()
        three.close()
        ac.close()


@pytest.mark.parametrize("net", sorted(HIDDEN))
def test_grad_is_deterministic(gm, env, net):
    from gmx.ppo import DevicePPOLearner
    _, flat, batch, _ = crafted(net)
    ac = make_ac(env, net, flat)
    learners = {g: DevicePPOLearner(ac, n_groups=g, use_entropy_regularisation=True, entropy_coefficient=0.01)
                for g in (3, 5)}
    try:
        data = device_batch(batch, ROWS)
        for g, l in learners.items():
            l.grad_pi(data)
            g1, s1 = l.read()
            l.grad_vf(data)                                  # another gradient in between
            l.grad_pi(device_batch(batch, 37))
            l.grad_pi(data)
            g2, s2 = l.read()
            a, c = parts(*sizes_of(net), g1)
            a2, c2 = parts(*sizes_of(net), g2)
            assert a.tobytes() == a2.tobytes()
            assert all(s1[k].tobytes() == s2[k].tobytes() for k in s1 if k != "loss_v")
            assert np.abs(c).max() == 0 and np.abs(c2).max() > 0 and np.abs(a).max() > 0     # vf's gradient is held too
    finally:
        for l in learners.values():
            l.close()
        ac.close()


@pytest.mark.parametrize("optimiser", ["adam", "adamW"])
def test_optimiser_steps_match_torch_elementwise(gm, env, optimiser):
    import torch
    from gmx.ppo import DevicePPOLearner, pack
    net = "64-64"
    asz, csz = sizes_of(net)
    _, flat, batch, _ = crafted(net)
    packed0, coff, end = pack(asz, csz, flat, categorical=True)
    assert end == packed0.size
    data = device_batch(batch, ROWS)
    nm = names(asz, csz)
    lrs = dict(pi=3e-4, vf=1e-3)
    idx = dict(pi=pi_indices(asz, csz), vf=vf_indices(asz, csz))
    ac = make_ac(env, net, flat)
    probe = DevicePPOLearner(ac)
    learner = clone = copy = None
    worst = 0.0
    try:
        probe.grad_pi(data)
        probe.grad_vf(data)
        g0 = np.abs(probe.read()[0])
        clamp = float(np.median(g0[g0 > 0]))                # both sides of the clamp occur
        assert clamp > 0 and (g0 > clamp).any() and ((g0 < clamp) & (g0 > 0)).any()
        learner = DevicePPOLearner(ac, optimiser=optimiser, grad_clamp_value=clamp)
        cls = torch.optim.AdamW if optimiser == "adamW" else torch.optim.Adam
        kw = dict(amsgrad=True) if optimiser == "adamW" else {}
        ref = {}
        for dt in (torch.float32, torch.float64):
            a, c = parts(asz, csz, flat)
            ts = tensors(asz, a, dt, grad=True) + tensors(csz, c, dt, grad=True)
            ref[dt] = (ts, {w: cls([ts[i] for i in idx[w]], lr=lrs[w], betas=(0.9, 0.999), **kw) for w in ("pi", "vf")})
        for step in range(1, 6):
            for w in ("pi", "vf"):
                packed_before = ac.get_packed()
                (learner.grad_pi if w == "pi" else learner.grad_vf)(data)
                g = torch.clamp(torch.from_numpy(learner.read()[0]), -clamp, clamp)     # the device's own gradient
                (learner.step_pi if w == "pi" else learner.step_vf)()
                packed_after = ac.get_packed()
                p_dev = split_all(asz, csz, ac.get_params())
                gs = split_all(asz, csz, g.numpy())
                for dt, (ts, opts) in ref.items():
                    for i in idx[w]:
                        ts[i].grad = torch.from_numpy(gs[i].copy()).reshape(ts[i].shape).to(dt)
                    opts[w].step()
                for i in idx[w]:
                    t32, t64 = (ref[dt][0][i].detach().reshape(-1) for dt in (torch.float32, torch.float64))
                    b = bound(t32, t64)
                    err = float(np.abs(p_dev[i].astype(np.float64) - t64.numpy()).max())
                    worst = max(worst, err / b)
                    assert err <= b, f"{optimiser} {w} step {step} {nm[i]}: {err:.3e} > {b:.3e}"
                lo, hi = (coff, end) if w == "pi" else (0, coff)      # the other optimiser's range keeps its bytes
                assert packed_before[lo:hi].tobytes() == packed_after[lo:hi].tobytes(), f"{w} stepped the other's weights"
                assert packed_before.tobytes() != packed_after.tobytes()
            print(f"{optimiser} step {step}: worst |device - f64| / bound so far {worst:.3f}")
        # the state round trip carries no log_std entries: exactly the flat parameter count
        state = learner.state()
        assert state["exp_avg"].size == flat.size == ac.get_params().size
        assert state["step_pi"] == 5 and state["step_vf"] == 5 and np.abs(state["exp_avg"]).max() > 0
        copy = make_ac(env, net, ac.get_params())
        clone = DevicePPOLearner(copy, optimiser=optimiser, grad_clamp_value=clamp)
        clone.load_state(state)
        for l in (learner, clone):
            l.grad_pi(data)
            l.step_pi()
            l.grad_vf(data)
            l.step_vf()
        assert ac.get_packed().tobytes() == copy.get_packed().tobytes()
        s1, s2 = learner.state(), clone.state()
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert s1[k].tobytes() == s2[k].tobytes(), k
    finally:
        for l in (probe, learner, clone):
            if l is not None:
                l.close()
        if copy is not None:
            copy.close()
        ac.close()


# ---- update: a trajectory buffer filled from torch with the crafted rows
K_TRAJ = 8                        # 8 env-steps x 16 envs = 128 rows
ITERS = 6
UPD = dict(train_pi_iters=ITERS, train_vf_iters=ITERS, learning_rate_pi=3e-3, grad_clamp_value=0.05)


def fill_traj(env, net):
    """A TrajectoryBuffer(act_dim=1) holding 128 crafted rows (end cycling 0 / 0 / 1 / 0 / 2), and the new parameters."""
    import torch
    from gmx.ppo import TrajectoryBuffer
    seed, _, _, _ = crafted(net)
    flat, batch = craft(net, seed, rows=K_TRAJ * N_ENVS)
    g = torch.Generator().manual_seed(77)
    traj = TrajectoryBuffer(env, K_TRAJ, act_dim=1)
    traj.obs.copy_(torch.from_numpy(batch["obs"]).reshape(K_TRAJ, N_ENVS, N_OBS))
    traj.act.copy_(torch.from_numpy(batch["act"]).reshape(K_TRAJ, N_ENVS, 1))
    traj.logp.copy_(torch.from_numpy(batch["logp"]).reshape(K_TRAJ, N_ENVS))
    traj.val.copy_(torch.randn((K_TRAJ, N_ENVS), generator=g))
    traj.rew.copy_(torch.randn((K_TRAJ, N_ENVS), generator=g))
    end = torch.tensor([0, 0, 1, 0, 2], dtype=torch.uint8).repeat(K_TRAJ * N_ENVS // 5 + 1)[:K_TRAJ * N_ENVS]
    traj.end.copy_(end.reshape(K_TRAJ, N_ENVS))
    traj.boot.copy_(torch.randn((K_TRAJ, N_ENVS), generator=g) * (end.reshape(K_TRAJ, N_ENVS) == 2))
    traj.last_val.copy_(torch.randn((N_ENVS,), generator=g))
    torch.cuda.synchronize()
    return traj, flat


def by_calls(env, learner, traj, opts, iters, stop_at=None):
    """optimise_model through the single calls, the host reading kl and breaking as the reference
    does: returns (per-iteration kl, policy steps taken, first scalars, last scalars)."""
    from gmx.ppo import adv_normalise
    adv, ret = traj.gae(opts.get("gamma", 0.99), opts.get("lam", 0.97))
    adv_normalise(env, adv)
    data = dict(obs=traj.obs.reshape(-1, N_OBS), act=traj.act.reshape(-1, 1), logp=traj.logp.reshape(-1),
                adv=adv.reshape(-1), ret=ret.reshape(-1))
    kls, first, last, steps = [], {}, {}, 0
    for i in range(iters):
        learner.grad_pi(data)
        sc = learner.read()[1]
        kls.append(float(sc["kl"]))
        for k in ("loss_pi", "kl", "ent", "cf"):
            last[k] = sc[k]
            first.setdefault(k, sc[k])
        if stop_at is not None and float(sc["kl"]) > stop_at:
            break
        learner.step_pi()
        steps += 1
    for i in range(iters):
        learner.grad_vf(data)
        sc = learner.read()[1]
        last["loss_v"] = sc["loss_v"]
        first.setdefault("loss_v", sc["loss_v"])
        learner.step_vf()
    return kls, steps, first, last


@pytest.mark.parametrize("optimiser", ["adam", "adamW"])
def test_update_equals_the_calls_it_enqueues(gm, env, optimiser):
    from gmx.ppo import DevicePPOLearner
    net = "64-64"
    traj, flat = fill_traj(env, net)
    opts = dict(UPD, optimiser=optimiser, use_entropy_regularisation=True, entropy_coefficient=0.01, **NO_STOP)
    a, b = make_ac(env, net, flat), make_ac(env, net, flat)
    fused, calls = DevicePPOLearner(a, n_groups=3, **opts), DevicePPOLearner(b, n_groups=3, **opts)
    try:
        info = fused.update(traj)
        kls, steps, first, last = by_calls(env, calls, traj, opts, ITERS)
        assert info["pi_iters_done"] == steps == ITERS
        same_learner_bytes(a, b, fused, calls)
        same_info(info, first, last)
        assert fused.state()["step_pi"] == ITERS and fused.state()["step_vf"] == ITERS
        assert np.isfinite(a.get_params()).all() and a.get_params().tobytes() != flat.tobytes()
        assert float(info["first"]["ent"]) > 0
    finally:
        fused.close()
        calls.close()
        a.close()
        b.close()


def test_kl_stop(gm, env):
    from gmx.ppo import DevicePPOLearner, pack
    net = "64-64"
    asz, csz = sizes_of(net)
    traj, flat = fill_traj(env, net)
    p0, coff, _ = pack(asz, csz, flat, categorical=True)
    free = dict(UPD, **NO_STOP)
    acs, learners = [], []

    def pair(opts, params=flat):
        ac = make_ac(env, net, params)
        acs.append(ac)
        learners.append(DevicePPOLearner(ac, n_groups=5, **opts))
        return ac, learners[-1]
    try:
        ref_ac, ref = pair(free)
        kls, _, _, _ = by_calls(env, ref, traj, free, ITERS)
        print("kl per policy iteration:", kls)
        rising = [j for j in range(0, ITERS - 1) if kls[j] < kls[j + 1] and max(kls[:j + 1]) < 0.5 * (kls[j] + kls[j + 1])]
        assert rising, f"no pair of consecutive iterations with kl_j < kl_j+1 above every earlier kl: {kls}"
        j = rising[-1] if rising[-1] > 0 else rising[0]
        thr = 0.5 * (kls[j] + kls[j + 1])
        assert sum(k <= thr for k in kls[:j + 2]) == j + 1
        stop = dict(UPD, target_kl=thr, max_kl_ratio=1.0)

        # the stop inside update against the host loop that breaks as the reference does
        a, la = pair(stop)
        b, lb = pair(stop)
        info = la.update(traj)
        _, steps, first, last = by_calls(env, lb, traj, stop, ITERS, stop_at=thr)
        assert info["pi_iters_done"] == steps == j + 1
        assert la.state()["step_pi"] == j + 1 and la.state()["step_vf"] == ITERS
        same_learner_bytes(a, b, la, lb)
        same_info(info, first, last)
        assert np.float64(info["last"]["kl"]) > thr
        pa, pref = a.get_packed(), ref_ac.get_packed()
        assert pa[coff:].tobytes() == pref[coff:].tobytes()             # the critic: all its iterations, the same bytes
        if j + 1 < ITERS:
            assert pa[:coff].tobytes() != pref[:coff].tobytes()         # fewer policy steps than the free run

        # a threshold below kl_0: no policy step at all, the actor's bytes unchanged, the critic trained
        c, lc = pair(dict(UPD, target_kl=kls[0] - abs(kls[0]) * 0.5 - 1e-6, max_kl_ratio=1.0))
        info3 = lc.update(traj)
        pc = c.get_packed()
        assert info3["pi_iters_done"] == 0 and lc.state()["step_pi"] == 0 and lc.state()["step_vf"] == ITERS
        assert pc[:coff].tobytes() == p0[:coff].tobytes()
        assert pc[coff:].tobytes() == pref[coff:].tobytes()
        assert info3["first"]["kl"].tobytes() == info3["last"]["kl"].tobytes() == np.float32(kls[0]).tobytes()
    finally:
        for l in learners:
            l.close()
        for ac in acs:
            ac.close()


def test_padding_stays_zero_under_training(gm, env):
    from gmx.ppo import DevicePPOLearner, pack
    net = "20-20"
    asz, csz = sizes_of(net)
    traj, flat = fill_traj(env, net)
    ac = make_ac(env, net, flat)
    learner = DevicePPOLearner(ac, optimiser="adamW", train_pi_iters=2, train_vf_iters=2, learning_rate_pi=1e-3,
                               use_entropy_regularisation=True, **NO_STOP)         # AdamW: weight decay and amsgrad
    try:
        pad = pack(asz, csz, np.ones(flat.size, dtype=np.float32), categorical=True)[0] == 0
        assert pad.any()
        before = ac.get_packed()
        assert (before[pad] == 0.0).all()
        for _ in range(20):
            learner.update(traj)
        packed = ac.get_packed()
        assert (packed[pad] == 0.0).all(), f"{int((packed[pad] != 0).sum())} padding entries moved"
        assert (packed[~pad] != before[~pad]).mean() > 0.9            # and the weights did move
        assert np.isfinite(packed).all()
    finally:
        learner.close()
        ac.close()


def test_it_learns(gm, env):
    """loss_v over 30 short updates on a fixed buffer against the torch model's own fall on the
    same rows and returns (Adam, lr 1e-3, 4 iterations an update): both fall, the device's by at
    least 0.9 of the torch model's (the two are the same algorithm in f32; they differ by rounding)."""
    import torch
    from gmx.ppo import DevicePPOLearner
    net = "64-64"
    asz, csz = sizes_of(net)
    traj, flat = fill_traj(env, net)
    ac = make_ac(env, net, flat)
    learner = DevicePPOLearner(ac, train_pi_iters=4, train_vf_iters=4, **NO_STOP)
    try:
        _, ret = traj.gae(0.99, 0.97)
        obs, ret = traj.obs.reshape(-1, N_OBS).cpu(), ret.reshape(-1).cpu().clone()
        infos = [learner.update(traj) for _ in range(30)]
        lv = [float(i["first"]["loss_v"]) for i in infos] + [float(infos[-1]["last"]["loss_v"])]
        ts = tensors(csz, parts(asz, csz, flat)[1], torch.float32, grad=True)
        opt = torch.optim.Adam(ts, lr=1e-3)
        tl = []
        for _ in range(30 * 4 + 1):
            loss = ((mlp(ts, obs)[:, 0] - ret) ** 2).mean()
            tl.append(float(loss.detach()))
            opt.zero_grad()
            loss.backward()
            opt.step()
        print(f"loss_v device {lv[0]:.4f} -> {lv[-1]:.4f}; torch {tl[0]:.4f} -> {tl[-2]:.4f}; first update's loss_pi "
              f"{float(infos[0]['first']['loss_pi']):.4f} -> {float(infos[0]['last']['loss_pi']):.4f}")
        assert np.isfinite(lv).all() and lv[-1] < lv[0] and tl[-2] < tl[0]
        assert abs(lv[0] - tl[0]) <= 1e-4 * tl[0]                       # the same start
        assert (lv[0] - lv[-1]) >= 0.9 * (tl[0] - tl[-2])               # and the torch model's fall, to 10 %
        # (loss_pi is not asked to fall within the first update: on these rows the torch model's own
        # rises over its first Adam steps -- a clipped row's r is free to run, and row 7's does)
        assert all(np.isfinite(float(i[w][k])) for i in infos for w in ("first", "last") for k in i[w])
    finally:
        learner.close()
        ac.close()


def test_argument_errors(gm, env):
    import torch
    from gmx.ppo import DevicePPOLearner
    from gmx._lib import PpoBatch
    net = "20-20"
    _, flat, batch, _ = crafted(net)
    ac = make_ac(env, net, flat)
    learner = DevicePPOLearner(ac)
    try:
        wrong = device_batch(batch, 17)
        wrong["act"] = torch.zeros((17, N_ACT), device="cuda")             # the Gaussian's width
        with pytest.raises(ValueError, match="act"):
            learner.grad_pi(wrong)
        missing = device_batch(batch, 17)
        del missing["adv"]
        with pytest.raises(KeyError):
            learner.grad_pi(missing)
        d = device_batch(batch, 17)
        b = PpoBatch()
        b.n, b.obs, b.logp, b.adv = 17, d["obs"].data_ptr(), d["logp"].data_ptr(), d["adv"].data_ptr()    # no act
        assert env.lib.gm_ppo_learner_grad_pi(learner._l, C.byref(b)) == -1
        assert b"incomplete batch" in env.lib.gm_last_error(env.ctx)
        with pytest.raises(ValueError, match="RMSprop"):
            DevicePPOLearner(ac, optimiser="rmsprop")
        from gmx.ppo import TrajectoryBuffer
        with pytest.raises(ValueError, match="act_dim"):                   # update checks the buffer's action width too
            learner.update(TrajectoryBuffer(env, 2))
        with pytest.raises(RuntimeError, match="n < 1"):
            learner.grad_pi(device_batch(batch, 0))
    finally:
        learner.close()
        ac.close()


def test_rollout_update_rollout(gm):
    """33 envs, 3 env-steps, 2-step episodes: rollout -> update -> rollout; the second rollout's
    per-step form still equals the fused one, with the weights the learner left on the device."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.ppo import DeviceCategoricalActorCritic, DevicePPOLearner, TrajectoryBuffer
    from test_ac_rollout import snapshot, assert_same
    from test_actor_critic_forward import torch_forward
    from test_cat_rollout import make_env, per_step, PSEED, DEC0
    n, k, mx = 33, 3, 2
    ra = torch.zeros((k, n, 3), dtype=torch.int32, device="cuda")
    rb = torch.zeros((k, n, 3), dtype=torch.int32, device="cuda")
    a, b = make_env(gm, n=n), make_env(gm, n=n)
    pa, pb = (DeviceCategoricalActorCritic(e, hidden=(20, 20), seed=3) for e in (a, b))
    la, lb = (DevicePPOLearner(p, train_pi_iters=3, train_vf_iters=3, learning_rate_pi=3e-3, **NO_STOP) for p in (pa, pb))
    ta, tb = TrajectoryBuffer(a, k, act_dim=1), TrajectoryBuffer(b, k, act_dim=1)
    try:
        before = pa.get_params()
        infos = []
        for p, l, t, r in ((pa, la, ta, ra), (pb, lb, tb, rb)):
            p.rollout(t, sample=True, seed=PSEED, decision0=DEC0, max_episode_steps=mx, records_dev_ptr=r.data_ptr())
            infos.append(l.update(t))
        assert infos[0]["pi_iters_done"] == infos[1]["pi_iters_done"] == 3
        for w in ("first", "last"):
            assert all(np.isfinite(v) for v in infos[0][w].values()), infos[0]
        assert 0 < float(infos[0]["first"]["ent"]) <= np.log(8) * (1 + 1e-6)
        after = pa.get_params()
        # every weight moved, but the first layers' from observation columns that are 0 in every row
        # (most of a 2-step episode's sensor history is)
        assert np.isfinite(after).all()
        moved = after != before
        pos = 0
        for sizes in (pa.actor_sizes, pa.critic_sizes):
            w0 = sizes[0] * sizes[1]
            assert moved[pos:pos + w0].mean() > 0.1 and moved[pos + w0:pos + w0 + sizes[1]].all()
            pos += w0
            rest = sum(sizes[i] * sizes[i + 1] + sizes[i + 1] for i in range(1, len(sizes) - 1)) + sizes[1]
            assert moved[pos:pos + rest].mean() > 0.9, (sizes, moved[pos:pos + rest].mean())
            pos += rest
        assert pos == after.size
        assert pa.get_packed().tobytes() == pb.get_packed().tobytes()       # two learners, the same bytes
        per_step(a, pa, ta, ra, 0, k, max_ep=mx)
        pa.finish(ta)
        pb.rollout(tb, sample=True, seed=PSEED, decision0=DEC0, max_episode_steps=mx, records_dev_ptr=rb.data_ptr())
        sa, sb = snapshot(a, ta, ra), snapshot(b, tb, rb)
        assert_same(gm, sa, sb)
        assert np.isfinite(sa["mu"]).all() and np.isfinite(sa["val"]).all() and np.isfinite(sa["logp"]).all()
        # the second rollout read the stepped weights: its first row's logits are the torch forward's of
        # the stepped parameters within the forward's bound, and not the initial parameters'
        class Nets:
            params, actor_sizes, critic_sizes = after, pa.actor_sizes, pa.critic_sizes
        x32, x64 = (torch_forward(Nets, sa["obs"][0], dt)[0] for dt in (torch.float32, torch.float64))
        bd = bound(x32, x64)
        assert float(np.abs(sa["mu"][0].astype(np.float64) - x64.numpy()).max()) <= bd
        Nets.params = before
        assert float(np.abs(sa["mu"][0].astype(np.float64) - torch_forward(Nets, sa["obs"][0], torch.float64)[0].numpy()).max()) > 8 * bd
    finally:
        la.close()
        lb.close()
        pa.close()
        pb.close()
        a.close()
        b.close()
