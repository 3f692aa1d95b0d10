"""The on-device PPO learner on the GPU (gm_ppo_learner_*, gm_ac_adv_normalise, gm_ac_get_params)
against torch autograd and torch.optim on the CPU, on crafted batches.  No env-stepping, except
the last test.

Tolerances are the project's measured convention (`bound` of tests/test_replay_sample_td.py):
every expected value is computed on the CPU in float32 and in float64, and the device must agree
with the float64 one within 8 x max|f32 - f64| + one f32 ulp of the largest magnitude, the maximum
taken per parameter tensor; for a scalar, over the crafted batch's per-row values (and the scalar).
As in that file the per-row maximum is taken over the whole crafted batch, of which the smaller
batches are prefixes: it estimates the f32 evaluation error for these parameters and inputs, which
one row cannot -- its |f32 - f64| may be 0, and the bound then shrinks to one ulp of a quantity
whose f32 evaluation error is several (n = 1, hidden (20, 20): loss_v = (v - ret)^2 misses its own
row's bound by a factor 1.18 while torch's f32 value happens to equal the f64 one to 1.3e-9).

Crafted data: obs uniform in [-1, 1]; "old" parameters and "new" ones = old + a perturbation;
act = mu_old + sigma_old z; logp_old from the old parameters in float64, rounded to f32; adv and ret
standard normal.  The clipped surrogate has kinks at r = 1 -+ eps, so the parameter seed is the
first below 64 (CPU, torch alone) for which every row's r is further from both edges than the bound
on r, and for which all five branches occur (r > 1 + eps with A > 0 and with A < 0, r < 1 - eps
with both, r inside).  No row is left out; tanh has no kink.  Adam's first steps are ~ lr sign(g)
where g ~ 0, so the optimisers are never compared end to end with autograd's gradients: the
device's own gradient is read back and fed to torch.optim.
Measured worst |device - f64| / bound: see DESIGN.md, "PPO learner"."""

import numpy as np
import pytest

from conftest import gpu_available
from test_replay_sample_td import bound
from test_dqn_learner import tensors, split

pytestmark = pytest.mark.gpu

N_ENVS, N_OBS, N_ACT = 16, 63, 4
EPS = 0.2
ROWS = 117                        # 8 tiles, the last one partial
NS = (1, 17, 37)                  # one row, one row into a second tile, a partial third tile
# the gradient kernels' three paths: rows and the workgroup's partial gradient in LDS (64-64, 20-20); the
# rows in LDS, the partial in global memory (128-128: its packed net does not fit behind the rows); neither (spill)
HIDDEN = {"64-64": (64, 64), "20-20": (20, 20), "128-128": (128, 128), "spill": (256, 256, 200)}
PERTURB = {"64-64": 0.02, "20-20": 0.04, "128-128": 0.02, "spill": 0.02}    # std of new - old: r lands on both sides of 1 -+ eps
MODES = {"clip": {}, "clip-entropy": dict(use_entropy_regularisation=True, entropy_coefficient=0.01),
         "kl": dict(use_kl_penalty=True), "kl-entropy": dict(use_kl_penalty=True, use_entropy_regularisation=True,
                                                             entropy_coefficient=0.01)}
NO_STOP = dict(target_kl=1e30)    # the KL stop never fires


def sizes_of(net):
    return [N_OBS, *HIDDEN[net], N_ACT], [N_OBS, *HIDDEN[net], 1]


def parts(asz, csz, flat):
    """(actor flat, critic flat, log_std) views of flat parameters."""
    na = sum(asz[i] * asz[i + 1] + asz[i + 1] for i in range(len(asz) - 1))
    nc = sum(csz[i] * csz[i + 1] + csz[i + 1] for i in range(len(csz) - 1))
    return flat[:na], flat[na:na + nc], flat[na + nc:]


def names(asz, csz):
    out = [f"pi.{'W' if i % 2 == 0 else 'b'}{i // 2}" for i in range(2 * (len(asz) - 1))]
    out += [f"vf.{'W' if i % 2 == 0 else 'b'}{i // 2}" for i in range(2 * (len(csz) - 1))]
    return out + ["log_std"]


def split_all(asz, csz, flat):
    a, c, ls = parts(asz, csz, flat)
    return split(asz, a) + split(csz, c) + [ls]


def mlp(ts, x):
    import torch
    for l in range(len(ts) // 2):
        x = torch.nn.functional.linear(x, ts[2 * l], ts[2 * l + 1])
        if l < len(ts) // 2 - 1:
            x = torch.tanh(x)
    return x


def craft(net, seed, rows=ROWS):
    """(new flat parameters, batch as f32 numpy) of the module docstring for one parameter seed."""
    import torch
    from gmx.ppo import init_params
    asz, csz = sizes_of(net)
    g = torch.Generator().manual_seed(1000 + seed)
    old = init_params(asz, csz, seed)
    new = (old.astype(np.float64) + PERTURB[net] * torch.randn(old.size, generator=g, dtype=torch.float64).numpy())
    obs = (torch.rand((rows, N_OBS), generator=g) * 2 - 1).numpy()
    a_old, _, ls_old = parts(asz, csz, old)
    with torch.no_grad():
        mu = mlp(tensors(asz, a_old, torch.float64), torch.from_numpy(obs).double())
        std = torch.exp(torch.from_numpy(ls_old).double())
        act = (mu + std * torch.randn((rows, N_ACT), generator=g, dtype=torch.float64)).float()
        logp = torch.distributions.Normal(mu, std).log_prob(act.double()).sum(-1).float()
    batch = dict(obs=obs, act=act.numpy(), logp=logp.numpy(), adv=torch.randn(rows, generator=g).numpy(),
                 ret=torch.randn(rows, generator=g).numpy())
    return new.astype(np.float32), batch


def loss_pi(asz, csz, flat, batch, n, dtype, opts, grad=True):
    """compute_loss_pi in torch on the CPU: dict of per-row and scalar values and the gradients."""
    import torch
    a, _, ls = parts(asz, csz, flat)
    ts = tensors(asz, a, dtype, grad=grad)
    log_std = torch.from_numpy(np.asarray(ls)).to(dtype).clone().requires_grad_(grad)
    obs, act, adv, lold = (torch.from_numpy(batch[k][:n]).to(dtype) for k in ("obs", "act", "adv", "logp"))
    pi = torch.distributions.Normal(mlp(ts, obs), torch.exp(log_std))
    logp = pi.log_prob(act).sum(-1)
    ratio = torch.exp(logp - lold)
    if opts.get("use_kl_penalty"):
        rows = -(ratio * adv) + opts.get("kl_penalty_coefficient", 0.2) * (lold - logp)
        loss = -(ratio * adv).mean() + opts.get("kl_penalty_coefficient", 0.2) * (lold - logp).mean()
    else:
        rows = -torch.min(ratio * adv, torch.clamp(ratio, 1 - EPS, 1 + EPS) * adv)
        loss = rows.mean()
    if opts.get("use_entropy_regularisation"):
        loss = loss - opts["entropy_coefficient"] * pi.entropy().mean()
    if grad:
        loss.backward()
    clipped = ratio.gt(1 + EPS) | ratio.lt(1 - EPS)
    return dict(loss=loss.detach(), rows=rows.detach(), r=ratio.detach(), kl_rows=(lold - logp).detach(),
                kl=(lold - logp).mean().detach(), ent_rows=pi.entropy().detach().reshape(-1),
                ent=pi.entropy().mean().detach(), clipped=int(clipped.sum()),
                grads=[t.grad for t in ts] + [log_std.grad] if grad else None)


def loss_v(asz, csz, flat, batch, n, dtype):
    import torch
    _, c, _ = parts(asz, csz, flat)
    ts = tensors(csz, c, dtype, grad=True)
    rows = (mlp(ts, torch.from_numpy(batch["obs"][:n]).to(dtype))[:, 0] - torch.from_numpy(batch["ret"][:n]).to(dtype)) ** 2
    loss = rows.mean()
    loss.backward()
    return dict(loss=loss.detach(), rows=rows.detach(), grads=[t.grad for t in ts])


def branches(r, adv):
    hi, lo = r > 1 + EPS, r < 1 - EPS
    return [int((hi & (adv > 0)).sum()), int((hi & (adv < 0)).sum()), int((lo & (adv > 0)).sum()),
            int((lo & (adv < 0)).sum()), int((~hi & ~lo).sum())]


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


@pytest.fixture(scope="module")
def env(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    from test_actor_critic_forward import make_env
    e = make_env(gm, n=N_ENVS)
    assert (e.n_obs, e.n_actions) == (N_OBS, N_ACT)
    yield e
    e.close()


def device_batch(batch, n, dev="cuda"):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v[:n])).to(dev) for k, v in batch.items()}


def make_ac(env, net, flat):
    from gmx.ppo import DeviceActorCritic
    asz, csz = sizes_of(net)
    return DeviceActorCritic(env, actor_sizes=asz, critic_sizes=csz, params=flat)


def check_scalar(tag, dev, x32, x64, rows32, rows64, worst, key):
    import torch
    b = bound(torch.cat([rows32.reshape(-1), x32.reshape(1)]), torch.cat([rows64.reshape(-1), x64.reshape(1)]))
    err = abs(float(dev) - float(x64))
    worst[key] = max(worst.get(key, 0.0), err / b)
    print(f"{tag} {key}: device {float(dev):.9g} f64 {float(x64):.9g} err {err:.3e} bound {b:.3e} ratio {err / b:.3f}")
    assert err <= b, f"{tag} {key}: {err:.3e} > {b:.3e}"


def check_grads(tag, asz, csz, g_dev, which, g32, g64, worst):
    """which: the indices (into names) of the tensors g32 / g64 list."""
    nm = names(asz, csz)
    dev = split_all(asz, csz, g_dev)
    for i, t32, t64 in zip(which, g32, g64):
        b = bound(t32.reshape(-1), t64.reshape(-1))
        err = float(np.abs(dev[i].astype(np.float64) - t64.reshape(-1).numpy()).max())
        worst[nm[i]] = max(worst.get(nm[i], 0.0), err / b)
        print(f"{tag} {nm[i]}: max |device - f64| {err:.3e} bound {b:.3e} ratio {err / b:.3f} "
              f"max |g| {float(t64.abs().max()):.3e}")
        assert err <= b, f"{tag} {nm[i]}: {err:.3e} > {b:.3e}"


def pi_indices(asz, csz):
    return list(range(2 * (len(asz) - 1))) + [2 * (len(asz) - 1) + 2 * (len(csz) - 1)]


def vf_indices(asz, csz):
    return list(range(2 * (len(asz) - 1), 2 * (len(asz) - 1) + 2 * (len(csz) - 1)))


def check_pi(tag, learner, net, flat, batch, n, opts, worst):
    import torch
    asz, csz = sizes_of(net)
    learner.grad_pi(device_batch(batch, n))
    g_dev, sc = learner.read()
    r32 = loss_pi(asz, csz, flat, batch, n, torch.float32, opts)
    r64 = loss_pi(asz, csz, flat, batch, n, torch.float64, opts)
    f32, f64 = (loss_pi(asz, csz, flat, batch, ROWS, dt, opts, grad=False) for dt in (torch.float32, torch.float64))
    check_scalar(tag, sc["loss_pi"], r32["loss"], r64["loss"], f32["rows"], f64["rows"], worst, "loss_pi")
    check_scalar(tag, sc["kl"], r32["kl"], r64["kl"], f32["kl_rows"], f64["kl_rows"], worst, "kl")
    check_scalar(tag, sc["ent"], r32["ent"], r64["ent"], f32["ent_rows"], f64["ent_rows"], worst, "ent")
    assert r32["clipped"] == r64["clipped"]
    assert sc["cf"] == np.float32(r64["clipped"]) / np.float32(n), (tag, sc["cf"], r64["clipped"], n)
    check_grads(tag, asz, csz, g_dev, pi_indices(asz, csz), r32["grads"], r64["grads"], worst)


def check_vf(tag, learner, net, flat, batch, n, worst):
    import torch
    asz, csz = sizes_of(net)
    learner.grad_vf(device_batch(batch, n))
    g_dev, sc = learner.read()
    r32, r64 = (loss_v(asz, csz, flat, batch, n, dt) for dt in (torch.float32, torch.float64))
    f32, f64 = (loss_v(asz, csz, flat, batch, ROWS, dt) for dt in (torch.float32, torch.float64))
    check_scalar(tag, sc["loss_v"], r32["loss"], r64["loss"], f32["rows"], f64["rows"], worst, "loss_v")
    check_grads(tag, asz, csz, g_dev, vf_indices(asz, csz), r32["grads"], r64["grads"], worst)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("net", sorted(HIDDEN))
def test_actor_gradients_match_autograd(gm, env, net, mode):
    from gmx.ppo import DevicePPOLearner
    seed, flat, batch, fig = crafted(net)
    ok, fig = clear_of_edges(net, flat, batch)
    assert ok, f"a row on a clip edge or a branch missing: {fig}"
    print(f"{net}: seed {seed}, nearest clip edge {fig[0]:.2e} vs bound on r {fig[1]:.2e}, rows per branch {fig[2]}")
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


@pytest.mark.parametrize("net", sorted(HIDDEN))
def test_critic_gradients_match_autograd(gm, env, net):
    from gmx.ppo import DevicePPOLearner
    _, flat, batch, _ = crafted(net)
    ac = make_ac(env, net, flat)
    learner, three = DevicePPOLearner(ac), DevicePPOLearner(ac, n_groups=3)
    worst = {}
    try:
        for n in NS:
            check_vf(f"{net} n {n}", learner, net, flat, batch, n, worst)
        check_vf(f"{net} n {ROWS} G 3", three, net, flat, batch, ROWS, worst)
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
    learners = {g: DevicePPOLearner(ac, n_groups=g) for g in (3, 5)}
    worst = {}
    try:
        data = device_batch(batch, ROWS)
        for g, l in learners.items():
            l.grad_pi(data)
            g1, s1 = l.read()
            l.grad_vf(data)                                  # another gradient in between
            l.grad_pi(device_batch(batch, 37))
            l.grad_pi(data)
            g2, s2 = l.read()
            pi = [k for k in s1 if k != "loss_v"]
            a, c, ls = parts(*sizes_of(net), g1)
            a2, c2, ls2 = parts(*sizes_of(net), g2)
            assert a.tobytes() == a2.tobytes() and ls.tobytes() == ls2.tobytes()
            assert all(s1[k].tobytes() == s2[k].tobytes() for k in pi)
            assert np.abs(c).max() == 0 and np.abs(c2).max() > 0 and np.abs(a).max() > 0     # vf's gradient is held too
            check_pi(f"{net} G {g}", l, net, flat, batch, ROWS, {}, worst)
            check_vf(f"{net} G {g}", l, net, flat, batch, ROWS, worst)
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
    _, coff, lsoff = pack(asz, csz, flat)
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
            a, c, ls = parts(asz, csz, flat)
            ts = tensors(asz, a, dt, grad=True) + tensors(csz, c, dt, grad=True) + \
                [torch.from_numpy(ls.copy()).to(dt).requires_grad_(True)]
            ref[dt] = (ts, {w: cls([ts[i] for i in idx[w]], lr=lrs[w], betas=(0.9, 0.999), **kw) for w in ("pi", "vf")})
        for step in range(1, 6):
            for w in ("pi", "vf"):
                other = "vf" if w == "pi" else "pi"
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
                # the other optimiser's part of the blob keeps its bytes
                lo, hi = (coff, lsoff) if w == "pi" else (0, coff)
                assert packed_before[lo:hi].tobytes() == packed_after[lo:hi].tobytes(), f"{w} stepped {other}'s weights"
                if w == "vf":
                    assert packed_before[lsoff:].tobytes() == packed_after[lsoff:].tobytes(), "vf stepped log_std"
                assert packed_before.tobytes() != packed_after.tobytes()
            print(f"{optimiser} step {step}: worst |device - f64| / bound so far {worst:.3f}")
        # the state round trip: a second learner on a copy of the weights takes the same next steps
        copy = make_ac(env, net, ac.get_params())
        clone = DevicePPOLearner(copy, optimiser=optimiser, grad_clamp_value=clamp)
        state = learner.state()
        assert state["step_pi"] == 5 and state["step_vf"] == 5 and np.abs(state["exp_avg"]).max() > 0
        clone.load_state(state)
        for l in (learner, clone):
            l.grad_pi(data)
            l.step_pi()
            l.grad_vf(data)
            l.step_vf()
        assert ac.get_packed().tobytes() == copy.get_packed().tobytes()
        s1, s2 = learner.state(), clone.state()
        assert s1["step_pi"] == s2["step_pi"] == 6 and s1["step_vf"] == s2["step_vf"] == 6
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


def fill_traj(env, net):
    """A TrajectoryBuffer holding 128 crafted rows (end cycling 0 / 0 / 1 / 0 / 2), and the new parameters."""
    import torch
    from gmx.ppo import TrajectoryBuffer
    seed, _, _, _ = crafted(net)
    flat, batch = craft(net, seed, rows=K_TRAJ * N_ENVS)
    g = torch.Generator().manual_seed(77)
    traj = TrajectoryBuffer(env, K_TRAJ)
    traj.obs.copy_(torch.from_numpy(batch["obs"]).reshape(K_TRAJ, N_ENVS, N_OBS))
    traj.act.copy_(torch.from_numpy(batch["act"]).reshape(K_TRAJ, N_ENVS, N_ACT))
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
    data = dict(obs=traj.obs.reshape(-1, N_OBS), act=traj.act.reshape(-1, N_ACT), logp=traj.logp.reshape(-1),
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


def same_learner_bytes(a, b, la, lb):
    assert a.get_packed().tobytes() == b.get_packed().tobytes()
    s1, s2 = la.state(), lb.state()
    assert (s1["step_pi"], s1["step_vf"]) == (s2["step_pi"], s2["step_vf"])
    for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        assert s1[k].tobytes() == s2[k].tobytes(), k
    assert la.read()[0].tobytes() == lb.read()[0].tobytes()
    assert all(la.read()[1][k].tobytes() == lb.read()[1][k].tobytes() for k in la.read()[1])


def same_info(info, first, last):
    for k in first:
        assert info["first"][k].tobytes() == np.float32(first[k]).tobytes(), ("first", k)
        assert info["last"][k].tobytes() == np.float32(last[k]).tobytes(), ("last", k)


ITERS = 6
UPD = dict(train_pi_iters=ITERS, train_vf_iters=ITERS, learning_rate_pi=3e-3, grad_clamp_value=0.05)


@pytest.mark.parametrize("optimiser", ["adam", "adamW"])
def test_update_equals_the_calls_it_enqueues(gm, env, optimiser):
    from gmx.ppo import DevicePPOLearner
    net = "64-64"
    traj, flat = fill_traj(env, net)
    opts = dict(UPD, optimiser=optimiser, **NO_STOP)
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
    _, coff, lsoff = pack(asz, csz, flat)
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
        rising = [j for j in range(1, ITERS - 1) if kls[j] < kls[j + 1] and max(kls[:j + 1]) < 0.5 * (kls[j] + kls[j + 1])]
        assert rising, f"no pair of consecutive iterations with kl_j < kl_j+1 above every earlier kl: {kls}"
        j = rising[0]
        thr = 0.5 * (kls[j] + kls[j + 1])
        assert sum(k <= thr for k in kls[:j + 2]) == j + 1
        stop = dict(UPD, target_kl=thr, max_kl_ratio=1.0)
        assert np.float64(stop["target_kl"]) * stop["max_kl_ratio"] == thr

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
        assert pa[:coff].tobytes() != pref[:coff].tobytes()             # fewer policy steps than the free run
        assert pa[coff:lsoff].tobytes() == pref[coff:lsoff].tobytes()   # the critic: all its iterations, the same bytes

        # a second update continues Adam's bias correction from the right step
        info2 = la.update(traj)
        _, steps2, first2, last2 = by_calls(env, lb, traj, stop, ITERS, stop_at=thr)
        assert info2["pi_iters_done"] == steps2 and la.state()["step_pi"] == j + 1 + steps2
        assert la.state()["step_vf"] == 2 * ITERS
        same_learner_bytes(a, b, la, lb)
        same_info(info2, first2, last2)

        # a threshold below kl_0: no policy step at all, the critic trained
        c, lc = pair(dict(UPD, target_kl=kls[0] - abs(kls[0]) * 0.5 - 1e-6, max_kl_ratio=1.0))
        info3 = lc.update(traj)
        pc, p0 = c.get_packed(), pack(asz, csz, flat)[0]
        assert info3["pi_iters_done"] == 0 and lc.state()["step_pi"] == 0 and lc.state()["step_vf"] == ITERS
        assert pc[:coff].tobytes() == p0[:coff].tobytes() and pc[lsoff:].tobytes() == p0[lsoff:].tobytes()
        assert pc[coff:lsoff].tobytes() == pref[coff:lsoff].tobytes()
        assert info3["first"]["kl"].tobytes() == info3["last"]["kl"].tobytes() == np.float32(kls[0]).tobytes()
    finally:
        for l in learners:
            l.close()
        for ac in acs:
            ac.close()


@pytest.mark.parametrize("net", ["64-64", "20-20"])
def test_padding_stays_zero_under_training(gm, env, net):
    from gmx.ppo import DevicePPOLearner, pack
    asz, csz = sizes_of(net)
    traj, flat = fill_traj(env, net)
    ac = make_ac(env, net, flat)
    learner = DevicePPOLearner(ac, optimiser="adamW", train_pi_iters=2, train_vf_iters=2, learning_rate_pi=1e-3,
                               **NO_STOP)         # AdamW: weight decay and amsgrad
    try:
        pad = pack(asz, csz, np.ones(flat.size, dtype=np.float32))[0] == 0
        assert pad.any()
        before = ac.get_packed()
        assert (before[pad] == 0.0).all()
        for _ in range(20):
            learner.update(traj)
        packed = ac.get_packed()
        assert (packed[pad] == 0.0).all(), f"{int((packed[pad] != 0).sum())} padding entries moved"
        assert (packed[~pad] != before[~pad]).mean() > 0.9            # and the weights did move
    finally:
        learner.close()
        ac.close()


@pytest.mark.parametrize("n", [2, 37, 4099])
def test_adv_normalise(gm, env, n):
    import torch
    from gmx.ppo import adv_normalise
    x = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3 + 1.5)
    dev = adv_normalise(env, x.to("cuda")).cpu().numpy()
    again = adv_normalise(env, x.to("cuda")).cpu().numpy()
    assert dev.tobytes() == again.tobytes()
    x64 = x.numpy().astype(np.float64)
    want = (x64 - x64.mean()) / x64.std(ddof=1)
    std32, mean32 = torch.std_mean(x)                                  # PPOBuffer.get's own f32 evaluation
    b = bound((x - mean32) / std32, torch.from_numpy(want))
    err = float(np.abs(dev.astype(np.float64) - want).max())
    print(f"n {n}: max |device - f64| {err:.3e} bound {b:.3e} ratio {err / b:.3f}")
    assert err <= b


def test_adv_normalise_needs_two_values(gm, env):
    import torch
    from gmx.ppo import adv_normalise
    with pytest.raises(RuntimeError, match="standard deviation"):
        adv_normalise(env, torch.ones(1, device="cuda"))


def test_rollout_reads_the_updated_weights(gm, env):
    import torch
    from gmx.ppo import DevicePPOLearner, TrajectoryBuffer
    from test_actor_critic_forward import torch_forward
    net = "64-64"
    traj, flat = fill_traj(env, net)
    ac = make_ac(env, net, flat)
    learner = DevicePPOLearner(ac, **dict(UPD, **NO_STOP))
    other = None
    try:
        learner.update(traj)
        trained = ac.get_params()
        assert ac.params.tobytes() == flat.tobytes() and trained.tobytes() != flat.tobytes()
        one = TrajectoryBuffer(env, 1)
        ac.act(one, 0, sample=False)
        torch.cuda.synchronize()
        obs = env.observation()

        class Nets:                         # torch_forward reads params, actor_sizes, critic_sizes
            params, actor_sizes, critic_sizes = trained, ac.actor_sizes, ac.critic_sizes
        ref = {dt: torch_forward(Nets, obs, dt) for dt in (torch.float32, torch.float64)}
        for q, dev in ((0, one.mu[0].cpu().numpy()), (1, one.val[0].cpu().numpy())):
            b = bound(ref[torch.float32][q], ref[torch.float64][q])
            err = float(np.abs(dev.astype(np.float64) - ref[torch.float64][q].numpy()).max())
            assert err <= b, f"{'mu' if q == 0 else 'val'}: |device - f64| {err:.3e} > bound {b:.3e}"
        # state_dict, in MLPActorCriticPG's key names, round-trips through set_params
        sd = ac.state_dict()
        assert set(sd) == {"pi.log_std"} | {f"{p}{2 * l}.{w}" for p in ("pi.mu_net.", "vf.v_net.") for l in range(3)
                                            for w in ("weight", "bias")}
        assert sd["pi.mu_net.0.weight"].shape == (64, N_OBS) and sd["vf.v_net.4.weight"].shape == (1, 64)
        other = make_ac(env, net, flat)
        other.set_params(sd)
        assert other.get_params().tobytes() == trained.tobytes()
        assert other.get_packed().tobytes() == ac.get_packed().tobytes()
    finally:
        learner.close()
        ac.close()
        if other is not None:
            other.close()


def test_it_learns(gm, env):
    from gmx.ppo import DevicePPOLearner
    net = "64-64"
    traj, flat = fill_traj(env, net)
    ac = make_ac(env, net, flat)
    learner = DevicePPOLearner(ac, train_pi_iters=4, train_vf_iters=4, **NO_STOP)
    try:
        infos = [learner.update(traj) for _ in range(30)]
        lv = [float(i["first"]["loss_v"]) for i in infos] + [float(infos[-1]["last"]["loss_v"])]
        print(f"loss_v {lv[0]:.4f} -> {lv[-1]:.4f}; first update's loss_pi {float(infos[0]['first']['loss_pi']):.4f} -> "
              f"{float(infos[0]['last']['loss_pi']):.4f}")
        assert np.isfinite(lv).all() and lv[-1] < lv[0]
        assert float(infos[0]["first"]["loss_pi"]) > float(infos[0]["last"]["loss_pi"])
    finally:
        learner.close()
        ac.close()


def test_argument_errors(gm, env):
    import torch
    from gmx.ppo import DevicePPOLearner
    net = "20-20"
    _, flat, batch, _ = crafted(net)
    ac = make_ac(env, net, flat)
    learner = DevicePPOLearner(ac)
    try:
        with pytest.raises(RuntimeError, match="n < 1"):
            learner.grad_pi(device_batch(batch, 0))
        with pytest.raises(RuntimeError, match="n < 1"):
            learner.grad_vf(device_batch(batch, 0))
        with pytest.raises(ValueError, match="RMSprop"):
            DevicePPOLearner(ac, optimiser="rmsprop")
        with pytest.raises(ValueError, match="incorrect key"):
            DevicePPOLearner(ac, learning_rate=1e-3)
        wrong = device_batch(batch, 17)
        wrong["act"] = torch.zeros((17, N_ACT + 1), device="cuda")
        with pytest.raises(ValueError, match="act"):
            learner.grad_pi(wrong)
        wrong = device_batch(batch, 17)
        wrong["obs"] = wrong["obs"][:, :N_OBS - 1].contiguous()
        with pytest.raises(ValueError, match="obs"):
            learner.grad_vf(wrong)
        wrong = device_batch(batch, 17)
        wrong["ret"] = wrong["ret"][:16]
        with pytest.raises(ValueError, match="ret"):
            learner.grad_vf(wrong)
        learner.close()
        for call in (lambda: learner.grad_pi(device_batch(batch, 17)), learner.step_pi, learner.step_vf, learner.read,
                     learner.state):
            with pytest.raises(RuntimeError, match="closed"):
                call()
    finally:
        learner.close()
        ac.close()


def test_rollout_update_rollout(gm):
    """At the smallest env shape tests/test_ac_rollout.py uses (33 envs, 3 env-steps, 2-step
    episodes): rollout -> update -> rollout; the second rollout's per-step form still equals the
    fused one (that file's helpers), with the weights the learner left on the device."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.ppo import DeviceActorCritic, DevicePPOLearner, TrajectoryBuffer
    from test_ac_rollout import make_env, per_step, snapshot, assert_same, NOISE, PSEED, DEC0
    n, k, mx = 33, 3, 2
    ra = torch.zeros((k, n, 3), dtype=torch.int32, device="cuda")
    rb = torch.zeros((k, n, 3), dtype=torch.int32, device="cuda")
    a, b = make_env(gm, n=n), make_env(gm, n=n)
    pa, pb = DeviceActorCritic(a, seed=3), DeviceActorCritic(b, seed=3)
    la, lb = (DevicePPOLearner(p, train_pi_iters=3, train_vf_iters=3, **NO_STOP) for p in (pa, pb))
    ta, tb = TrajectoryBuffer(a, k), TrajectoryBuffer(b, k)
    try:
        before = pa.get_params()
        infos = []
        for p, l, t, r in ((pa, la, ta, ra), (pb, lb, tb, rb)):
            p.rollout(t, sample=True, noise=NOISE, seed=PSEED, decision0=DEC0, max_episode_steps=mx,
                      records_dev_ptr=r.data_ptr())
            infos.append(l.update(t))
        assert infos[0]["pi_iters_done"] == infos[1]["pi_iters_done"] == 3
        for w in ("first", "last"):
            assert all(np.isfinite(v) for v in infos[0][w].values()), infos[0]
        after = pa.get_params()
        assert np.isfinite(after).all() and (after != before).mean() > 0.5     # (weights of constant-0 observations keep still)
        assert pa.get_packed().tobytes() == pb.get_packed().tobytes()       # two learners, the same bytes
        per_step(a, pa, ta, ra, 0, k, max_ep=mx)
        pa.finish(ta)
        pb.rollout(tb, sample=True, noise=NOISE, seed=PSEED, decision0=DEC0, max_episode_steps=mx,
                   records_dev_ptr=rb.data_ptr())
        sa, sb = snapshot(a, ta, ra), snapshot(b, tb, rb)
        assert_same(gm, sa, sb)
        assert np.isfinite(sa["mu"]).all() and np.isfinite(sa["val"]).all() and np.isfinite(sa["logp"]).all()
    finally:
        la.close()
        lb.close()
        pa.close()
        pb.close()
        a.close()
        b.close()
