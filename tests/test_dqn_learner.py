"""The on-device DQN learner on the GPU (gm_learner_*, gm_policy_get_params, gm_policy_soft_update)
against torch autograd and torch.optim on the CPU, on the crafted replay memory of
tests/test_replay_sample_td.py (its fixtures and helpers are imported, not copied).  No env-stepping.

Tolerances are that file's measured convention: every expected value is computed on the CPU in
float32 and in float64, and the device must agree with the float64 one within
8 x max|f32 - f64| + one f32 ulp of the largest magnitude (`bound`), the maximum taken per
parameter tensor.  For the scalar loss the maximum is taken over the batch's per-row losses (and the
mean): the mean inherits every row's evaluation error, and one scalar's |f32 - f64| may be 0.

Autograd's gradient has kinks -- where a hidden pre-activation changes sign between f32 and f64 and
where |q_a - y| crosses 1 (smooth-L1) -- so the parameter seed is the first below 64 (CPU, torch
alone) whose float64 values keep clear of both in EVERY row: each hidden pre-activation further
from 0 than 8 x max|pre32 - pre64|, each |q_a - y| further from 1 than the bound on q_a.  No row is
left out.  Adam's first steps are ~ lr sign(g) where g ~ 0, so the optimiser is never compared end
to end with autograd's gradients: the device's own gradient is read back and fed to torch.optim.
Measured worst |device - f64| / bound: see DESIGN.md, "DQN learner"."""
import numpy as np
import pytest

from test_replay_sample_td import CAP, GAMMA, NETS, bound, env, memory  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NS = (1, 17, 37, 128)            # one row, one row into a second tile, a partial tile, 8 full tiles
# the rows of a net this deep and wide do not fit the gradient kernel's LDS: its global spill path
SPILL_NET = [63, 256, 256, 200, 8]


def tensors(sizes, flat, dtype, grad=False):
    """[W0, b0, W1, b1, ...] of the flat parameters as torch tensors."""
    import torch
    p = torch.from_numpy(np.asarray(flat)).to(dtype)
    out, pos = [], 0
    for l in range(len(sizes) - 1):
        fin, fout = sizes[l], sizes[l + 1]
        out.append(p[pos:pos + fout * fin].reshape(fout, fin).clone().requires_grad_(grad))
        pos += fout * fin
        out.append(p[pos:pos + fout].clone().requires_grad_(grad))
        pos += fout
    return out


def split(sizes, flat):
    """Views of a flat numpy array per parameter tensor."""
    out, pos = [], 0
    for l in range(len(sizes) - 1):
        for cnt in (sizes[l] * sizes[l + 1], sizes[l + 1]):
            out.append(flat[pos:pos + cnt])
            pos += cnt
    return out


def forward(ts, x, dtype):
    """(hidden pre-activations, softmax outputs) of VariableNetwork.forward."""
    import torch
    h = torch.from_numpy(x).to(dtype)
    pre = []
    for l in range(len(ts) // 2):
        h = torch.nn.functional.linear(h, ts[2 * l], ts[2 * l + 1])
        if l < len(ts) // 2 - 1:
            pre.append(h)
            h = torch.relu(h)
    return pre, torch.softmax(h, dim=1)


def row_losses(q_a, y, loss):
    import torch
    fn = torch.nn.functional.mse_loss if loss == "MSELoss" else torch.nn.functional.smooth_l1_loss
    return fn(q_a, y, reduction="none")


def autograd(sizes, flat, x, a, y, loss, dtype):
    """(per-row losses, mean loss, [dL/dW0, dL/db0, ...]) with torch autograd on the CPU."""
    import torch
    ts = tensors(sizes, flat, dtype, grad=True)
    _, q = forward(ts, x, dtype)
    q_a = q.gather(1, torch.from_numpy(a).long()[:, None])[:, 0]
    rows = row_losses(q_a, torch.from_numpy(y).to(dtype), loss)
    mean = rows.mean()
    mean.backward()
    return rows.detach(), mean.detach(), [t.grad for t in ts]


def clear_of_kinks(sizes, flat, x, a, y):
    """Every hidden pre-activation and every |q_a - y| of every row beyond its bound from the kink."""
    import torch
    with torch.no_grad():
        pre32, q32 = forward(tensors(sizes, flat, torch.float32), x, torch.float32)
        pre64, q64 = forward(tensors(sizes, flat, torch.float64), x, torch.float64)
        diff = max(float((p32.double() - p64).abs().max()) for p32, p64 in zip(pre32, pre64))
        near0 = min(float(p64.abs().min()) for p64 in pre64)
        idx = torch.from_numpy(a).long()[:, None]
        qa32, qa64 = q32.gather(1, idx)[:, 0], q64.gather(1, idx)[:, 0]
        kink = float(((qa64 - torch.from_numpy(y).double()).abs() - 1.0).abs().min())
    return near0 > 8.0 * diff and kink > bound(qa32, qa64), (near0, diff, kink)


def choose_seed(sizes, x, a, y_of_seed):
    from gmx.policy import init_params
    for seed in range(64):
        ok, figures = clear_of_kinks(sizes, init_params(sizes, seed), x, a, y_of_seed(seed))
        if ok:
            return seed, figures
    raise AssertionError("no parameter seed below 64 keeps every row clear of autograd's kinks")


def first_rows(buf, n):
    """The first n rows of the crafted memory as a batch (device views)."""
    return {k: getattr(buf, k)[:n] for k in ("state", "action", "next_state", "reward", "end")}


def cpu_td_target(sizes, tflat, nxt, rew):
    import torch
    with torch.no_grad():
        _, q = forward(tensors(sizes, tflat, torch.float32), nxt, torch.float32)
        return (q.max(1)[0] * GAMMA + torch.from_numpy(rew)).numpy()


@pytest.mark.parametrize("ysrc", ["crafted", "td_target"])
@pytest.mark.parametrize("loss", ["smoothL1Loss", "MSELoss"])
@pytest.mark.parametrize("net", sorted(NETS) + ["spill"])
def test_gradients_match_autograd(gm, env, memory, net, loss, ysrc):
    import torch
    from gmx.policy import DevicePolicy, DeviceLearner, init_params
    sizes = NETS.get(net, SPILL_NET)
    buf, rows = memory
    buf.pushed = CAP
    x, a, nxt, rew = (rows[k][:128] for k in ("state", "action", "next_state", "reward"))
    if ysrc == "crafted":
        seed, fig = choose_seed(sizes, x, a, lambda s: (rew + np.float32(0.99 * 0.3)).astype(np.float32))
    else:   # the search sees the CPU's TD target; the device's own is rechecked below
        seed, fig = choose_seed(sizes, x, a, lambda s: cpu_td_target(sizes, init_params(sizes, s + 100), nxt, rew))
    print(f"{net} {loss} {ysrc}: seed {seed}, min |pre| {fig[0]:.2e} vs 8 x {fig[1]:.2e}, kink distance {fig[2]:.2e}")
    online = DevicePolicy(env, sizes=sizes, seed=seed)
    target = DevicePolicy(env, sizes=sizes, seed=seed + 100)
    learner = DeviceLearner(online, target, loss_criterion=loss)
    worst = {}
    try:
        full = first_rows(buf, 128)
        if ysrc == "crafted":
            y_dev = (full["reward"] + np.float32(0.99 * 0.3)).contiguous()
        else:
            y_dev, _ = online.td_target(full, GAMMA, target=target)
        y = y_dev.cpu().numpy()
        ok, fig = clear_of_kinks(sizes, online.params, x, a, y)
        assert ok, f"the device's y moves a row onto a kink: {fig}"
        quad = float((np.abs(forward(tensors(sizes, online.params, torch.float64), x, torch.float64)[1]
                             .gather(1, torch.from_numpy(a).long()[:, None])[:, 0].numpy() - y) < 1).mean())
        assert loss != "smoothL1Loss" or 0.05 < quad < 0.95, f"one smooth-L1 branch only ({quad:.2f} quadratic)"
        for n in NS:
            learner.grad(first_rows(buf, n), y_dev[:n].contiguous())
            g_dev, loss_dev = learner.read()
            r32, m32, g32 = autograd(sizes, online.params, x[:n], a[:n], y[:n], loss, torch.float32)
            r64, m64, g64 = autograd(sizes, online.params, x[:n], a[:n], y[:n], loss, torch.float64)
            b = bound(torch.cat([r32, m32[None]]), torch.cat([r64, m64[None]]))
            err = abs(loss_dev - float(m64))
            worst["loss"] = max(worst.get("loss", 0.0), err / b)
            print(f"{net} {loss} {ysrc} n {n} loss: device {loss_dev:.9g} f64 {float(m64):.9g} err {err:.3e} "
                  f"bound {b:.3e} ratio {err / b:.3f}")
            assert err <= b, f"n {n} loss: {err:.3e} > {b:.3e}"
            for i, (gd, t32, t64) in enumerate(zip(split(sizes, g_dev), g32, g64)):
                name = f"{'W' if i % 2 == 0 else 'b'}{i // 2}"
                b = bound(t32.reshape(-1), t64.reshape(-1))
                err = float(np.abs(gd.astype(np.float64) - t64.reshape(-1).numpy()).max())
                worst[name] = max(worst.get(name, 0.0), err / b)
                print(f"{net} {loss} {ysrc} n {n} {name}: max |device - f64| {err:.3e} bound {b:.3e} "
                      f"ratio {err / b:.3f} max |g| {float(t64.abs().max()):.3e}")
                assert err <= b, f"n {n} {name}: {err:.3e} > {b:.3e}"
        print(f"{net} {loss} {ysrc}: worst |device - f64| / bound {worst}")
    finally:
        learner.close()
        online.close()
        target.close()


@pytest.mark.parametrize("net", sorted(NETS) + ["spill"])
def test_grad_is_deterministic(gm, env, memory, net):
    from gmx.policy import DevicePolicy, DeviceLearner
    sizes = NETS.get(net, SPILL_NET)
    buf, _ = memory
    buf.pushed = CAP
    online = DevicePolicy(env, sizes=sizes, seed=5)
    learner = DeviceLearner(online)
    try:
        batch = first_rows(buf, 128)
        y = (batch["reward"] * 0.5).contiguous()
        learner.grad(batch, y)
        g1, l1 = learner.read()
        learner.grad(first_rows(buf, 37), y[:37].contiguous())        # another gradient in between
        learner.grad(batch, y)
        g2, l2 = learner.read()
        assert g1.tobytes() == g2.tobytes() and np.float32(l1).tobytes() == np.float32(l2).tobytes()
        assert np.abs(g1).max() > 0
    finally:
        learner.close()
        online.close()


@pytest.mark.parametrize("net", sorted(NETS))
def test_get_params_inverts_set_params(gm, env, net):
    from gmx.policy import DevicePolicy, init_params, pack
    sizes = NETS[net]
    p = DevicePolicy(env, sizes=sizes, seed=1)
    try:
        assert p.get_params().tobytes() == init_params(sizes, 1).tobytes()
        new = init_params(sizes, seed=2)
        p.set_params(new)
        assert p.get_params().tobytes() == new.tobytes()
        assert p.get_packed().tobytes() == pack(sizes, new).tobytes()
    finally:
        p.close()


@pytest.mark.parametrize("net", sorted(NETS))
def test_padding_stays_zero_under_training(gm, env, memory, net):
    from gmx.policy import DevicePolicy, DeviceLearner, pack
    sizes = NETS[net]
    buf, _ = memory
    buf.pushed = CAP
    online = DevicePolicy(env, sizes=sizes, seed=3)
    target = DevicePolicy(env, sizes=sizes, seed=4)
    learner = DeviceLearner(online, target, learning_rate=1e-3)     # AdamW with decay, amsgrad, soft updates
    try:
        pad = pack(sizes, np.ones(online.params.size, dtype=np.float32)) == 0
        assert pad.any()
        before = online.get_packed()
        learner.train(buf, 20, batch_size=37, seed=2, draw0=0)
        for name, pol in (("online", online), ("target", target)):
            packed = pol.get_packed()
            assert (packed[pad] == 0.0).all(), f"{name}: {int((packed[pad] != 0).sum())} padding entries moved"
        assert (online.get_packed()[~pad] != before[~pad]).mean() > 0.9       # and the weights did move
    finally:
        learner.close()
        online.close()
        target.close()


STEP_CASES = {"adam": dict(optimiser="adam", amsgrad=False, weight_decay=0.0),
              "adam-amsgrad-decay": dict(optimiser="adam", amsgrad=True, weight_decay=0.01),
              "adamw": dict(optimiser="adamW", amsgrad=False, weight_decay=0.0),
              "adamw-amsgrad-decay": dict(optimiser="adamW", amsgrad=True, weight_decay=0.01)}


@pytest.mark.parametrize("case", sorted(STEP_CASES))
def test_optimiser_steps_match_torch_elementwise(gm, env, memory, case):
    import torch
    from gmx.policy import DevicePolicy, DeviceLearner
    sizes = NETS["canonical"]
    opts = STEP_CASES[case]
    buf, _ = memory
    buf.pushed = CAP
    online = DevicePolicy(env, sizes=sizes, seed=0)
    probe = DeviceLearner(online)
    learner = clone = None
    worst = 0.0
    try:
        batch = first_rows(buf, 128)
        y = (batch["reward"] + np.float32(0.99 * 0.3)).contiguous()
        probe.grad(batch, y)
        g0 = np.abs(probe.read()[0])
        clamp = float(np.median(g0[g0 > 0]))                # both sides of the clamp occur
        assert clamp > 0 and (g0 > clamp).any() and ((g0 < clamp) & (g0 > 0)).any()
        learner = DeviceLearner(online, grad_clamp_value=clamp, **opts)
        cls = torch.optim.AdamW if opts["optimiser"] == "adamW" else torch.optim.Adam
        ref = {}
        for dt in (torch.float32, torch.float64):
            ts = tensors(sizes, online.params, dt, grad=True)
            ref[dt] = (ts, cls(ts, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=opts["weight_decay"],
                               amsgrad=opts["amsgrad"]))
        for step in range(1, 6):
            learner.grad(batch, y)
            g = torch.clamp(torch.from_numpy(learner.read()[0]), -clamp, clamp)     # the device's own gradient
            learner.step()
            p_dev = split(sizes, online.get_params())
            for dt, (ts, opt) in ref.items():
                for t, gt in zip(ts, split(sizes, g)):
                    t.grad = gt.reshape(t.shape).to(dt)
                opt.step()
            for i, (pd, t32, t64) in enumerate(zip(p_dev, *(ref[dt][0] for dt in (torch.float32, torch.float64)))):
                b = bound(t32.detach().reshape(-1), t64.detach().reshape(-1))
                err = float(np.abs(pd.astype(np.float64) - t64.detach().reshape(-1).numpy()).max())
                worst = max(worst, err / b)
                assert err <= b, f"{case} step {step} tensor {i}: {err:.3e} > {b:.3e}"
            print(f"{case} step {step}: worst |device - f64| / bound so far {worst:.3f}")
        # the state round trip: a second learner on a copy of the weights takes the same next step
        copy = DevicePolicy(env, sizes=sizes, params=online.get_params())
        clone = DeviceLearner(copy, grad_clamp_value=clamp, **opts)
        state = learner.state()
        assert state["step"] == 5 and np.abs(state["exp_avg"]).max() > 0
        clone.load_state(state)
        for l in (learner, clone):
            l.grad(batch, y)
            l.step()
        assert online.get_params().tobytes() == copy.get_params().tobytes()
        s1, s2 = learner.state(), clone.state()
        assert s1["step"] == s2["step"] == 6
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert s1[k].tobytes() == s2[k].tobytes(), k
        copy.close()
    finally:
        for l in (probe, learner, clone):
            if l is not None:
                l.close()
        online.close()


@pytest.mark.parametrize("tau", [0.05, 1.0])
@pytest.mark.parametrize("net", sorted(NETS))
def test_soft_update(gm, env, net, tau):
    from gmx.policy import DevicePolicy
    sizes = NETS[net]
    online = DevicePolicy(env, sizes=sizes, seed=6)
    target = DevicePolicy(env, sizes=sizes, seed=7)
    try:
        p, t = online.get_params(), target.get_params()
        target.soft_update(online, tau)
        got = target.get_params()
        tau64 = float(np.float32(tau))                               # the value the C ABI's float carries
        want = p.astype(np.float64) * tau64 + t.astype(np.float64) * (1.0 - tau64)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        worst = float((np.abs(got.astype(np.float64) - want) / ulp).max())
        print(f"{net} tau {tau}: worst error {worst:.3f} ulp")
        assert worst <= 2.0
        if tau == 1.0:
            assert got.tobytes() == p.tobytes()
        assert online.get_params().tobytes() == p.tobytes()          # the online net is only read
    finally:
        online.close()
        target.close()


@pytest.mark.parametrize("pushed", [200, 3 * CAP + 17])             # size < capacity; a wrapped ring
@pytest.mark.parametrize("double", [False, True])
def test_train_equals_the_calls_it_enqueues(gm, env, memory, double, pushed):
    from gmx.policy import DevicePolicy, DeviceLearner
    sizes = NETS["canonical"]
    buf, _ = memory
    buf.pushed = pushed
    assert len(buf) == min(pushed, CAP)
    nets = [DevicePolicy(env, sizes=sizes, seed=s) for s in (8, 9, 8, 9)]          # online, target, twice
    kw = dict(use_double_dqn=double, soft_target_tau=0.05, gamma=GAMMA, learning_rate=1e-3)
    fused, calls = DeviceLearner(nets[0], nets[1], **kw), DeviceLearner(nets[2], nets[3], **kw)
    try:
        losses = fused.train(buf, 3, batch_size=37, seed=12, draw0=40).cpu().numpy()
        by_call = []
        for u in range(3):
            batch = buf.sample(37, seed=12, draw=40 + u)
            y, _ = nets[2].td_target(batch, GAMMA, target=nets[3], double=double)
            calls.grad(batch, y)
            by_call.append(calls.read()[1])
            calls.step()
            nets[3].soft_update(nets[2], 0.05)
        assert losses.tobytes() == np.asarray(by_call, dtype=np.float32).tobytes()
        assert nets[0].get_packed().tobytes() == nets[2].get_packed().tobytes()
        assert nets[1].get_packed().tobytes() == nets[3].get_packed().tobytes()
        s1, s2 = fused.state(), calls.state()
        assert s1["step"] == s2["step"] == 3
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert s1[k].tobytes() == s2[k].tobytes(), k
        assert fused.read()[0].tobytes() == calls.read()[0].tobytes()
        assert np.isfinite(losses).all()
        assert nets[0].get_packed().tobytes() != nets[1].get_packed().tobytes()     # tau < 1: two nets still
    finally:
        fused.close()
        calls.close()
        for p in nets:
            p.close()


def test_it_learns(gm, env, memory):
    from gmx.policy import DevicePolicy, DeviceLearner
    buf, _ = memory
    buf.pushed = CAP
    online, target = DevicePolicy(env, seed=1), DevicePolicy(env, seed=2)
    learner = DeviceLearner(online, target, learning_rate=1e-3)
    try:
        losses = learner.train(buf, 200, batch_size=128, seed=1, draw0=0).cpu().numpy()
        assert np.isfinite(losses).all()
        print(f"mean loss, first 20 updates {losses[:20].mean():.4f}, last 20 {losses[-20:].mean():.4f}")
        assert losses[-20:].mean() < losses[:20].mean()
    finally:
        learner.close()
        online.close()
        target.close()


def test_argument_errors(gm, env, memory):
    import torch
    from gmx.policy import DevicePolicy, DeviceLearner, LEARNER_MAX_BATCH
    from test_policy_rollout import make_env
    buf, _ = memory
    buf.pushed = CAP
    online = DevicePolicy(env, sizes=NETS["canonical"], seed=1)
    other_sizes = DevicePolicy(env, sizes=NETS["widest-narrowest"], seed=1)
    learner = DeviceLearner(online, other_sizes)
    env2 = make_env(gm, n=16)
    foreign = DevicePolicy(env2, sizes=NETS["canonical"], seed=1)
    try:
        n = LEARNER_MAX_BATCH + 1
        with pytest.raises(RuntimeError, match="holds"):             # batch above the learner's maximum
            learner.grad(first_rows(buf, n), torch.zeros(n, device=buf.state.device))
        with pytest.raises(RuntimeError, match="holds"):
            DeviceLearner(online).train(buf, 1, batch_size=n)
        with pytest.raises(RuntimeError, match="layer sizes"):       # mismatched sizes
            other_sizes.soft_update(online, 0.05)
        with pytest.raises(RuntimeError, match="layer sizes"):
            learner.train(buf, 1, batch_size=16)
        with pytest.raises(RuntimeError, match="different contexts"):   # a policy from another context
            foreign.soft_update(online, 0.05)
        with pytest.raises(RuntimeError, match="different contexts"):
            DeviceLearner(online, foreign).train(buf, 1, batch_size=16)
        with pytest.raises(RuntimeError, match="n < 1"):
            learner.grad(first_rows(buf, 16), torch.zeros(0, device=buf.state.device))
        with pytest.raises(ValueError):
            DeviceLearner(online, optimiser="RMSProp")
    finally:
        learner.close()
        foreign.close()
        env2.close()
        online.close()
        other_sizes.close()
