"""The on-device SAC learner on the GPU (gm_sac_learner_*, gm_sac_soft_update) against torch
autograd and torch.optim on the CPU, on a crafted action replay memory of 128 rows filled from
torch (uniform observations and actions, normal rewards, end cycling 0 / 1 / 2).  No env-stepping.
The torch side is tests/sac_model.py's module with MLPActorCriticAC's parameter names.

Tolerances are the project's measured convention: every expected value is computed on the CPU in
float32 and in float64, and the device must agree with the float64 one within
8 x max|f32 - f64| + one f32 ulp of the largest magnitude (sac_model.bound), the maximum taken per
parameter tensor; for the scalar losses it is taken over the 128-row batch's per-row terms and the
mean (tests/test_ppo_learner.py's rule: one scalar's |f32 - f64| may be 0).  The actor loss's
reference uses the device's own draws z (the debug output, cast exactly) in u = mu + exp(ls) z.

Autograd's gradient has kinks -- where a ReLU pre-activation changes sign between f32 and f64, where
min(q1, q2) changes its argument, where the raw log_std crosses a clamp limit -- so the parameter
seed is the first below 64 (CPU, torch alone, the float64 mirror of the draws) whose float64 values
keep clear of all of them in EVERY row: each ReLU pre-activation of every net at every point it is
evaluated (the critics on the memory's actions, the actor, the critics on the actor's actions)
further from 0 than 8 x max|pre32 - pre64|, |q1 - q2| on the actor-loss rows above the bound on
q1 - q2, the raw log_std further from -20 and 2 than its bound.  No row is left out, and the guard
is checked again on what the device itself drew and on its own backup y.

The search asks one thing more of a seed, from the reference's own error alone (well_posed).
8 x max|f32 - f64| estimates the f32 evaluation error of a tensor from ONE f32 evaluation, torch's;
where a tensor has one live element (n = 1 on the (3, 256) and (256, 3) nets: one row, three units,
two of them dead) that one number can equal the f64 one to a hundredth of its ulp by chance, and
the bound collapses below what any f32 summation order gives.  So a seed also has to be one whose
bounds torch itself meets in a second f32 evaluation of the same network: the hidden units of every
layer in reverse order (weights permuted to match, the same function; only the order of the f32
sums changes), for every parameter tensor of both losses and every n.  The bound itself is
unchanged, and is still formed from the unpermuted module alone.

Adam's first steps are ~ lr sign(g) where g ~ 0,
so the optimisers are never compared end to end with autograd: the device's own gradient is read
back and fed to torch.optim.  Measured worst |device - f64| / bound: see DESIGN.md, "SAC learner".

test_it_learns' inputs: the crafted memory below (generator seed 11), nets (256, 256) ReLU from
init_params seeds 1 (online) and 2 (target), Adam at lr 1e-3, batch 128 = the whole memory,
gamma 0.99, alpha 0.2, target frozen.  The torch module runs the same loop on the CPU (its own
normal draws) from a mean loss_q of 1.32 over the first 20 updates to 0.015 over the last 20."""
import numpy as np
import pytest

from conftest import gpu_available
from sac_model import module_from_flat, in_dtype, logp_of, bound, LOG_STD_MIN, LOG_STD_MAX

pytestmark = pytest.mark.gpu

CAP, N_ENVS = 128, 16
GAMMA, ALPHA = 0.99, 0.2
NS = (1, 17, 37, 128)            # one row, one row into a second tile, a partial tile, 8 full tiles
NETS = {"tanh20": dict(hidden=(20, 20), activation="tanh", action_limit=0.5),
        "wide-narrow": dict(hidden=(256, 3), activation="relu", action_limit=1.0),
        "narrow-wide": dict(hidden=(3, 256), activation="relu", action_limit=1.0),
        "spill": dict(hidden=(256, 256), activation="relu", action_limit=1.0)}    # the rows leave LDS
NOISE_SEED, DRAW = 77, 21


@pytest.fixture(scope="module")
def env(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    from test_sac_rollout import make_env
    e = make_env(gm, n=N_ENVS)
    yield e
    e.close()


@pytest.fixture(scope="module")
def memory(env):
    """The crafted memory, made once and left unchanged: (ActionReplayBuffer, its rows as numpy)."""
    import torch
    from gmx import ActionReplayBuffer
    g = torch.Generator().manual_seed(11)
    rows = dict(state=torch.rand((CAP, env.n_obs), generator=g) * 2 - 1,
                action=torch.rand((CAP, env.n_actions), generator=g) * 2 - 1,
                next_state=torch.rand((CAP, env.n_obs), generator=g) * 2 - 1,
                reward=torch.randn((CAP,), generator=g),
                end=(torch.arange(CAP) % 3).to(torch.uint8))
    buf = ActionReplayBuffer(env, CAP)
    for k, v in rows.items():
        getattr(buf, k).copy_(v)
    torch.cuda.synchronize()
    return buf, {k: v.numpy() for k, v in rows.items()}


def first_rows(buf, n):
    """The first n rows of the crafted memory as a batch (device views)."""
    return {k: getattr(buf, k)[:n] for k in ("state", "action", "next_state", "reward", "end")}


def make_sac(env, net, seed=0, params=None):
    from gmx import DeviceSAC
    return DeviceSAC(env, seed=seed, params=params, **NETS[net])


def module(env, net, flat):
    return module_from_flat(env.n_obs, env.n_actions, NETS[net]["hidden"], NETS[net]["activation"], flat)


def tensor_names(mod):
    return [k for k, _ in mod.named_parameters()]


def split(mod, flat):
    """{parameter name: view of a flat numpy array}, parameters() order being the flat order."""
    out, pos = {}, 0
    for k, p in mod.named_parameters():
        out[k] = flat[pos:pos + p.numel()]
        pos += p.numel()
    assert pos == flat.size
    return out


def layers(seq, x):
    """(outputs of every Linear of an nn.Sequential, its result)."""
    import torch
    lin, h = [], x
    for m in seq:
        h = m(h)
        if isinstance(m, torch.nn.Linear):
            lin.append(h)
    return lin, h


def critic_eval(mod, o, a):
    """(hidden pre-activations of both critics, q1, q2) on cat(o, a)."""
    import torch
    x = torch.cat([o, a], dim=-1)
    l1, q1 = layers(mod.q1.q, x)
    l2, q2 = layers(mod.q2.q, x)
    return l1[:-1] + l2[:-1], q1[:, 0], q2[:, 0]


def actor_eval(mod, o, z, limit):
    """The actor's reparameterised sample from given draws: hidden pre-activations, raw log_std, u,
    a and logp, all differentiable."""
    import torch
    pre, h = layers(mod.pi.net, o)
    mu, raw = mod.pi.mu_layer(h), mod.pi.log_std_layer(h)
    ls = torch.clamp(raw, LOG_STD_MIN, LOG_STD_MAX)
    u = mu + torch.exp(ls) * z
    return dict(pre=pre, raw=raw, mu=mu, u=u, a=limit * torch.tanh(u), logp=logp_of(u, mu, ls))


def ref_q(mod, o, a, y):
    """compute_loss_q with autograd: (per-row terms of both critics, loss_q, {name: gradient})."""
    import torch
    _, q1, q2 = critic_eval(mod, o, a)
    r1, r2 = (q1 - y) ** 2, (q2 - y) ** 2
    loss = r1.mean() + r2.mean()
    ps = {k: p for k, p in mod.named_parameters() if k.startswith("q")}
    gs = torch.autograd.grad(loss, list(ps.values()))
    return torch.cat([r1, r2]).detach(), loss.detach(), dict(zip(ps, gs))


def ref_pi(mod, o, z, alpha, limit):
    """compute_loss_pi with autograd through the critics into the actor: the sample, both critics,
    the per-row terms, loss_pi and {name: gradient} of the actor's tensors (the critics frozen)."""
    import torch
    s = actor_eval(mod, o, z, limit)
    _, q1, q2 = critic_eval(mod, o, s["a"])
    rows = alpha * s["logp"] - torch.min(q1, q2)
    loss = rows.mean()
    ps = {k: p for k, p in mod.named_parameters() if k.startswith("pi.")}
    gs = torch.autograd.grad(loss, list(ps.values()))
    out = {k: s[k].detach() for k in ("u", "a", "logp")}
    out.update(q1=q1.detach(), q2=q2.detach(), rows=rows.detach(), loss=loss.detach(), grads=dict(zip(ps, gs)))
    return out


def clear_of_kinks(mod, relu, o, a_mem, z, limit):
    """Every row of the 128 clear of every kink of both losses (see the module docstring):
    (ok, figures)."""
    import torch
    with torch.no_grad():
        ev = {}
        for dt in (torch.float32, torch.float64):
            m = in_dtype(mod, dt)
            od = torch.from_numpy(o).to(dt)
            s = actor_eval(m, od, torch.from_numpy(z).to(dt), limit)
            pre_mem, _, _ = critic_eval(m, od, torch.from_numpy(a_mem).to(dt))
            pre_pi, q1, q2 = critic_eval(m, od, s["a"])
            ev[dt] = dict(points=[pre_mem, s["pre"], pre_pi], gap=q1 - q2, raw=s["raw"])
        e32, e64 = ev[torch.float32], ev[torch.float64]
        margin = np.inf                     # min over the evaluation points of min|pre64| / (8 max|pre32 - pre64|)
        if relu:
            for p32s, p64s in zip(e32["points"], e64["points"]):
                diff = max(float((p32.double() - p64).abs().max()) for p32, p64 in zip(p32s, p64s))
                near0 = min(float(p64.abs().min()) for p64 in p64s)
                margin = min(margin, near0 / (8.0 * diff))
        gap = float(e64["gap"].abs().min()) / bound(e32["gap"], e64["gap"])
        raw = e64["raw"]
        clamp = float(torch.minimum((raw - LOG_STD_MIN).abs(), (raw - LOG_STD_MAX).abs()).min()) / bound(e32["raw"], raw)
    return margin > 1.0 and gap > 1.0 and clamp > 1.0, dict(relu_margin=margin, min_gap_over_bound=gap,
                                                             clamp_distance_over_bound=clamp)


def cpu_backup(env, net, flat_target, mod, rows):
    """compute_loss_q's backup on the CPU in f32 (the search's stand-in for the device's y): the
    actor `mod` on next_state with the mirror of draw DRAW - 1, the critics of the target seed."""
    import torch
    from gmx.sac import normal_draws
    with torch.no_grad():
        o2 = torch.from_numpy(rows["next_state"])
        z = torch.from_numpy(normal_draws(NOISE_SEED, np.arange(CAP), DRAW - 1, env.n_actions).astype(np.float32))
        s = actor_eval(mod, o2, z, NETS[net]["action_limit"])
        _, q1, q2 = critic_eval(module(env, net, flat_target), o2, s["a"])
        boots = torch.from_numpy(rows["end"] == 0)
        y = torch.from_numpy(rows["reward"]) + GAMMA * boots * (torch.min(q1, q2) - ALPHA * s["logp"])
    return y.numpy()


def reversed_units(tensors, back=False):
    """{name: tensor} of the module's parameters (or their gradients) with the hidden units of
    every layer in reverse order: rows of a layer that feeds a hidden layer, columns of a layer that
    reads one.  Its own inverse."""
    import torch
    out = {}
    for k, t in tensors.items():
        net, layer = k.rsplit(".", 2)[0], k.rsplit(".", 2)[1]       # e.g. "q1.q", "4"; "pi.net", "2"; "pi", "mu_layer"
        if net == "pi":
            feeds, reads = False, True                               # the heads read the last hidden layer
        else:
            last = max(int(x.rsplit(".", 2)[1]) for x in tensors if x.startswith(net + "."))
            feeds = net == "pi.net" or int(layer) < last             # every pi.net layer is followed by its activation
            reads = int(layer) > 0
        if feeds:
            t = torch.flip(t, [0])
        if reads and t.dim() == 2:
            t = torch.flip(t, [1])
        out[k] = t.contiguous()
    return out


def well_posed(mod, o, a, y, z, limit, ns=NS):
    """For every parameter tensor of both losses and every n: torch's f32 gradient of the same
    network with its hidden units in reverse order is inside the bound formed from the module as
    it stands (see the module docstring).  (ok, worst |f32 reversed - f64| / bound)."""
    import copy
    import torch
    m32, m64 = in_dtype(mod, torch.float32), in_dtype(mod, torch.float64)
    rev = copy.deepcopy(m32)
    rev.load_state_dict(reversed_units({k: p.detach() for k, p in m32.named_parameters()}))
    worst = 0.0
    for n in ns:
        o32, a32, y32, z32 = (torch.from_numpy(x[:n]) for x in (o, a, y, z))
        g32 = dict(ref_q(m32, o32, a32, y32)[2], **ref_pi(m32, o32, z32, ALPHA, limit)["grads"])
        g64 = dict(ref_q(m64, o32.double(), a32.double(), y32.double())[2],
                   **ref_pi(m64, o32.double(), z32.double(), ALPHA, limit)["grads"])
        other = reversed_units(dict(ref_q(rev, o32, a32, y32)[2], **ref_pi(rev, o32, z32, ALPHA, limit)["grads"]))
        for k in g64:
            err = float((other[k].double() - g64[k]).abs().max())
            worst = max(worst, err / bound(g32[k].reshape(-1), g64[k].reshape(-1)))
    return worst <= 1.0, worst


def mirror_z(n_actions):
    """The float64 mirror of the device's draws for batch rows 0 .. 127, as float32's values."""
    from gmx.sac import normal_draws
    return normal_draws(NOISE_SEED, np.arange(CAP), DRAW, n_actions).astype(np.float32)


_SEEDS = {}


def choose_seed(env, net, rows, edit=None, key=None):
    """The first parameter seed below 64 (CPU, torch alone) that keeps all 128 rows clear of every
    kink; edit(flat params) -> flat params crafts the weights first.  Searched once per case."""
    from gmx.sac import init_params, sizes
    key = key or net
    if key not in _SEEDS:
        psz, qsz = sizes(env.n_obs, env.n_actions, NETS[net]["hidden"])
        z = mirror_z(env.n_actions)
        for seed in range(64):
            flat = init_params(psz, qsz, seed)
            flat = edit(flat) if edit else flat
            mod = module(env, net, flat)
            ok, fig = clear_of_kinks(mod, NETS[net]["activation"] == "relu", rows["state"], rows["action"], z,
                                     NETS[net]["action_limit"])
            if ok:       # (the cheaper test first)
                ok, fig["reversed_f32_over_bound"] = well_posed(
                    mod, rows["state"], rows["action"], cpu_backup(env, net, init_params(psz, qsz, 100), mod, rows), z,
                    NETS[net]["action_limit"])
            if ok:
                _SEEDS[key] = (seed, flat, fig)
                break
        else:
            raise AssertionError(f"{key}: no parameter seed below 64 keeps every row clear of autograd's kinks")
    return _SEEDS[key]


def compare(name, dev, t32, t64, worst, label):
    b = bound(t32.reshape(-1), t64.reshape(-1))
    err = float(np.abs(np.asarray(dev, dtype=np.float64).reshape(-1) - t64.reshape(-1).numpy()).max())
    worst[name] = max(worst.get(name, 0.0), err / b)
    print(f"{label} {name}: max |device - f64| {err:.3e} bound {b:.3e} ratio {err / b:.3f}")
    assert np.isfinite(np.asarray(dev)).all(), f"{label} {name}: not finite"
    assert err <= b, f"{label} {name}: {err:.3e} > {b:.3e}"


def check_both_gradients(env, buf, rows, net, flat, label, ns=NS):
    """grad_q and grad_pi of a learner on `flat` against autograd for every n of ns; returns
    (worst ratios, the flat device gradient of the last n, the module)."""
    import torch
    from gmx import DeviceSACLearner
    limit, relu = NETS[net]["action_limit"], NETS[net]["activation"] == "relu"
    online, target = make_sac(env, net, params=flat), make_sac(env, net, seed=100)
    learner = DeviceSACLearner(online, target)
    mod = module(env, net, flat)
    mods = {dt: in_dtype(mod, dt) for dt in (torch.float32, torch.float64)}
    worst, g_dev = {}, None
    try:
        full = first_rows(buf, CAP)
        y_dev = target.target(full, GAMMA, ALPHA, online=online, seed=NOISE_SEED, draw=DRAW - 1)
        y = y_dev.cpu().numpy()
        # the device's own draws, and the guard again on them
        dbg = learner.grad_pi(full, ALPHA, seed=NOISE_SEED, draw=DRAW, debug=True)
        z = dbg["z"].cpu().numpy()
        assert np.abs(z - mirror_z(env.n_actions)).max() < 1e-5 and np.abs(z).max() > 1.5
        ok, fig = clear_of_kinks(mod, relu, rows["state"], rows["action"], z, limit)
        assert ok, f"the device's own draws move a row onto a kink: {fig}"
        ok, fig = well_posed(mod, rows["state"], rows["action"], y, z, limit, ns)
        assert ok, f"with the device's own y and z torch's reversed f32 evaluation leaves a tensor's bound: {fig}"
        # the rows of the scalars' bound: the whole 128-row batch
        full_q, full_pi = {}, {}
        for dt, m in mods.items():
            t = lambda x: torch.from_numpy(x).to(dt)                    # noqa: E731
            full_q[dt] = ref_q(m, t(rows["state"]), t(rows["action"]), t(y))
            full_pi[dt] = ref_pi(m, t(rows["state"]), t(z), ALPHA, limit)
        for k in ("u", "a", "logp", "q1", "q2"):
            compare(k, dbg[k].cpu().numpy(), full_pi[torch.float32][k], full_pi[torch.float64][k], worst, f"{label} n {CAP}")
        for n in ns:
            batch = first_rows(buf, n)
            learner.grad_q(batch, y_dev[:n].contiguous())
            g_q, loss_q, _ = learner.read()
            learner.grad_pi(batch, ALPHA, seed=NOISE_SEED, draw=DRAW)
            g_dev, loss_q2, loss_pi = learner.read()
            assert loss_q2 == loss_q
            rq, rp = {}, {}
            for dt, m in mods.items():
                t = lambda x: torch.from_numpy(x[:n]).to(dt)            # noqa: E731
                rq[dt] = ref_q(m, t(rows["state"]), t(rows["action"]), t(y))
                rp[dt] = ref_pi(m, t(rows["state"]), t(z), ALPHA, limit)
            f32, f64 = torch.float32, torch.float64
            for name, dev, r32, r64 in (("loss_q", loss_q, (full_q[f32][0], rq[f32][1]), (full_q[f64][0], rq[f64][1])),
                                        ("loss_pi", loss_pi, (full_pi[f32]["rows"], rp[f32]["loss"]),
                                         (full_pi[f64]["rows"], rp[f64]["loss"]))):
                b = bound(torch.cat([r32[0], r32[1][None]]), torch.cat([r64[0], r64[1][None]]))
                err = abs(dev - float(r64[1]))
                worst[name] = max(worst.get(name, 0.0), err / b)
                print(f"{label} n {n} {name}: device {dev:.9g} f64 {float(r64[1]):.9g} err {err:.3e} bound {b:.3e} "
                      f"ratio {err / b:.3f}")
                assert err <= b, f"{label} n {n} {name}: {err:.3e} > {b:.3e}"
            dev_t = split(mod, g_dev)
            assert split(mod, g_q).keys() == dev_t.keys()
            for k in tensor_names(mod):
                t32 = rq[f32][2][k] if k.startswith("q") else rp[f32]["grads"][k]
                t64 = rq[f64][2][k] if k.startswith("q") else rp[f64]["grads"][k]
                compare(k, dev_t[k], t32, t64, worst, f"{label} n {n}")
            # the actor-loss call left the critics' gradient as grad_q made it
            for k in tensor_names(mod):
                if k.startswith("q"):
                    assert split(mod, g_q)[k].tobytes() == dev_t[k].tobytes(), k
        print(f"{label}: worst |device - f64| / bound {worst}")
        return worst, g_dev, mod
    finally:
        learner.close()
        online.close()
        target.close()


@pytest.mark.parametrize("net", sorted(NETS))
def test_gradients_match_autograd(gm, env, memory, net):
    buf, rows = memory
    seed, flat, fig = choose_seed(env, net, rows)
    print(f"{net}: seed {seed}, {fig}")
    worst, g, mod = check_both_gradients(env, buf, rows, net, flat, net)
    for k, v in split(mod, g).items():
        assert np.abs(v).max() > 0, f"{k}: an all-zero gradient"


@pytest.mark.parametrize("bias", [30.0, -30.0])
def test_clamped_log_std_rows(gm, env, memory, bias):
    """log_std_layer.bias = +-30 puts every raw log_std outside the clamp: its layer's gradient is
    exactly 0 (torch's clamp passes none), the rest stays within the bound, finite where tanh
    saturates (std = e^2 under +30)."""
    from gmx.sac import flat_to_state_dict, params_from_state_dict, sizes
    buf, rows = memory
    net = "tanh20"
    psz, qsz = sizes(env.n_obs, env.n_actions, NETS[net]["hidden"])

    def edit(flat):
        sd = flat_to_state_dict(psz, qsz, flat)
        sd["pi.log_std_layer.bias"][:] = bias
        return params_from_state_dict(sd)[2]
    seed, flat, fig = choose_seed(env, net, rows, edit, key=f"{net}{bias:+.0f}")
    print(f"{net} bias {bias:+.0f}: seed {seed}, {fig}")
    worst, g, mod = check_both_gradients(env, buf, rows, net, flat, f"{net} bias {bias:+.0f}", ns=(37, 128))
    g = split(mod, g)
    for k in ("pi.log_std_layer.weight", "pi.log_std_layer.bias"):
        assert (g[k] == 0.0).all(), f"{k}: {int((g[k] != 0).sum())} non-zero entries"
    assert np.abs(g["pi.mu_layer.weight"]).max() > 0


@pytest.mark.parametrize("net", ["tanh20", "spill"])
def test_gradients_are_deterministic(gm, env, memory, net):
    from gmx import DeviceSACLearner
    buf, _ = memory
    online = make_sac(env, net, seed=5)
    learner = DeviceSACLearner(online)
    try:
        batch = first_rows(buf, CAP)
        y = (batch["reward"] * 0.5).contiguous()

        def both(b, yy):
            learner.grad_q(b, yy)
            learner.grad_pi(b, ALPHA, seed=3, draw=4)
            return learner.read()
        g1, q1, p1 = both(batch, y)
        both(first_rows(buf, 37), y[:37].contiguous())            # other gradients in between
        learner.grad_pi(batch, ALPHA, seed=3, draw=5)             # and other noise
        g_other = learner.read()[0]
        g2, q2, p2 = both(batch, y)
        assert g1.tobytes() == g2.tobytes()
        assert np.float32(q1).tobytes() == np.float32(q2).tobytes() and np.float32(p1).tobytes() == np.float32(p2).tobytes()
        assert np.abs(g1).max() > 0 and g_other.tobytes() != g1.tobytes()
    finally:
        learner.close()
        online.close()


OPT_CASES = {"adam": (dict(optimiser="adam"), dict(weight_decay=0.0, amsgrad=False)),
             "adamw": (dict(optimiser="adamW"), dict(weight_decay=0.01, amsgrad=True))}


@pytest.mark.parametrize("case", sorted(OPT_CASES))
@pytest.mark.parametrize("net", ["tanh20", "wide-narrow"])
def test_optimiser_steps_match_torch_elementwise(gm, env, memory, net, case):
    import torch
    from gmx import DeviceSACLearner
    opts, tkw = OPT_CASES[case]
    buf, _ = memory
    online = make_sac(env, net, seed=0)
    learner = DeviceSACLearner(online, **opts)
    clone = copy = None
    worst = 0.0
    try:
        batch = first_rows(buf, CAP)
        y = (batch["reward"] + np.float32(0.99 * 0.3)).contiguous()
        cls = torch.optim.AdamW if case == "adamw" else torch.optim.Adam
        mod = module(env, net, online.params)
        ref = {}
        for dt in (torch.float32, torch.float64):
            ts = {k: p.detach().clone().requires_grad_(True) for k, p in in_dtype(mod, dt).named_parameters()}
            kw = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, **tkw)
            ref[dt] = (ts, cls([t for k, t in ts.items() if k.startswith("q")], **kw),
                       cls([t for k, t in ts.items() if k.startswith("pi.")], **kw))

        def check(which, g, before):
            nonlocal worst
            after = split(mod, online.get_params())
            mine = (lambda k: k.startswith("q")) if which == 1 else (lambda k: k.startswith("pi."))
            for dt, r in ref.items():
                for k, t in r[0].items():
                    t.grad = torch.from_numpy(split(mod, g)[k].copy()).reshape(t.shape).to(dt) if mine(k) else None
                r[which].step()
            for k in after:
                if not mine(k):                                        # the other optimiser's range: bit-unchanged
                    assert after[k].tobytes() == split(mod, before)[k].tobytes(), k
                    continue
                t32, t64 = (ref[dt][0][k].detach().reshape(-1) for dt in (torch.float32, torch.float64))
                b = bound(t32, t64)
                err = float(np.abs(after[k].astype(np.float64) - t64.numpy()).max())
                worst = max(worst, err / b)
                assert err <= b, f"{case} {k}: {err:.3e} > {b:.3e}"
        for step in range(1, 6):
            before = online.get_params()
            learner.grad_q(batch, y)
            g = learner.read()[0]
            learner.step_q()
            check(1, g, before)
            before = online.get_params()
            learner.grad_pi(batch, ALPHA, seed=NOISE_SEED, draw=step)
            g = learner.read()[0]
            learner.step_pi()
            check(2, g, before)
            print(f"{net} {case} step {step}: worst |device - f64| / bound so far {worst:.3f}")
        # the state round trip: a rebuilt learner on a copy of the weights takes the same next step
        copy = make_sac(env, net, params=online.get_params())
        clone = DeviceSACLearner(copy, **opts)
        state = learner.state()
        assert state["step_q"] == state["step_pi"] == 5 and np.abs(state["exp_avg"]).max() > 0
        assert (np.abs(state["max_exp_avg_sq"]).max() > 0) == (case == "adamw")
        clone.load_state(state)
        for l in (learner, clone):
            l.grad_q(batch, y)
            l.step_q()
            l.grad_pi(batch, ALPHA, seed=NOISE_SEED, draw=9)
            l.step_pi()
        assert online.get_params().tobytes() == copy.get_params().tobytes()
        s1, s2 = learner.state(), clone.state()
        assert s1["step_q"] == s2["step_q"] == 6 and s1["step_pi"] == s2["step_pi"] == 6
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert s1[k].tobytes() == s2[k].tobytes(), k
    finally:
        for x in (clone, copy, learner, online):
            if x is not None:
                x.close()


@pytest.mark.parametrize("tau", [0.05, 1.0])
@pytest.mark.parametrize("net", ["tanh20", "spill"])
def test_soft_update(gm, env, net, tau):
    online, target = make_sac(env, net, seed=6), make_sac(env, net, seed=7)
    try:
        p, t = online.get_params(), target.get_params()
        target.soft_update(online, tau)
        got = target.get_params()
        tau64 = float(np.float32(tau))                               # the value the C ABI's float carries
        want = p.astype(np.float64) * tau64 + t.astype(np.float64) * (1.0 - tau64)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        worst = float((np.abs(got.astype(np.float64) - want) / ulp).max())
        print(f"{net} tau {tau}: worst error {worst:.3f} ulp over all three nets")
        assert worst <= 0.5
        if tau == 1.0:
            assert got.tobytes() == p.tobytes()
        assert (got != t).mean() > 0.9
        assert online.get_params().tobytes() == p.tobytes()          # the online handle is only read
    finally:
        online.close()
        target.close()


def test_padding_stays_zero_under_training(gm, env, memory):
    from gmx import DeviceSACLearner
    from gmx.sac import pack
    net = "wide-narrow"
    buf, _ = memory
    buf.pushed = CAP
    online, target = make_sac(env, net, seed=3), make_sac(env, net, seed=4)
    learner = DeviceSACLearner(online, target, optimiser="adamW", learning_rate=1e-3)     # decay, amsgrad, polyak
    try:
        pad = pack(online.pi_sizes, online.q_sizes, np.ones(online.params.size, dtype=np.float32))[0] == 0
        assert pad.any()
        before = online.get_packed()
        learner.train(buf, 20, batch_size=37, seed=2, draw0=0)
        for name, h in (("online", online), ("target", target)):
            packed = h.get_packed()
            assert (packed[pad] == 0.0).all(), f"{name}: {int((packed[pad] != 0).sum())} padding entries moved"
        assert (online.get_packed()[~pad] != before[~pad]).mean() > 0.9       # and the weights did move
    finally:
        learner.close()
        online.close()
        target.close()


@pytest.mark.parametrize("pushed", [100, 3 * CAP + 17])             # size < capacity; a wrapped ring
@pytest.mark.parametrize("net", ["tanh20", "spill"])
def test_train_equals_the_calls_it_enqueues(gm, env, memory, net, pushed):
    from gmx import DeviceSACLearner
    buf, _ = memory
    nets = [make_sac(env, net, seed=s) for s in (8, 9, 8, 9)]          # online, target, twice
    kw = dict(optimiser="adamW", learning_rate=1e-3, soft_target_tau=0.05, gamma=GAMMA, alpha=ALPHA)
    fused, calls = DeviceSACLearner(nets[0], nets[1], **kw), DeviceSACLearner(nets[2], nets[3], **kw)
    try:
        buf.pushed = pushed
        assert len(buf) == min(pushed, CAP)
        losses = fused.train(buf, 3, batch_size=37, seed=12, noise_seed=5, draw0=40).cpu().numpy()
        by_call = []
        for u in range(3):
            d = 40 + u
            batch = buf.sample(37, seed=12, draw=d)
            y = nets[3].target(batch, GAMMA, ALPHA, online=nets[2], seed=5, draw=2 * d)
            calls.grad_q(batch, y)
            calls.step_q()
            calls.grad_pi(batch, ALPHA, seed=5, draw=2 * d + 1)
            calls.step_pi()
            by_call.append(calls.read()[1:])
            nets[3].soft_update(nets[2], 0.05)
        assert losses.tobytes() == np.asarray(by_call, dtype=np.float32).tobytes()
        assert nets[0].get_packed().tobytes() == nets[2].get_packed().tobytes()
        assert nets[1].get_packed().tobytes() == nets[3].get_packed().tobytes()
        s1, s2 = fused.state(), calls.state()
        assert s1["step_q"] == s2["step_q"] == 3 and s1["step_pi"] == s2["step_pi"] == 3
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert s1[k].tobytes() == s2[k].tobytes(), k
        assert fused.read()[0].tobytes() == calls.read()[0].tobytes()
        assert np.isfinite(losses).all() and np.abs(fused.read()[0]).max() > 0
        assert nets[0].get_packed().tobytes() != nets[1].get_packed().tobytes()     # tau < 1: two nets still
    finally:
        buf.pushed = CAP
        fused.close()
        calls.close()
        for p in nets:
            p.close()


def test_it_learns(gm, env, memory):
    from gmx import DeviceSACLearner
    buf, _ = memory
    buf.pushed = CAP
    online, target = make_sac(env, "spill", seed=1), make_sac(env, "spill", seed=2)
    learner = DeviceSACLearner(online, target, learning_rate=1e-3)
    try:
        frozen = target.get_packed()
        losses = learner.train(buf, 200, batch_size=CAP, seed=1, noise_seed=2, draw0=0, tau=0.0).cpu().numpy()
        assert np.isfinite(losses).all()
        print(f"mean loss_q, first 20 updates {losses[:20, 0].mean():.4f}, last 20 {losses[-20:, 0].mean():.4f}; "
              f"loss_pi {losses[:20, 1].mean():.4f} -> {losses[-20:, 1].mean():.4f}")
        assert losses[-20:, 0].mean() < losses[:20, 0].mean()
        assert target.get_packed().tobytes() == frozen.tobytes()      # tau = 0: the target is left alone
    finally:
        learner.close()
        online.close()
        target.close()


def test_argument_errors(gm, env, memory):
    import torch
    from gmx import DeviceSACLearner
    from gmx.sac import LEARNER_MAX_BATCH
    from test_sac_rollout import make_env
    buf, _ = memory
    buf.pushed = CAP
    online, other = make_sac(env, "tanh20", seed=1), make_sac(env, "wide-narrow", seed=1)
    learner = DeviceSACLearner(online, other)
    env2 = make_env(gm, n=16)
    foreign = make_sac(env2, "tanh20", seed=1)
    try:
        n = LEARNER_MAX_BATCH + 1
        dev = buf.state.device
        big = dict(state=torch.zeros((n, env.n_obs), device=dev), action=torch.zeros((n, env.n_actions), device=dev))
        with pytest.raises(RuntimeError, match="holds"):             # batch above the learner's maximum
            learner.grad_q(big, torch.zeros(n, device=dev))
        with pytest.raises(RuntimeError, match="holds"):
            learner.grad_pi(big)
        with pytest.raises(RuntimeError, match="holds"):
            DeviceSACLearner(online, online).train(buf, 1, batch_size=n, tau=0.0)
        with pytest.raises(RuntimeError, match="n < 1"):
            learner.grad_q(first_rows(buf, 16), torch.zeros(0, device=dev))
        with pytest.raises(RuntimeError, match="network sizes"):     # mismatched handles
            other.soft_update(online, 0.05)
        with pytest.raises(RuntimeError, match="network sizes"):
            learner.train(buf, 1, batch_size=16)
        with pytest.raises(RuntimeError, match="different contexts"):   # a handle from another context
            foreign.soft_update(online, 0.05)
        with pytest.raises(RuntimeError, match="different contexts"):
            DeviceSACLearner(online, foreign).train(buf, 1, batch_size=16)
        with pytest.raises(RuntimeError, match="of its own"):        # a polyak update onto the online handle
            DeviceSACLearner(online, online).train(buf, 1, batch_size=16)
        with pytest.raises(ValueError, match="RMSprop"):
            DeviceSACLearner(online, optimiser="RMSProp")
        with pytest.raises(ValueError, match="incorrect key"):
            DeviceSACLearner(online, grad_clamp_value=100)
    finally:
        learner.close()
        foreign.close()
        env2.close()
        online.close()
        other.close()
