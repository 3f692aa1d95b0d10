"""The collider on crafted edge poses and at contact capacity (tests/contact_cases.py).

test_oracle_matches_closed_form (CPU): every closed-form case through one oracle substep
from its record against the numpy closed form, the oracle-only cases against or_collide on
the independent FK poses, and the asserts that keep the table from being vacuous (which
side of a threshold a pose falls on, how many candidates the capacity states carry, which
contacts come from the second 64-pair batch).

test_device_matches_oracle_and_closed_form (GPU): the same records on the device, one
debug substep, against the oracle's substep and directly against the closed form, under the
default dispatch and with GM_DUO forced on and off.  The diagnostic substep always runs the
one-wave kernel (gm_capi.hip launch_step: DUO workgroups run the env-step proper), so
test_duo_env_step_from_crafted_states_equals_one_wave runs one whole env-step from the same
records on DUO workgroups (the helper wave's collider, its own box-box hit slots, both pair
batches) and on the one-wave kernel and asserts the states equal bit for bit.

What the table could not reach, searched for on the CPU: contacts of a box-box face lane
of rank >= GM_BB_SLOTS (18) that are kept.  Such a lane needs 18 face-case pairs before it,
each with at least one contact and in every pose found at least two, so its contacts start
past slot 32 and its guarded stores drop them (the engulfing states run that path: 31 and
37 face lanes); only ncon, overflow and the kept contacts before it can be compared there.
ncon == 32 exactly without overflow was found (the slab on six segments).

Measured on an MI355X, worst |device - oracle| / |device - closed form| per family (contact
geometry): see DESIGN.md, "GM_MAX_CON = 32".
"""
import os

import numpy as np
import pytest

import contact_cases as cc
from conftest import gpu_available

GM_MAX_CON = 32
GM_BB_SLOTS = 18


class Table:
    def __init__(self, gm, n_seg):
        import oracle_lib as ol
        self.sc = cc.Scene(gm, n_seg)
        self.cases = cc.make_cases(self.sc)
        self.objs, self.recs = cc.build_records(self.sc, self.cases)
        sc = self.sc
        self.ncon, self.nefc, self.con, self.efc, self.qacc, self.w, self.after = \
            ol.batch_substep(sc.model, sc.cfg, self.objs, self.recs)
        for a in (self.ncon, self.nefc, self.con, self.efc, self.qacc, self.after, self.recs):
            a.setflags(write=False)


_tables = {}


@pytest.fixture(scope="module")
def tables(gm):
    def get(n_seg):
        if n_seg not in _tables:
            _tables[n_seg] = Table(gm, n_seg)
        return _tables[n_seg]
    return get


def pair_ids(con, n):
    return [(int(con[k, 13]), int(con[k, 14])) for k in range(n)]


def is_mpr_pair(sc, case, g1, g2):
    return case.otype == cc.CYL and sc.g_ground not in (g1, g2)


def against_closed_form(sc, case, ncon, con, who):
    """ncon, the pair ids in candidate-pair order and every contact against the closed form
    (within a pair matched by position): 1e-12 absolute, MPR pairs at the collider's own
    tolerance on depth and normal.  Returns the worst error of the 1e-12 kind (for an MPR
    case the worst depth error instead)."""
    exp = case.expected
    assert ncon == len(exp) == case.counts, f"{who}, {case.name}: ncon {ncon}, closed form {len(exp)}, stated {case.counts}"
    ids = pair_ids(con, ncon)
    assert ids == [(e["g1"], e["g2"]) for e in exp], f"{who}, {case.name}: pair ids {ids}"
    used, worst = set(), 0.0
    for e in exp:
        cand = [k for k in range(ncon) if k not in used and ids[k] == (e["g1"], e["g2"])]
        k = cand[0] if e["pos"] is None else min(cand, key=lambda k: np.abs(con[k, 1:4] - e["pos"]).max())
        used.add(k)
        n = con[k, 4:7]
        if e["mpr"]:
            assert abs(con[k, 0] - e["dist"]) <= cc.MPR_DEPTH, f"{who}, {case.name}: depth {con[k, 0]!r} vs {e['dist']!r}"
            assert np.abs(n - e["n"]).max() <= cc.MPR_NORMAL, f"{who}, {case.name}: normal {n} vs {e['n']}"
            worst = max(worst, abs(con[k, 0] - e["dist"]))
        else:
            err = max(abs(con[k, 0] - e["dist"]), np.abs(con[k, 1:4] - e["pos"]).max(), np.abs(n - e["n"]).max())
            assert err <= 1e-12, f"{who}, {case.name}: contact {con[k, :7]} vs dist {e['dist']!r} pos {e['pos']} n {e['n']}"
            worst = max(worst, err)
        # the frame is orthonormal and right-handed
        F = con[k, 4:13].reshape(3, 3)
        assert np.abs(F @ F.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(F) > 0.5, f"{who}, {case.name}: frame"
    return worst


def kept_ids_from_pair_counts(counts):
    ids = [(g1, g2) for g1, g2, n in counts for _ in range(n)]
    return ids[:GM_MAX_CON], len(ids)


def case_named(t, part):
    hits = [i for i, c in enumerate(t.cases) if part in c.name]
    assert len(hits) == 1, (part, hits)
    return hits[0], t.cases[hits[0]]


@pytest.mark.parametrize("n_seg", [8, 10])
def test_oracle_matches_closed_form(gm, tables, n_seg):
    t = tables(n_seg)
    sc = t.sc
    ov = gm.env_state_view(t.after)
    worst = {}
    for i, c in enumerate(t.cases):
        assert np.isfinite(t.qacc[i]).all() and np.isfinite(t.efc[i]).all(), c.name
        if c.kind == cc.CLOSED:
            w = against_closed_form(sc, c, int(t.ncon[i]), t.con[i], "oracle")
            worst[c.family] = float(max(worst.get(c.family, 0.0), w))
            assert int(ov["overflow"][i]) == 0
        else:
            # pair ids and per-pair counts: or_collide on the independent FK poses, in pair
            # order, cut at GM_MAX_CON
            ids, total = kept_ids_from_pair_counts(cc.oracle_pair_counts(sc, c))
            assert pair_ids(t.con[i], int(t.ncon[i])) == ids, c.name
            assert int(t.ncon[i]) == min(total, GM_MAX_CON) and int(ov["overflow"][i]) == (total > GM_MAX_CON), c.name
        assert int(t.nefc[i]) == 4 * int(t.ncon[i]) + sc.m.nlock, c.name
    print(f"\nN = {n_seg}: worst |oracle - closed form| per family {worst}")
    assert sum(c.kind == cc.CLOSED for c in t.cases) >= (38 if n_seg == 8 else 3)

    # ---- the table is not vacuous
    # second pair batch / its one-batch control: the hooks' ground contacts
    i, c = case_named(t, "hooks in the ground, box on the ground")
    ids = pair_ids(t.con[i], int(t.ncon[i]))
    pidx = [sc.pair_index(*p) for p in ids]
    assert pidx == sorted(pidx) and pidx[0] == 0 and len(set(pidx)) == 4
    hook3 = sc.pair_index(sc.g_ground, sc.finger_geom(2, sc.n_seg + 1))
    if n_seg == 10:
        assert sc.npair == 75
        late = [(k, p) for k, p in enumerate(pidx) if p >= 64]
        assert late and all(k > 0 for k, _ in late) and hook3 >= 64, "no kept contact from the second pair batch"
        assert any(p < 64 and p > 0 for p in pidx), "no ground-finger contact from the first batch"
        # the cut at GM_MAX_CON against the batches: kept contacts of the second batch at
        # slots 28, 29; then 32 from the first batch alone and the overflow from the second
        i4, _ = case_named(t, "slab on 4 segments")
        p4 = [sc.pair_index(*p) for p in pair_ids(t.con[i4], int(t.ncon[i4]))]
        assert int(t.ncon[i4]) == 30 and [k for k, p in enumerate(p4) if p >= 64] == [28, 29] and not ov["overflow"][i4]
        i5, c5 = case_named(t, "slab on 5 segments")
        counts = cc.oracle_pair_counts(sc, c5)
        assert sum(n for (_, _, n) in counts[:64]) == GM_MAX_CON and sum(n for (_, _, n) in counts[64:]) == 2
        assert int(t.ncon[i5]) == GM_MAX_CON and int(ov["overflow"][i5]) == 1
    else:
        assert sc.npair == 63 and hook3 < 64
    # the engulfing state: >= 19 gripper-object pairs with a manifold (more face-case lanes
    # than hit slots), more candidates than GM_MAX_CON, a converged solve at full width
    engulfing = [i for i, c in enumerate(t.cases) if "engulfing" in c.name]
    assert engulfing
    for i in engulfing:
        counts = cc.oracle_pair_counts(sc, t.cases[i])
        assert sum(1 for g1, g2, n in counts if n >= 2 and sc.g_ground not in (g1, g2)) >= GM_BB_SLOTS + 1
        assert sum(n for _, _, n in counts) > GM_MAX_CON
        assert int(t.ncon[i]) == GM_MAX_CON and int(ov["overflow"][i]) == 1
        assert int(t.nefc[i]) == 4 * GM_MAX_CON + sc.m.nlock
    caps0 = gm.env_state_view(t.recs)["newton_caps"]
    for i, c in enumerate(t.cases):
        if c.capacity:
            assert int(ov["newton_caps"][i]) == int(caps0[i]), f"{c.name}: the solve ran into a cap"
    if n_seg == 8:
        # full width without overflow, and exactly GM_MAX_CON without overflow
        i, _ = case_named(t, "(ncon 28)")
        assert 25 <= int(t.ncon[i]) < GM_MAX_CON and not ov["overflow"][i]
        i, _ = case_named(t, "(ncon 32, no overflow)")
        assert int(t.ncon[i]) == GM_MAX_CON and not ov["overflow"][i]
        # the thresholds: which side each pose is on, a factor of two or more away
        for part, fallback in (("cylinder upright", True), ("5e-7 (fallback", True), ("2e-6 (rim", False),
                               ("skew axis", False), ("tilted 20 deg", False)):
            _, c = case_named(t, part)
            lw = cc.cyl_rim_dir(c.R)[1]
            assert (lw < 0.5e-6) if fallback else (lw > 1.999e-6), (c.name, lw)   # (sin 2e-6 is a hair under 2e-6)
        g = sc.finger_geom(0, 4)
        (cb, Rb), hs = sc.fk_geoms(sc.q0)[g], sc.gsize[g]
        for part, lo, hi, inside in (("4e-13 off", 2e-13, 1e-12 / 2, False), ("2e-12 off", 2e-12 / 1.01, 4e-12, False),
                                     ("1e-9 under", 0.5e-9, 2e-9, True), ("inside a segment", 0.5e-3, 2e-3, True)):
            _, c = case_named(t, "sphere centre " + part)
            l = Rb.T @ (c.c - cb)
            out = np.abs(l) - hs
            assert bool(np.all(out <= 0)) == inside, c.name
            d = -out.max() if inside else np.linalg.norm(np.maximum(out, 0.0))
            assert lo <= d <= hi, (c.name, d)
        # the shallow and the clear MPR cases sit at twice the collider's tolerance and ten times it
        assert sc.m.mpr_tolerance == 1e-6
        # more than four corners below the ground: the kept four are the first in index order
        for part, nbelow in (("box sunk, 8", 8), ("box sunk upside", 8), ("box sunk and tilted", 6)):
            _, c = case_named(t, part)
            assert sum(v[2] < 0 for v in cc.box_vertices(c.c, c.R, c.osize)) == nbelow, c.name


DISPATCH = {"default": None, "duo": "1", "one-wave": "0"}


def make_env(gm, t, duo):
    old = os.environ.get("GM_DUO")
    if duo is None:
        os.environ.pop("GM_DUO", None)
    else:
        os.environ["GM_DUO"] = duo
    try:
        return gm.BatchedGripperEnv(len(t.cases), settings=t.sc.settings, seed=3, model_blob=t.sc.model, objects=t.objs)
    finally:
        if old is None:
            os.environ.pop("GM_DUO", None)
        else:
            os.environ["GM_DUO"] = old


@pytest.mark.gpu
@pytest.mark.parametrize("dispatch", list(DISPATCH))
@pytest.mark.parametrize("n_seg", [8, 10])
def test_device_matches_oracle_and_closed_form(gm, tables, n_seg, dispatch):
    if not gpu_available():
        pytest.skip("no GPU")
    t = tables(n_seg)
    sc = t.sc
    env = make_env(gm, t, DISPATCH[dispatch])
    try:
        if DISPATCH[dispatch] is not None:
            assert env.dispatch_info()["waves_per_env"] == (2 if dispatch == "duo" else 1)
        env.set_env_states(t.recs)
        ncon, con, efc, qacc, nefc, _ = env.debug_substep(full=True)
        after = env.env_states()
    finally:
        env.close()
    dv, ov = gm.env_state_view(after), gm.env_state_view(t.after)
    nv = sc.nv
    rep_o, rep_c, rep_f = {}, {}, {}
    # every figure is measured (and printed) before anything is asserted
    for i, c in enumerate(t.cases):
        n = min(int(ncon[i]), int(t.ncon[i]))
        g = float(np.abs(con[i, :n, :13] - t.con[i, :n, :13]).max(initial=0.0))
        fs = max(1.0, float(np.abs(t.efc[i]).max()))
        qs = max(1.0, float(np.abs(t.qacc[i]).max()))
        f = max(float(np.abs(efc[i] - t.efc[i]).max()) / fs, float(np.abs(qacc[i, :nv] - t.qacc[i, :nv]).max()) / qs)
        rep_o[c.family] = max(rep_o.get(c.family, 0.0), g)
        rep_f[c.family] = max(rep_f.get(c.family, 0.0), f)
    print(f"\nN = {n_seg}, {dispatch}: worst |device - oracle| per family, contact geometry {rep_o}, "
          f"scaled efc_force / qacc {rep_f}")
    for i, c in enumerate(t.cases):
        who = f"{c.name} ({dispatch}, N = {n_seg})"
        assert ncon[i] == t.ncon[i] and nefc[i] == t.nefc[i], f"{who}: ncon {ncon[i]} / {t.ncon[i]}, nefc {nefc[i]} / {t.nefc[i]}"
        n = int(ncon[i])
        np.testing.assert_array_equal(con[i, :, 13:15], t.con[i, :, 13:15], err_msg=f"{who}: contact pair ids")
        for k in range(n):
            tol = 1e-9 if is_mpr_pair(sc, c, int(con[i, k, 13]), int(con[i, k, 14])) else 1e-12
            np.testing.assert_allclose(con[i, k, :13], t.con[i, k, :13], rtol=0, atol=tol, err_msg=f"{who}: contact {k}")
        np.testing.assert_array_equal(con[i, :, 15], t.con[i, :, 15], err_msg=f"{who}: friction")
        np.testing.assert_array_equal(con[i, n:], 0.0, err_msg=f"{who}: rows past ncon")
        tol = 1e-7 if c.capacity else 1e-10
        fs = max(1.0, float(np.abs(t.efc[i]).max()))
        np.testing.assert_allclose(efc[i] / fs, t.efc[i] / fs, rtol=0, atol=tol, err_msg=f"{who}: efc_force")
        qs = max(1.0, float(np.abs(t.qacc[i]).max()))
        np.testing.assert_allclose(qacc[i, :nv] / qs, t.qacc[i, :nv] / qs, rtol=0, atol=tol, err_msg=f"{who}: qacc")
        np.testing.assert_allclose(dv["qpos"][i], ov["qpos"][i], rtol=0, atol=1e-9, err_msg=f"{who}: qpos after the substep")
        assert dv["newton_caps"][i] == ov["newton_caps"][i], f"{who}: newton_caps"
        if c.kind == cc.CLOSED:
            w = against_closed_form(sc, c, n, con[i], "device, " + dispatch)
            rep_c[c.family] = float(max(rep_c.get(c.family, 0.0), w))
    print(f"N = {n_seg}, {dispatch}: worst |device - closed form| per family {rep_c}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_seg", [8, 10])
def test_duo_env_step_from_crafted_states_equals_one_wave(gm, tables, n_seg):
    """One env-step (every substep's collider on the DUO helper wave, with its own hit
    slots) from the crafted records equals the one-wave kernel's bit for bit, the capacity
    and second-batch states included; the first substep of each is the state the substep
    test pins to the oracle."""
    if not gpu_available():
        pytest.skip("no GPU")
    t = tables(n_seg)
    a, b = make_env(gm, t, "1"), make_env(gm, t, "0")
    try:
        assert a.dispatch_info()["waves_per_env"] == 2 and b.dispatch_info()["waves_per_env"] == 1
        act = np.zeros((len(t.cases), a.n_actions), dtype=np.float32)
        outs = []
        for e in (a, b):
            e.set_env_states(t.recs)
            obs, rew, done, _ = e.step(act)
            outs.append((obs.copy(), np.asarray(rew).copy(), np.asarray(done).copy(), e.env_states()))
        (oa, ra, da, sa), (ob, rb, db, sb) = outs
        np.testing.assert_array_equal(oa, ob, err_msg="observations")
        np.testing.assert_array_equal(ra, rb, err_msg="rewards")
        np.testing.assert_array_equal(da, db, err_msg="done flags")
        va, vb = gm.env_state_view(sa), gm.env_state_view(sb)
        for f in va.dtype.names:
            np.testing.assert_array_equal(va[f], vb[f], err_msg=f)
        # the states moved (the step ran) and stayed finite where the contact was ordinary
        v0 = gm.env_state_view(t.recs)
        assert (va["time"] > v0["time"]).all()
        ordinary = [i for i, c in enumerate(t.cases) if not c.capacity]
        assert np.isfinite(va["qpos"][ordinary]).all()
    finally:
        a.close()
        b.close()
