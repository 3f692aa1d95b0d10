"""The constraint rows, the Newton optimum and mj_Euler on crafted states against an
independent model (tests/constraint_model.py, tests/constraint_cases.py).

Every other test of the constraint stage compares the device with oracle/physics.c, which
restates the device's rows and solver operation for operation.  Here both are compared with
a numpy model written from DESIGN section 2 and MuJoCo's documented formulas:

CPU (oracle against model)
1  body_invweight0 / dof_invweight0 of the compiled model against H~^-1 at qpos0, N = 5, 8, 10;
2  rows: lambda_model(qacc) = max(0, -D (J qacc - aref)) at the oracle's qacc against the
   oracle's efc_force, row by row, locks folded (no solve: any single-row error shows);
3  optimum: the oracle's qacc and efc_force against the model's qacc* and lambda*;
4  warm-start invariance of the oracle's answer;
5  mj_Euler: qvel' and qpos' from the model's formula with the oracle's own efc_force
   (capped solves included, the free joint's quaternion on spinning objects);
6  the conditions that keep the table from being vacuous.
GPU: the same records through one debug substep per batch, 2, 3 and 5 for the device
against the model (built from the device's own contact list), the device against the oracle
at compare_substep's bounds, warm-start invariance on the device, one env-step on DUO
workgroups bit-equal to the one-wave kernel's from the (b), (c), (d) records, and
decoupled first points counted on the (b) records with a converged warm start.

Bounds.  Nothing is taken from what the device or the oracle achieves: for each quantity
and family the model is evaluated in float64 and in longdouble on the same cases, the worst
difference is the float64 floor of that family, and the bound is 100 x the floor, never
below 1e-13 (two backward-stable fp64 algorithms with different operation order summing up
to 170 terms differ by a modest multiple of the floor; the modelling errors this test
exists for move forces by 1e-3 or more).  A bound above 1e-8 fails: such a family is too
ill-conditioned to test anything.  Forces and accelerations are scaled by max(1, |x|.max())
per env, velocities likewise, positions are absolute.  Without an 80-bit longdouble the
bound is 1e-9.

Measured figures: DESIGN.md section 4, "The constraint stage on crafted states".
"""
import os

import numpy as np
import pytest

import constraint_cases as ccs
import constraint_model as cm
import indep_physics as ip
from conftest import gpu_available

QUANT = ("rows", "qacc", "lambda", "qvel", "qpos")
FAMILIES = ("a", "b", "c", "d", "e", "f")
FACTOR, BOUND_MIN, BOUND_MAX, BOUND_NO_LD = 100.0, 1e-13, 1e-8, 1e-9
REF = cm.LD if cm.HAVE_LONGDOUBLE else cm.F64


_iw = {}


def body_iw(sc, obj):
    """Translational invweight0 per body from the model itself (cm.invweights at qpos0, the
    centre-of-mass Jacobian; the blob's values are compared with these in a test of their
    own), the live object's 1 / mass."""
    if id(sc) not in _iw:
        _iw[id(sc)] = np.asarray(cm.invweights(sc.M, cm.F64)[1], dtype=np.float64)
    biw = _iw[id(sc)].copy()
    biw[sc.m.body_obj] = 1.0 / float(obj.mass)
    return biw


# Disagreements left unresolved (the issue's rule: a strict xfail that names the row and the
# size, never a wider bound): (record, quantities, measured / bound) per source.  Each entry is
# one strict xfail of its own (test_*_known_disagreement); the main tests hold these figures
# to BOUND_MAX and every other figure of every record to its bound.  All are rounding in how
# the engine carries a solve that starts from the warm start of norm 1e3 |qacc|, or forms
# mj_Euler's right-hand side; none is a modelling error:
# - at a converged solve the engine integrates H~ qacc in place of qfrc_smooth + J^T efc
#   (equal at the optimum), so qvel' inherits the Newton point's own rounding; on the box
#   under the stiff clamped solref (forces four times larger) that is 1.9 x the bound;
# - at a capped solve efc_force is the line search's running J a - aref and the residual
#   H~ q - (qfrc_smooth + J^T efc) uses the running H~ q, both carried from the warm start:
#   from norm 1e3 |qacc| their rounding (1e-16 x 1e3 |H~ qacc|) is what is left in the rows,
#   in qvel' and in qpos'.  The capped records from the negated warm start (norm |qacc|)
#   run the same paths and hold every bound.
SOLREF_BOX = "box on the ground, at rest, N = 8, 0.7 mm deep [solref (0.004, 0.7)]"
R1 = "; warm start random x 1e3 [newton_maxit 1]"
R2 = "; warm start random x 1e3 [newton_maxit 2]"
KNOWN_OVER = {
    "oracle": [
        (SOLREF_BOX, ("qvel",), "qvel' 5.4e-12 / 2.9e-12"),
        ("sphere on the ground, sliding askew, N = 8" + R1, ("rows",), "rows 1.3e-12 / 9.0e-13"),
        ("sphere on the ground, lifting while sliding, N = 8" + R1, ("rows", "qvel"), "rows 2.1e-11 / 9.0e-13, qvel' 1.6e-11 / 3.3e-12"),
        ("box on the ground, at rest, N = 8" + R1, ("rows",), "rows 3.0e-12 / 9.0e-13"),
        ("cylinder on its rim on the ground, at rest, N = 8" + R1, ("rows",), "rows 6.5e-12 / 9.0e-13"),
        ("cylinder on its rim on the ground, sliding askew, N = 8" + R1, ("rows", "qvel"), "rows 9.5e-12 / 9.0e-13, qvel' 7.1e-12 / 3.3e-12"),
        ("grasp: object 1, env-step 24" + R1, ("rows",), "rows 3.2e-12 / 9.0e-13"),
        ("grasp: object 1, env-step 32" + R1, ("rows",), "rows 1.5e-12 / 9.0e-13"),
        ("grasp: object 1, env-step 40" + R1, ("rows",), "rows 1.4e-12 / 9.0e-13"),
        ("grasp: object 1, env-step 47" + R1, ("rows", "qvel"), "rows 1.6e-10 / 9.0e-13, qvel' 2.4e-11 / 3.3e-12"),
        ("cylinder on its rim on the ground, lifting while sliding, N = 8" + R2, ("rows",), "rows 1.0e-11 / 9.0e-13"),
        ("grasp: object 1, env-step 24" + R2, ("rows", "qvel"), "rows 9.3e-13 / 9.0e-13, qvel' 7.0e-12 / 3.3e-12"),
        ("grasp: object 1, env-step 32" + R2, ("rows",), "rows 1.5e-12 / 9.0e-13"),
        ("grasp: object 1, env-step 40" + R2, ("qvel",), "qvel' 8.7e-12 / 3.3e-12"),
        ("grasp: object 1, env-step 47" + R2, ("rows", "qvel"), "rows 9.1e-13 / 9.0e-13, qvel' 2.4e-11 / 3.3e-12"),
    ],
    "device": [
        (SOLREF_BOX, ("qvel",), "qvel' 5.0e-12 / 2.9e-12"),
        ("sphere on the ground, lifting while sliding, N = 8" + R1, ("rows", "qvel"), "rows 1.1e-11 / 9.0e-13, qvel' 9.6e-12 / 3.3e-12"),
        ("box on the ground, at rest, N = 8" + R1, ("rows",), "rows 3.0e-12 / 9.0e-13"),
        ("cylinder on its rim on the ground, at rest, N = 8" + R1, ("rows",), "rows 2.8e-12 / 9.0e-13"),
        ("cylinder on its rim on the ground, sliding askew, N = 8" + R1, ("rows", "qvel"), "rows 5.9e-12 / 9.0e-13, qvel' 3.8e-12 / 3.3e-12"),
        ("cylinder on its rim on the ground, lifting while sliding, N = 8" + R1, ("qvel",), "qvel' 5.0e-12 / 3.3e-12"),
        ("grasp: object 1, env-step 24" + R1, ("rows",), "rows 3.2e-12 / 9.0e-13"),
        ("grasp: object 1, env-step 40" + R1, ("rows",), "rows 1.4e-12 / 9.0e-13"),
        ("grasp: object 1, env-step 47" + R1, ("rows", "qvel"), "rows 1.6e-10 / 9.0e-13, qvel' 2.7e-11 / 3.3e-12"),
        ("cylinder on its rim on the ground, lifting while sliding, N = 8" + R2, ("rows",), "rows 3.7e-12 / 9.0e-13"),
        ("grasp: object 1, env-step 24" + R2, ("rows", "qvel"), "rows 9.4e-13 / 9.0e-13, qvel' 5.5e-12 / 3.3e-12"),
        ("grasp: object 1, env-step 40" + R2, ("qvel",), "qvel' 9.0e-12 / 3.3e-12"),
        ("grasp: object 1, env-step 47" + R2, ("rows", "qvel"), "rows 9.1e-13 / 9.0e-13, qvel' 2.7e-11 / 3.3e-12"),
    ],
}


def known_over(who, q, item):
    return any(item.name == kn and q in kq for kn, kq, _ in KNOWN_OVER[who])


def check_known(t, rows, who, name, quantities):
    """The named figures of one record against the issue's bound (all must hold for the
    xfail to be lifted)."""
    hit = [(b, k, err) for b, k, err in rows if b.items[k].name == name]
    assert len(hit) == 1, name
    b, k, err = hit[0]
    for q in quantities:
        print(f"{who}, {name}: {q} {err[q]:.2e}, bound {t.bound(q, b.items[k].family):.2e}")
    assert all(err[q] <= t.bound(q, b.items[k].family) for q in quantities)


def no_longdouble_note():
    if not cm.HAVE_LONGDOUBLE:
        pytest.skip(f"no 80-bit longdouble here: the asserts ran at {BOUND_NO_LD:g} instead of 100 x the float64 floor")


class Solved:
    """The model of one state in one dtype: the problem and its optimum."""

    def __init__(self, sc, item, rec, contacts, dtype):
        M = ip.Model(sc.model)
        ip.set_object(M, item.obj)
        self.M = M
        self.P = cm.build(M, rec, contacts, body_iw(sc, item.obj), sc.m.timestep, dtype)
        self.qacc, self.lam, self.iters, self.ls = cm.solve(self.P)
        self.efc = cm.folded(self.P, self.lam)


def scaled(d, ref):
    return float(np.abs(np.asarray(d, dtype=REF)).max(initial=0.0) / max(1.0, float(np.abs(ref).max(initial=0.0))))


def euler_expected(sc, S, efc):
    """(qvel', qpos') of the model; update_all's antiroll rule (an object slower than 1e-6
    m/s is stopped after the integration) applied to the velocity, as the engine's state
    after a substep carries it."""
    v1, q1 = cm.euler(S.M, S.P, efc)
    d0 = sc.m.dof_obj
    if float(np.sqrt(np.sum(v1[d0:d0 + 3] ** 2))) < 1e-6:
        v1 = v1.copy()
        v1[d0:d0 + 6] = 0
    return v1, q1


class Table:
    def __init__(self, gm):
        self.gm = gm
        self.batches = ccs.build_table(gm)
        self.cache = {}
        self.floors = {q: {f: 0.0 for f in FAMILIES} for q in QUANT}
        self.oracle_err = {q: {f: 0.0 for f in FAMILIES} for q in QUANT}
        self.rows = []                                    # (batch, k, errors) of the oracle
        for b in self.batches:
            for k, it in enumerate(b.items):
                err, floor = self.compare(b, k, b.ncon, b.con, b.efc, b.qacc, b.after, with_floor=True)
                self.rows.append((b, k, err))
                for q in err:
                    self.oracle_err[q][it.family] = max(self.oracle_err[q][it.family], err[q])
                    self.floors[q][it.family] = max(self.floors[q][it.family], floor[q])

    def solved(self, b, k, ncon, con, dtype):
        """Warm starts and caps of one state share its problem (neither enters it); the key is
        the state's own bytes that do: the record without qacc_warm, and the contact list."""
        it = b.items[k]
        n = int(ncon[k])
        rec = np.array(b.recs[k], copy=True)
        self.gm.env_state_view(rec)["qacc_warm"][...] = 0
        consts = tuple(b.sc.m.solimp[:]) + tuple(b.sc.m.solref[:])
        key = (b.n_seg, consts, rec.tobytes(), con[k, :n].tobytes(), bytes(it.obj), np.dtype(dtype).name)
        if key not in self.cache:
            self.cache[key] = Solved(b.sc, it, self.gm.env_state_view(b.recs[k]), b.contacts(k, ncon, con), dtype)
        return self.cache[key]

    def compare(self, b, k, ncon, con, efc, qacc, after, with_floor=False):
        """Errors of one source (oracle or device arrays of batch b) on item k against the
        model in the reference dtype, and the model's own float64 floor of the same case: the
        whole model run in float64 against the whole model run in longdouble (rows: both at
        the source's qacc; qvel', qpos': each with its own lambda*)."""
        sc, it = b.sc, b.items[k]
        nv, nq = sc.nv, sc.nq
        R = self.solved(b, k, ncon, con, REF)
        nrow = len(R.P.fold)
        assert nrow == int(b.nl[k]) + 4 * int(ncon[k])
        e, a = efc[k, :nrow], qacc[k, :nv]
        assert not efc[k, nrow:].any()
        av = self.gm.env_state_view(after)[k]
        capped = it.family == "f"

        def figures(S, forces):
            rows = cm.folded(S.P, cm.forces_at(S.P, a))
            v1, q1 = euler_expected(sc, S, forces)
            return dict(rows=rows, qacc=S.qacc, **{"lambda": S.efc}, qvel=v1, qpos=q1)
        ref = figures(R, e)
        fs = ref["lambda"] if not capped else e
        err = dict(rows=scaled(ref["rows"] - e, fs), qvel=scaled(ref["qvel"] - av["qvel"][:nv], ref["qvel"]),
                   qpos=float(np.abs(ref["qpos"] - av["qpos"][:nq]).max()))
        if not capped:          # a capped solve is not at the optimum: 3 does not apply, 5 must hold
            err["qacc"] = scaled(ref["qacc"] - a, ref["qacc"])
            err["lambda"] = scaled(ref["lambda"] - e, fs)
        floor = None
        if with_floor:
            if cm.HAVE_LONGDOUBLE:
                L = self.solved(b, k, ncon, con, cm.F64)
                lo, hi = figures(L, L.efc), figures(R, R.efc)
                floor = dict(rows=scaled(ref["rows"] - lo["rows"], fs), qacc=scaled(ref["qacc"] - lo["qacc"], ref["qacc"]),
                             **{"lambda": scaled(ref["lambda"] - lo["lambda"], ref["lambda"])},
                             qvel=scaled(hi["qvel"] - lo["qvel"], hi["qvel"]),
                             qpos=float(np.abs(hi["qpos"] - lo["qpos"]).max()))
            else:
                floor = {q: BOUND_NO_LD / FACTOR for q in QUANT}
        return err, floor

    def bound(self, q, family):
        if not cm.HAVE_LONGDOUBLE:
            return BOUND_NO_LD
        return max(FACTOR * self.floors[q][family], BOUND_MIN)

    def report(self, who, errs):
        for q in QUANT:
            print(f"{who} {q:7s} " + "  ".join(f"{f}: {errs[q][f]:.2e}" for f in FAMILIES))


_table = {}


def get_table(gm):
    if "t" not in _table:
        _table["t"] = Table(gm)
    return _table["t"]


@pytest.fixture(scope="module")
def table(gm):
    return get_table(gm)


# ================================================================ CPU
@pytest.mark.parametrize("n_seg", [5, 8, 10])
def test_invweight0_of_the_compiled_model(gm, n_seg):
    """mj_setConst: body_invweight0[b][0] = trace(J_b H~^-1 J_b^T) / 3 with the translational
    Jacobian of the body's centre of mass (mj_jacBodyCom), dof_invweight0 = diag(H~^-1), at
    qpos0.  Relative 1e-10: H~ at qpos0 has a condition number near 1e7."""
    sc = ccs.scene(gm, n_seg)
    M = sc.M
    org, com, dof = cm.invweights(M, REF)
    blob_b = ip.arr(M.raw.body_invweight0, ip.GM_MAX_BODY, 2)[:M.nbody, 0].astype(np.float64)
    blob_d = ip.arr(M.raw.dof_invweight0).astype(np.float64)[:M.nv]
    eb = np.abs(com - blob_b)[1:] / np.abs(com)[1:]
    ed = np.abs(dof - blob_d) / np.abs(dof)
    print(f"\nN = {n_seg}: body_invweight0 worst rel {float(eb.max()):.2e}, dof_invweight0 worst rel {float(ed.max()):.2e}; "
          f"at the frame origin instead: {float((np.abs(org - blob_b)[1:] / np.abs(org)[1:]).max()):.2e}")
    assert blob_b[0] == 0.0
    assert eb.max() <= 1e-10 and ed.max() <= 1e-10
    # the locks' and the contacts' regulariser really differ between bodies
    assert blob_b[1:].max() > 10 * blob_b[1:].min()


def test_table_conditions(gm, table):
    """The table reaches what it was crafted for (asserted, not measured)."""
    t = table
    multi = ls = b_ls = 0
    edges = {0: 0, 1: 0, 2: 0, 3: 0, 4: 0}
    n_items = 0
    fam = {f: 0 for f in FAMILIES}
    lock_components = set()
    for b in t.batches:
        for k, it in enumerate(b.items):
            n_items += 1
            fam[it.family] += 1
            multi += b.iters[k] >= 2
            ls += b.ls_evals[k] >= 1
            b_ls += b.ls_evals[k] >= 1 and (it.family == "b" or (it.base is not None and it.base.family == "b"))
            assert bool(b.capped[k]) == (it.family == "f"), f"{it.name}: newton_caps"
            assert not b.overflow[k] or it.may_overflow, f"{it.name}: overflow"
            assert np.isfinite(b.qacc[k]).all() and np.isfinite(b.efc[k]).all(), it.name
            if it.family != "f":
                for c in range(int(b.ncon[k])):
                    base = int(b.nl[k]) + 4 * c
                    edges[int((b.efc[k, base:base + 4] > 0).sum())] += 1
            if it.family == "d":
                S = t.solved(b, k, b.ncon, b.con, REF)
                for terms in S.P.fold[:int(b.nl[k])]:
                    lock_components.add(len(terms))
    print(f"\n{n_items} records in {len(t.batches)} batches, per family {fam}; >= 2 Newton iterations: {multi}, "
          f"line searches: {ls} ({b_ls} on (b) states); contacts by active edges {edges}; lock rows per lock {lock_components}")
    assert multi >= 12 and ls >= 8 and b_ls >= 4
    assert all(edges[n] >= 1 for n in (0, 1, 2, 4)), edges
    assert fam["f"] >= 8 and all(fam[f] > 0 for f in FAMILIES)
    f_warm = [it.warm for b in t.batches for it in b.items if it.family == "f"]
    print(f"capped records by warm start: {dict((w, f_warm.count(w)) for w in ccs.WARM[2:])}")
    assert f_warm.count(ccs.WARM[2]) >= 8, "too few capped solves outside the known disagreement"
    assert any(b.nefc.max() == 132 for b in t.batches)
    mus = np.concatenate([b.con[k, :b.ncon[k], 15] for b in t.batches for k in range(len(b.items))])
    assert (mus == 1.0).any() and (mus == 1.7).sum() >= 10, "no contact with mu != 1"
    assert {1} < lock_components, "no lock with one world component and one with several"
    # every record took part in every comparison that applies to it
    assert len(t.rows) == n_items
    assert all(set(err) == (set(QUANT) if b.items[k].family != "f" else {"rows", "qvel", "qpos"}) for b, k, err in t.rows)
    # every variant's constants reach the branch they are there for
    depths = {}
    for b in t.batches:
        if b.items[0].family == "e":
            d = np.concatenate([-b.con[k, :b.ncon[k], 0] for k in range(len(b.items))]) / ccs.WIDTH
            depths[b.variant] = d
            mid = b.sc.m.solimp[3]
            assert (d < mid).any() and ((d > mid) & (d < 1)).any() and (d > 1).any(), (b.variant, np.sort(d))
    assert set(depths) == set(ccs.E_VARIANTS)
    assert 2 * ccs.scene(gm, 8).m.timestep > 0.004      # the solref variant's time constant is clamped


def test_oracle_matches_the_model(table):
    """2, 3 and 5 for the oracle, every record, per family at 100 x the model's own float64
    floor."""
    t = table
    print()
    t.report("floor (model f64 - longdouble)", t.floors)
    t.report("oracle - model                ", t.oracle_err)
    print("bounds: " + "; ".join(f"{q} " + " ".join(f"{f} {t.bound(q, f):.1e}" for f in FAMILIES) for q in QUANT))
    for q in QUANT:
        for f in FAMILIES:
            assert t.bound(q, f) <= BOUND_MAX, f"{q}, family {f}: bound {t.bound(q, f):.2e}: too ill-conditioned to test"
    bad = [(b.items[k].name, q, e, t.bound(q, b.items[k].family)) for b, k, err in t.rows for q, e in err.items()
           if not e <= (BOUND_MAX if known_over("oracle", q, b.items[k]) else t.bound(q, b.items[k].family))]
    for x in bad:
        print("OVER", x)
    assert not bad, f"{len(bad)} figures over their bound, first: {bad[:5]}"
    no_longdouble_note()


@pytest.mark.xfail(strict=True, reason="rounding of the engine's running products from the 1e3 |qacc| warm start / of its "
                                       "H~ qacc right-hand side of mj_Euler: over 100 x the float64 floor, see KNOWN_OVER")
@pytest.mark.parametrize("name,quantities,size", KNOWN_OVER["oracle"])
def test_oracle_known_disagreement(table, name, quantities, size):
    check_known(table, table.rows, "oracle", name, quantities)


@pytest.mark.xfail(strict=True, reason="follow-up: MuJoCo's mj_makeImpedance is remembered to give a pyramid edge the regulariser "
                                       "2 mu^2 R (Rpy); DESIGN section 2, the engine and the model's default use R.  MuJoCo's "
                                       "source is not at hand to confirm; rows of the (b) records then differ by up to ~0.5 of "
                                       "their scale")
def test_pyramid_edges_carry_the_2_mu2_regulariser(gm, table):
    """The rows check (2) on the ground records with the model's contact rows regularised by
    2 mu^2 R.  Fails today for every such record, at friction 1 and at friction 1.7: whether
    the engine or this expectation is wrong is to be settled against MuJoCo's source."""
    t, worst, n = table, 0.0, 0
    for b in t.batches:
        for k, it in enumerate(b.items):
            if it.family != "b":
                continue
            M = ip.Model(b.sc.model)
            ip.set_object(M, it.obj)
            P = cm.build(M, gm.env_state_view(b.recs[k]), b.contacts(k), body_iw(b.sc, it.obj), b.sc.m.timestep, REF,
                         pyramid_rpy=True)
            e = b.efc[k, :len(P.fold)]
            worst = max(worst, scaled(cm.folded(P, cm.forces_at(P, b.qacc[k])) - e, e))
            n += 1
    print(f"\nrows with Rpy = 2 mu^2 R on {n} ground records: worst {worst:.2e}")
    assert n >= 20 and worst <= t.bound("rows", "b")


def test_oracle_answer_does_not_depend_on_the_warm_start(table):
    t = table
    worst, groups = {"qacc": 0.0, "lambda": 0.0}, 0
    for b in t.batches:
        by_base = {}
        for k, it in enumerate(b.items):
            if it.family == "c":
                by_base.setdefault(id(it.base), []).append(k)
        for ks in by_base.values():
            assert len(ks) == len(ccs.WARM)
            groups += 1
            for k in ks[1:]:
                worst["qacc"] = max(worst["qacc"], scaled(b.qacc[k] - b.qacc[ks[0]], b.qacc[ks[0]]))
                worst["lambda"] = max(worst["lambda"], scaled(b.efc[k] - b.efc[ks[0]], b.efc[ks[0]]))
    print(f"\n{groups} states x {len(ccs.WARM)} warm starts: worst spread of the oracle's answer {worst}")
    assert groups >= 16
    assert worst["qacc"] <= t.bound("qacc", "c") and worst["lambda"] <= t.bound("lambda", "c")
    no_longdouble_note()


# ================================================================ GPU
def make_env(gm, b, duo=None):
    old = os.environ.get("GM_DUO")
    if duo is None:
        os.environ.pop("GM_DUO", None)
    else:
        os.environ["GM_DUO"] = duo
    try:
        return gm.BatchedGripperEnv(len(b.items), settings=b.sc.settings, seed=3, model_blob=b.sc.model, objects=b.objs)
    finally:
        if old is None:
            os.environ.pop("GM_DUO", None)
        else:
            os.environ["GM_DUO"] = old


_device = {}


def device_substep(gm, t, bi):
    if bi not in _device:
        b = t.batches[bi]
        env = make_env(gm, b)
        try:
            env.set_env_states(b.recs)
            ncon, con, efc, qacc, nefc, _ = env.debug_substep(full=True)
            after = env.env_states()
        finally:
            env.close()
        _device[bi] = (ncon, con, efc, qacc[:, :b.sc.nv], nefc, after)
    return _device[bi]


GROUPS = {
    "N = 8, default model": lambda b: b.n_seg == 8 and b.variant == "default",
    "N = 5 and 10": lambda b: b.n_seg != 8,
    "solimp and solref variants": lambda b: b.variant in ccs.E_VARIANTS,
    "capped solves": lambda b: b.variant.startswith("newton_maxit"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_device_matches_the_model_and_the_oracle(gm, group):
    if not gpu_available():
        pytest.skip("no GPU")
    t = get_table(gm)
    picked = [bi for bi, b in enumerate(t.batches) if GROUPS[group](b)]
    assert picked
    dev_err = {q: {f: 0.0 for f in FAMILIES} for q in QUANT}
    vs_oracle = {"efc": 0.0, "qacc": 0.0, "qpos": 0.0}
    checks = []
    for bi in picked:
        b = t.batches[bi]
        ncon, con, efc, qacc, nefc, after = device_substep(gm, t, bi)
        gv = gm.env_state_view(after)
        ov = gm.env_state_view(b.after)
        for k, it in enumerate(b.items):
            who = f"{it.name} ({group})"
            assert ncon[k] == b.ncon[k] and nefc[k] == b.nefc[k], who
            np.testing.assert_array_equal(con[k, :, 13:15], b.con[k, :, 13:15], err_msg=who)
            err, _ = t.compare(b, k, ncon, con, efc, qacc, after)
            for q, e in err.items():
                dev_err[q][it.family] = max(dev_err[q][it.family], e)
                checks.append((it.name, q, e, BOUND_MAX if known_over("device", q, it) else t.bound(q, it.family)))
            # the device against the oracle at compare_substep's bounds (tests/test_grasp_parity.py)
            fs = max(1.0, float(np.abs(b.efc[k]).max()))
            qs = max(1.0, float(np.abs(b.qacc[k]).max()))
            o = dict(efc=float(np.abs(efc[k] - b.efc[k]).max()) / fs, qacc=float(np.abs(qacc[k] - b.qacc[k]).max()) / qs,
                     qpos=float(np.abs(gv["qpos"][k] - ov["qpos"][k]).max()))
            for q in o:
                vs_oracle[q] = max(vs_oracle[q], o[q])
            checks.append((who, "efc vs oracle", o["efc"], 1e-7))
            checks.append((who, "qacc vs oracle", o["qacc"], 1e-7))
            checks.append((who, "qpos vs oracle", o["qpos"], 1e-9))
            checks.append((who, "contact geometry vs oracle", float(np.abs(con[k, :, :13] - b.con[k, :, :13]).max()), 1e-9))
            assert gv["newton_caps"][k] == ov["newton_caps"][k], who
    print(f"\n{group}: {len(picked)} batches")
    t.report("device - model", dev_err)
    print(f"device - oracle: {vs_oracle}")
    bad = [c for c in checks if not c[2] <= c[3]]
    for x in bad:
        print("OVER", x)
    assert not bad, f"{len(bad)} figures over their bound, first: {bad[:5]}"
    no_longdouble_note()


@pytest.mark.gpu
@pytest.mark.xfail(strict=True, reason="rounding of the engine's running products from the 1e3 |qacc| warm start / of its "
                                       "H~ qacc right-hand side of mj_Euler: over 100 x the float64 floor, see KNOWN_OVER")
@pytest.mark.parametrize("name,quantities,size", KNOWN_OVER["device"])
def test_device_known_disagreement(gm, name, quantities, size):
    if not gpu_available():
        pytest.skip("no GPU")
    t = get_table(gm)
    for bi, b in enumerate(t.batches):
        ks = [k for k, it in enumerate(b.items) if it.name == name]
        if ks:
            ncon, con, efc, qacc, nefc, after = device_substep(gm, t, bi)
            check_known(t, [(b, ks[0], t.compare(b, ks[0], ncon, con, efc, qacc, after)[0])], "device", name, quantities)
            return
    raise AssertionError(f"no record named {name}")


@pytest.mark.gpu
def test_device_answer_does_not_depend_on_the_warm_start(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    t = get_table(gm)
    worst, groups = {"qacc": 0.0, "lambda": 0.0}, 0
    for bi, b in enumerate(t.batches):
        if not any(it.family == "c" for it in b.items):
            continue
        _, _, efc, qacc, _, _ = device_substep(gm, t, bi)
        by_base = {}
        for k, it in enumerate(b.items):
            if it.family == "c":
                by_base.setdefault(id(it.base), []).append(k)
        for ks in by_base.values():
            groups += 1
            for k in ks[1:]:
                worst["qacc"] = max(worst["qacc"], scaled(qacc[k] - qacc[ks[0]], qacc[ks[0]]))
                worst["lambda"] = max(worst["lambda"], scaled(efc[k] - efc[ks[0]], efc[ks[0]]))
    print(f"\n{groups} states x {len(ccs.WARM)} warm starts: worst spread of the device's answer {worst}")
    assert groups >= 16
    assert worst["qacc"] <= t.bound("qacc", "c") and worst["lambda"] <= t.bound("lambda", "c")


@pytest.mark.gpu
def test_duo_env_step_from_constraint_states_equals_one_wave(gm):
    """debug_substep always runs the one-wave kernel; the rows the DUO helper wave forms
    (duo_rows) are covered by one env-step from the (b), (c), (d) records on DUO workgroups,
    bit-equal to the one-wave kernel's."""
    if not gpu_available():
        pytest.skip("no GPU")
    ran = 0
    for b in get_table(gm).batches:
        if b.variant != "default" or not any(it.family in "bcd" for it in b.items):
            continue
        a, c = make_env(gm, b, "1"), make_env(gm, b, "0")
        try:
            assert a.dispatch_info()["waves_per_env"] == 2 and c.dispatch_info()["waves_per_env"] == 1
            act = np.zeros((len(b.items), a.n_actions), dtype=np.float32)
            outs = []
            for e in (a, c):
                e.set_env_states(b.recs)
                obs, rew, done, _ = e.step(act)
                outs.append((obs.copy(), np.asarray(rew).copy(), np.asarray(done).copy(), e.env_states()))
            (oa, ra, da, sa), (ob, rb, db, sb) = outs
            np.testing.assert_array_equal(oa, ob, err_msg="observations")
            np.testing.assert_array_equal(ra, rb, err_msg="rewards")
            np.testing.assert_array_equal(da, db, err_msg="done flags")
            va, vb = gm.env_state_view(sa), gm.env_state_view(sb)
            for f in va.dtype.names:
                np.testing.assert_array_equal(va[f], vb[f], err_msg=f)
            assert (va["time"] > gm.env_state_view(b.recs)["time"]).all()
            ran += 1
        finally:
            a.close()
            c.close()
    assert ran >= 3


@pytest.mark.gpu
def test_ground_states_with_a_converged_warm_start_take_the_decoupled_point(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    picked = [it for b in get_table(gm).batches for it in b.items
              if it.family == "c" and it.warm == "converged" and it.base.family == "b" and it.n_seg == 8]
    assert len(picked) >= 12
    b = ccs.Batch(gm, picked)
    env = make_env(gm, b, "0")
    try:
        env.set_env_states(b.recs)
        env.set_action(np.zeros((len(picked), env.n_actions), dtype=np.float32))
        env.step_profiled()
        taken = env.decoupled_points.copy()
    finally:
        env.close()
    print(f"\ndecoupled first points per env over one env-step: {taken.tolist()}")
    assert (taken > 0).all()
