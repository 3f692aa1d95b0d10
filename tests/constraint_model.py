"""An independent model of the constraint stage (test infrastructure only).

oracle/physics.c restates the device's constraint rows and Newton solve operation for
operation, so device-vs-oracle agreement cannot catch a modelling error they share (a
swapped body in a contact Jacobian, a missing mu^2, a wrong K or B, a wrong sigmoid half,
a wrong fold of the weld rows).  This module builds the same problem from DESIGN section 2
and MuJoCo's documented formulas, in numpy, on dense matrices, and solves it another way:

- H~ = M + armature from the natural-order sum of J^T M_b J (tests/indep_physics.py);
- qfrc_smooth = -K q - D qdot - (k_p (q - q*) + k_d qdot) - qfrc_bias;
- contact rows from point Jacobians, (n +- mu t)^T (J_2 - J_1) at the contact point;
- impedance from the solimp sigmoid in its early-return form with a general power,
  R = max(1e-15, (1 - imp) / imp diagApprox), aref = -B v - K imp r;
- body_invweight0 / dof_invweight0 from H~^-1 at qpos0, as mj_setConst defines them;
- motor locks as the reference's weld rows, one per world axis, kept separate;
- the optimum of 1/2 (a - a0)^T H~ (a - a0) + sum 1/2 D min(0, J a - aref)^2 by a primal
  Newton iteration started at H~^-1 f, with a dense Cholesky / LDL^T per iteration and an
  exact line search that sorts the breakpoints and walks the pieces;
- mj_Euler with implicit joint damping and the free joint's quaternion update.

Every routine takes a dtype: float64 goes through np.linalg, np.longdouble through a short
hand-written LDL^T (np.linalg has no longdouble).  The difference between the two is the
float64 floor of each case, which the tests scale into their bounds.
"""
from __future__ import annotations

import numpy as np

import indep_physics as ip

F64, LD = np.float64, np.longdouble
HAVE_LONGDOUBLE = bool(np.finfo(np.longdouble).eps < 1e-18)
MINVAL = 1e-15                      # MuJoCo's mjMINVAL


# ---------------------------------------------------------------- linear algebra
def _ldl(A):
    n = len(A)
    L = np.eye(n, dtype=A.dtype)
    d = np.zeros(n, dtype=A.dtype)
    for j in range(n):
        w = L[j, :j] * d[:j]
        d[j] = A[j, j] - L[j, :j] @ w
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ w) / d[j]
    return L, d


def spd_solve(A, B, dtype):
    """A^-1 B for a symmetric positive definite A (B a vector or a matrix of columns)."""
    A = np.asarray(A, dtype=dtype)
    B = np.asarray(B, dtype=dtype)
    if dtype == F64:
        L = np.linalg.cholesky(A)
        return np.linalg.solve(L.T, np.linalg.solve(L, B))
    L, d = _ldl(A)
    Y = B.copy()
    n = len(A)
    for j in range(1, n):
        Y[j] = Y[j] - L[j, :j] @ Y[:j]
    Y = (Y.T / d).T
    for j in range(n - 2, -1, -1):
        Y[j] = Y[j] - L[j + 1:, j] @ Y[j + 1:]
    return Y


# ---------------------------------------------------------------- the smooth dynamics
def dof_joint(M):
    return M.jnt[M.dof_body]


def mass_matrix(M, qpos, dtype):
    """H~ = sum_b m_b Jp^T Jp + Jr^T I_w Jr + armature, and the Jacobians it was built from."""
    Jp, Jr, Iw, xpos, xquat = ip.jacobians(M, np.asarray(qpos, dtype=dtype))
    H = np.zeros((M.nv, M.nv), dtype=dtype)
    for b in range(1, M.nbody):
        H = H + M.mass[b] * (Jp[b].T @ Jp[b]) + Jr[b].T @ (Iw[b] @ Jr[b])
    H = H + np.diag(M.armature[dof_joint(M)]).astype(dtype)
    return H, Jp, Jr, xpos, xquat


def bias_force(M, qpos, qvel, dtype):
    """qfrc_bias: ip.bias_force in float64; the same complex-step Newton-Euler sum carried
    in clongdouble for the longdouble path."""
    if dtype == F64:
        return ip.bias_force(M, qpos, qvel)
    h = LD(1e-40)
    q = np.asarray(qpos, dtype=np.clongdouble).copy()
    v = np.asarray(qvel, dtype=LD)
    for b in range(1, M.nbody):
        j = M.jnt[b]
        if j < 0:
            continue
        qa, d0 = M.jqadr[j], M.jdadr[j]
        if M.jtype[j] == ip.JNT_FREE:
            q[qa:qa + 3] = q[qa:qa + 3] + 1j * h * v[d0:d0 + 3]
            w = v[d0 + 3:d0 + 6]
            wn = np.sqrt(np.sum(w * w))
            if wn > 0:
                a = 0.5 * wn * (1j * h)
                dq = np.concatenate([[np.cos(a)], w / wn * np.sin(a)])
                q[qa + 3:qa + 7] = ip.quatmul(q[qa + 3:qa + 7], dq)
        else:
            q[qa] = q[qa] + 1j * h * v[d0]
    Jp, Jr, Iw, _, _ = ip.jacobians(M, np.asarray(qpos, dtype=LD))
    Jpc, Jrc, _, _, _ = ip.jacobians(M, q)
    dJp, dJr = Jpc.imag / h, Jrc.imag / h
    bias = np.zeros(M.nv, dtype=LD)
    g = M.gravity.astype(LD)
    for b in range(1, M.nbody):
        ac = dJp[b] @ v - g
        w = Jr[b] @ v
        tau = Iw[b] @ (dJr[b] @ v) + np.cross(w, Iw[b] @ w)
        bias = bias + Jp[b].T @ (M.mass[b] * ac) + Jr[b].T @ tau
    return bias


def gains_and_targets(raw, rec):
    """PD gains and targets per dof (the default scheme, mujoco_actuators = 1)."""
    nv = raw.nv
    kp, kd, tgt = np.zeros(nv), np.zeros(nv), np.zeros(nv)
    for f in range(3):
        d = raw.dof_pris[f]
        kp[d], kd[d], tgt[d] = raw.kp_gripper[0], raw.kd_gripper[0], float(rec["next"]["x"])
        d = raw.dof_rev[f]
        kp[d], kd[d], tgt[d] = raw.kp_gripper[1], raw.kd_gripper[1], float(rec["next"]["th"])
    d = raw.dof_palm
    kp[d], kd[d], tgt[d] = raw.kp_gripper[2], raw.kd_gripper[2], float(rec["next"]["z"])
    d = raw.dof_base
    kp[d], kd[d], tgt[d] = raw.kp_base[2], raw.kd_base[2], float(rec["base"][2])
    return kp, kd, tgt


# ---------------------------------------------------------------- impedance
def impedance(solimp, r, dtype):
    """MuJoCo's solimp sigmoid of the violation r, early-return form, general power."""
    dmin, dmax, width, mid, power = [dtype(x) for x in solimp]
    if dmin == dmax or width <= MINVAL:
        return (dmin + dmax) / 2
    x = abs(dtype(r)) / width
    if x >= 1:
        return dmax
    if x <= 0:
        return dmin
    if power == 1:
        y = x
    elif x <= mid:
        y = x ** power / mid ** (power - 1)
    else:
        y = 1 - (1 - x) ** power / (1 - mid) ** (power - 1)
    return dmin + y * (dmax - dmin)


def solref_kb(raw, h, dtype):
    tc = max(dtype(raw.solref[0]), 2 * dtype(h))
    dr, dmax = dtype(raw.solref[1]), dtype(raw.solimp[1])
    return 1 / (dmax * dmax * tc * tc * dr * dr), 2 / (dmax * tc)


# ---------------------------------------------------------------- invweight0
def invweights(M, dtype=F64):
    """(body_invweight0[b] translational, dof_invweight0[d]) at qpos0 as mj_setConst
    defines them: trace(J H~^-1 J^T) / 3 over the three translational rows of the body's
    Jacobian, the diagonal of H~^-1 per dof (a free joint's averaged over its translational
    and its rotational dofs).  Returned for the Jacobian at the body's frame origin and at
    its centre of mass: (origin, com, dof)."""
    q0 = np.array(M.raw.qpos0[:M.nq])
    H, Jp, Jr, xpos, xquat = mass_matrix(M, q0, dtype)
    Hi = spd_solve(H, np.eye(M.nv, dtype=dtype), dtype)
    org, com = np.zeros(M.nbody, dtype=dtype), np.zeros(M.nbody, dtype=dtype)
    for b in range(1, M.nbody):
        com[b] = np.trace(Jp[b] @ Hi @ Jp[b].T) / 3
        off = ip.quat2mat(xquat[b]) @ M.ipos[b]            # com - frame origin
        Jo = Jp[b] + np.cross(off, Jr[b].T).T              # v_origin = v_com - w x off
        org[b] = np.trace(Jo @ Hi @ Jo.T) / 3
    dof = np.diag(Hi).copy()
    for b in range(1, M.nbody):
        j = M.jnt[b]
        if j >= 0 and M.jtype[j] == ip.JNT_FREE:
            d0 = M.jdadr[j]
            dof[d0:d0 + 3] = dof[d0:d0 + 3].sum() / 3
            dof[d0 + 3:d0 + 6] = dof[d0 + 3:d0 + 6].sum() / 3
    return org, com, dof


# ---------------------------------------------------------------- the problem
class Problem:
    """One substep's constraint problem: H, Hd = H + h D_joint, f, rows (J, D, aref, eq),
    and fold: the device's row r is sum over model rows i of fold[r][i] lambda_i."""


def build(M, rec, contacts, body_iw, h, dtype=F64, pyramid_rpy=False):
    """M: ip.Model with the live object set (ip.set_object); rec: one GmEnvState record
    (structured scalar); contacts: dict of dist [n], pos [n, 3], frame [n, 3, 3] (rows n,
    t1, t2), g1, g2 [n], mu [n]; body_iw: translational invweight0 per body, the live
    object's included (1 / mass).  pyramid_rpy: the edges' regulariser scaled by 2 mu^2 (an
    open question, see test_pyramid_edges_carry_the_2_mu2_regulariser; off by default, as
    DESIGN section 2 has it)."""
    raw = M.raw
    nv, nq = M.nv, M.nq
    q = np.asarray(rec["qpos"][:nq], dtype=F64)
    v = np.asarray(rec["qvel"][:nv], dtype=F64)
    P = Problem()
    P.h, P.dtype, P.q, P.v = dtype(h), dtype, q, v
    H, Jp, Jr, xpos, xquat = mass_matrix(M, q, dtype)
    jd = dof_joint(M)
    stiff = ip.arr(raw.jnt_stiffness).astype(F64)[jd]
    damp = ip.arr(raw.jnt_damping).astype(F64)[jd]
    qd = np.zeros(nv, dtype=dtype)                          # the coordinate of each 1-dof joint
    for b in range(1, M.nbody):
        j = M.jnt[b]
        if j >= 0 and M.jtype[j] != ip.JNT_FREE:
            qd[M.jdadr[j]] = q[M.jqadr[j]]
    kp, kd, tgt = gains_and_targets(raw, rec)
    vd = v.astype(dtype)
    P.f = -stiff * qd - damp * vd - (kp * (qd - tgt.astype(dtype)) + kd * vd) - bias_force(M, q, v, dtype)
    P.H, P.Hd = H, H + np.diag(dtype(h) * damp.astype(dtype))
    K, B = solref_kb(raw, h, dtype)
    solimp = raw.solimp[:]
    biw = np.asarray(body_iw, dtype=dtype)
    rows_J, rows_D, rows_aref, rows_eq, fold = [], [], [], [], []
    # motor locks: the weld's translational rows along the slide axis, one per world axis
    for k in range(raw.nlock):
        if not int(rec["lock_active"][k]):
            continue
        d = int(raw.lock_dof[k])
        b = int(M.dof_body[d])
        axis = Jp[b][:, d]                                  # the slide's world axis
        tran = biw[b] + biw[M.parent[b]]
        dq = qd[d] - dtype(rec["lock_q"][k])
        terms = {}
        for r in range(3):
            a = axis[r]
            if a == 0:
                continue
            J = np.zeros(nv, dtype=dtype)
            J[d] = a
            imp = impedance(solimp, a * dq, dtype)
            R = max(dtype(MINVAL), (1 - imp) / imp * tran)
            terms[len(rows_J)] = a
            rows_J.append(J)
            rows_D.append(1 / R)
            rows_aref.append(-B * (a * vd[d]) - K * imp * (a * dq))
            rows_eq.append(True)
        fold.append(terms)
    gbody = ip.arr(raw.geom_body)
    R_ = [ip.quat2mat(xquat[b]) for b in range(M.nbody)]
    com = [xpos[b] + R_[b] @ M.ipos[b] for b in range(M.nbody)]
    P.edges = []
    for c in range(len(contacts["dist"])):
        b1, b2 = int(gbody[int(contacts["g1"][c])]), int(gbody[int(contacts["g2"][c])])
        p = np.asarray(contacts["pos"][c], dtype=dtype)
        n, t1, t2 = [np.asarray(contacts["frame"][c][k], dtype=dtype) for k in range(3)]
        mu = dtype(contacts["mu"][c])
        dist = dtype(contacts["dist"][c])

        def point_jac(b):
            if b == 0:
                return np.zeros((3, nv), dtype=dtype)
            return Jp[b] - np.cross(p - com[b], Jr[b].T).T  # v = Jp qd + (Jr qd) x (p - com)
        Jd = point_jac(b2) - point_jac(b1)
        tran = biw[b1] + biw[b2]
        imp = impedance(solimp, dist, dtype)
        R = max(dtype(MINVAL), (1 - imp) / imp * (tran + mu * mu * tran))
        if pyramid_rpy:
            R = 2 * mu * mu * R
        for u in (n + mu * t1, n - mu * t1, n + mu * t2, n - mu * t2):
            J = u @ Jd
            fold.append({len(rows_J): dtype(1)})
            rows_J.append(J)
            rows_D.append(1 / R)
            rows_aref.append(-B * (J @ vd) - K * imp * dist)
            rows_eq.append(False)
    m = len(rows_J)
    P.J = np.array(rows_J, dtype=dtype).reshape(m, nv)
    P.D = np.array(rows_D, dtype=dtype)
    P.aref = np.array(rows_aref, dtype=dtype)
    P.eq = np.array(rows_eq, dtype=bool)
    P.fold = fold
    return P


def forces_at(P, qacc):
    """lambda(qacc) per model row: -D (J qacc - aref), clamped at 0 on the contact rows."""
    lam = -P.D * (P.J @ np.asarray(qacc, dtype=P.dtype) - P.aref)
    return np.where(P.eq, lam, np.maximum(lam, 0))


def folded(P, lam):
    """Model rows -> the device's rows (one per active lock, then the contact edges)."""
    return np.array([sum(a * lam[i] for i, a in t.items()) for t in P.fold], dtype=P.dtype)


def spread(P, efc):
    """J^T lambda for forces given on the device's rows.  A lock's folded force acts on its
    slide dof (sum_r a_r lambda_r is exactly the generalised force of its rows)."""
    out = np.zeros(P.J.shape[1], dtype=P.dtype)
    for r, t in enumerate(P.fold):
        i = next(iter(t))
        if P.eq[i]:
            out = out + (P.J[i] != 0) * P.dtype(efc[r])
        else:
            out = out + P.J[i] * P.dtype(efc[r])
    return out


# ---------------------------------------------------------------- the optimum
def _line_search(P, a, d):
    """The exact minimiser over alpha >= 0 of the cost along a + alpha d: the derivative is
    piecewise linear and increasing, with breakpoints where a contact row changes sign."""
    jar = P.J @ a - P.aref
    jd = P.J @ d
    q0 = d @ (P.H @ a - P.f)
    q1 = d @ (P.H @ d)
    free = ~P.eq
    with np.errstate(divide="ignore", invalid="ignore"):
        bp = np.where(free & (jd != 0), -jar / jd, np.inf)
    bp = np.where(bp > 0, bp, np.inf)
    order = [i for i in np.argsort(bp) if np.isfinite(bp[i])]
    act = P.eq | (jar < 0) | ((jar == 0) & (jd < 0))
    lo = P.dtype(0)
    for i in order + [None]:
        g0 = q0 + np.sum(P.D[act] * jar[act] * jd[act])
        g1 = q1 + np.sum(P.D[act] * jd[act] * jd[act])
        root = -g0 / g1
        hi = np.inf if i is None else bp[i]
        if root <= hi:
            return max(root, lo)
        act[i] = not act[i]
        lo = hi
    raise AssertionError("the line search left its last piece")


def solve(P, max_iter=200):
    """(qacc*, lambda* per model row, iterations, line searches)."""
    dt = P.dtype
    a = spd_solve(P.H, P.f, dt)
    n_ls = 0
    for it in range(1, max_iter + 1):
        act = P.eq | (P.J @ a - P.aref < 0)
        Ja, Da = P.J[act], P.D[act]
        x = spd_solve(P.H + Ja.T @ (Da[:, None] * Ja), P.f + Ja.T @ (Da * P.aref[act]), dt)
        if np.array_equal(P.eq | (P.J @ x - P.aref < 0), act):
            return x, forces_at(P, x), it, n_ls
        d = x - a
        a = a + _line_search(P, a, d) * d
        n_ls += 1
    raise AssertionError("the active set did not reproduce itself")


# ---------------------------------------------------------------- mj_Euler
def euler(M, P, efc):
    """(qvel', qpos') from forces on the device's rows: qvel' = qvel + h (H~ + h D)^-1
    (f + J^T lambda); slides and hinges q + h qvel', the free joint pos + h v and
    quat x [cos(h |w| / 2), w / |w| sin(h |w| / 2)], normalised."""
    dt, h = P.dtype, P.h
    v1 = P.v.astype(dt) + h * spd_solve(P.Hd, P.f + spread(P, efc), dt)
    q1 = P.q.astype(dt).copy()
    for b in range(1, M.nbody):
        j = M.jnt[b]
        if j < 0:
            continue
        qa, d0 = M.jqadr[j], M.jdadr[j]
        if M.jtype[j] == ip.JNT_FREE:
            q1[qa:qa + 3] = q1[qa:qa + 3] + h * v1[d0:d0 + 3]
            w = v1[d0 + 3:d0 + 6]
            wn = np.sqrt(np.sum(w * w))
            if wn > 0:
                ang = h * wn / 2
                dq = np.concatenate([[np.cos(ang)], w / wn * np.sin(ang)])
                q1[qa + 3:qa + 7] = ip.qnormalise(ip.quatmul(q1[qa + 3:qa + 7], dq))
        else:
            q1[qa] = q1[qa] + h * v1[d0]
    return v1, q1
