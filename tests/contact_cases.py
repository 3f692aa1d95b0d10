"""Crafted collider states with known answers (test infrastructure only).

The grasp rollouts reach the collider's common paths; the branches behind thresholds and
caps are reached here on purpose.  Every case is one env: an object (type, size), its
free-joint pose, optionally a base offset, and what the collider must return.  A state is
the oracle's reset record for that object with qpos overwritten (qvel, qacc_warm zeroed),
so device and oracle start from the same bytes.

Two kinds of expectation:

- CLOSED: every contact of the state written out in numpy from the pose, with nothing
  taken from the engine: the gripper geoms' world poses come from the natural-order
  kinematics of tests/indep_physics.py (the reset pose is not axis-aligned: the finger
  frames carry ~9e-5 of tilt), the object is posed relative to them, and plane-sphere,
  plane-box, plane-cylinder and sphere-box are evaluated for every candidate pair, so a
  case also pins that no other pair touches.  Box-box manifolds are the object's
  vertices under a finger face (or the clipped overlap polygon, or the crossed-edge
  midpoint).  MPR pairs are closed form in depth and normal only (MPR_DEPTH, MPR_NORMAL).
- ORACLE: no clean closed form (the engulfing box, a cylinder's rim on a finger edge).
  Pair ids and per-pair counts are pinned to or_collide on the independent FK poses.

MuJoCo conventions: geom1 has the lower type (then the lower id), the normal points from
geom1 to geom2, dist < 0 penetrates, the point is midway between the surfaces.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import indep_physics as ip
import oracle_lib as ol

PLANE, SPH, CYL, BOX = ip.GEOM_PLANE, ip.GEOM_SPHERE, ip.GEOM_CYLINDER, ip.GEOM_BOX
CLOSED, ORACLE = "closed", "oracle"
MPR_DEPTH, MPR_NORMAL = 1e-6, 2e-3          # the convex collider's own tolerance (test_mpr_cylinder_box)
TIMESTEP = {8: None, 10: 2.1e-3, 5: 6.76e-3}  # N = 10 / 5 at the steps test_grasp_parity.py uses for them
FAR = np.array([0.3, 0.3])                  # object placed here touches nothing but the ground
Z = np.array([0.0, 0.0, 1.0])
TILT = 1e-4                                 # takes flush box faces off the exact-parallel tie (box_cases)


# ---------------------------------------------------------------- rotations
def mat2quat(R):
    """(w, x, y, z) of a rotation matrix (largest-pivot branch)."""
    R = np.asarray(R, dtype=np.float64)
    t = np.trace(R)
    if t > 0:
        s = 2.0 * np.sqrt(1.0 + t)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q = np.array(q)
    return q / np.linalg.norm(q)


# ---------------------------------------------------------------- closed forms
def con(g1, g2, dist, pos, n, mpr=False):
    return dict(g1=int(g1), g2=int(g2), dist=float(dist), pos=None if pos is None else np.asarray(pos, float),
                n=np.asarray(n, float), mpr=mpr)


def cf_plane_sphere(c, r):
    d = c[2] - r
    return [(d, np.array([c[0], c[1], c[2] - (r + 0.5 * d)]))] if d < 0 else []


def cf_plane_box(c, R, hs):
    """Corners below z = 0 in index order (bit 0: x, bit 1: y, bit 2: z), at most four."""
    out = []
    for i in range(8):
        s = np.array([hs[0] if i & 1 else -hs[0], hs[1] if i & 2 else -hs[1], hs[2] if i & 4 else -hs[2]])
        v = c + R @ s
        if v[2] < 0 and len(out) < 4:
            out.append((v[2], v - 0.5 * v[2] * Z))
    return out


def cyl_rim_dir(R):
    """The rim direction towards the ground, w = (a_z a - z) / |.|, and |.| itself; an
    upright cylinder (|.| < 1e-6) uses its own x axis."""
    a = R[:, 2]
    w = -Z + a[2] * a
    lw = np.linalg.norm(w)
    return (R[:, 0] if lw < 1e-6 else w / lw), lw


def cf_plane_cyl(c, R, r, hh):
    """Rim points of both caps along w, a x w, -w, -(a x w), top cap first; those below
    z = 0, at most four."""
    a = R[:, 2]
    w, _ = cyl_rim_dir(R)
    axw = np.cross(a, w)
    out = []
    for sg in (1.0, -1.0):
        for d in (w, axw, -w, -axw):
            v = c + sg * hh * a + r * d
            if v[2] < 0 and len(out) < 4:
                out.append((v[2], v - 0.5 * v[2] * Z))
    return out


def cf_sphere_box(cs, r, cb, Rb, hs):
    """(dist, pos, normal sphere -> box) or None.  Outside: along the line from the centre
    to the box's closest point (none when the centre is within 1e-12 of the surface);
    centre inside: through the nearest face, depth = distance to it + r."""
    l = Rb.T @ (cs - cb)
    q = np.clip(l, -hs, hs)
    if np.any(np.abs(l) > hs):
        d = l - q
        ln = np.linalg.norm(d)
        if ln < 1e-12 or not ln - r < 0:
            return None
        n = Rb @ (-d / ln)
        dist = ln - r
        qw = cb + Rb @ q
    else:
        k = int(np.argmin(hs - np.abs(l)))
        sg = 1.0 if l[k] >= 0 else -1.0
        nl = np.zeros(3); nl[k] = -sg
        ql = l.copy(); ql[k] = sg * hs[k]
        n = Rb @ nl
        dist = -((hs[k] - abs(l[k])) + r)
        qw = cb + Rb @ ql
    return dist, 0.5 * (qw + cs + n * r), n


def box_vertices(c, R, hs):
    return [c + R @ (np.array([sx, sy, sz]) * hs) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]


def cf_vertices_under_face(cb, Rb, hsb, ax, sg, co, Ro, hso):
    """Box-box with face (ax, sg) of box b as the reference: the other box's vertices below
    the face plane and over the face.  (dist, pos, outward face normal) each."""
    n = sg * Rb[:, ax]
    out = []
    for v in box_vertices(co, Ro, hso):
        l = Rb.T @ (v - cb)
        d = sg * l[ax] - hsb[ax]
        over = all(abs(l[k]) <= hsb[k] for k in range(3) if k != ax)
        if d < 0 and over:
            out.append((d, v - 0.5 * d * n, n))
    return out


def clip_polygon(poly, axes, bounds):
    """Sutherland-Hodgman: a planar polygon of 3-D points clipped to |p[k]| <= bounds[k] for
    k in axes (the crossing points are on the polygon's own edges)."""
    for k, b in zip(axes, bounds):
        for s in (1.0, -1.0):
            nxt = []
            for i, p in enumerate(poly):
                q = poly[(i + 1) % len(poly)]
                pi, qi = s * p[k] <= b, s * q[k] <= b
                if pi:
                    nxt.append(p)
                if pi != qi:
                    nxt.append(p + (b - s * p[k]) / (s * q[k] - s * p[k]) * (q - p))
            poly = nxt
    return poly


# ---------------------------------------------------------------- the scene
class Scene:
    """One model (N finger segments): its blobs, the independent kinematics and the reset
    pose of the gripper."""

    def __init__(self, gm, n_seg=8):
        self.gm = gm
        p = gm.ModelParams()
        gm.load_library().gm_default_model_params(C.byref(p))
        if TIMESTEP[n_seg] is not None:
            p.n_seg, p.timestep = n_seg, TIMESTEP[n_seg]
        self.n_seg = n_seg
        self.model = gm.ModelBlob(p)
        self.settings = gm.canonical_settings(noise=False, seed=3)
        self.cfg = gm.ConfigBlob(self.settings, self.model)
        self.M = ip.Model(self.model)
        m = self.M.raw
        self.m = m
        self.ngeom, self.npair, self.nq, self.nv = m.ngeom, m.npair, m.nq, m.nv
        self.gtype = ip.arr(m.geom_type)[:m.ngeom].copy()
        self.gbody = ip.arr(m.geom_body)[:m.ngeom].copy()
        self.gpos = ip.arr(m.geom_pos, ip.GM_MAX_GEOM, 3)[:m.ngeom]
        self.gquat = ip.arr(m.geom_quat, ip.GM_MAX_GEOM, 4)[:m.ngeom]
        self.gsize = ip.arr(m.geom_size, ip.GM_MAX_GEOM, 3)[:m.ngeom]
        self.pairs = list(zip(ip.arr(m.pair_a)[:m.npair].tolist(), ip.arr(m.pair_b)[:m.npair].tolist()))
        self.g_obj, self.g_ground = m.geom_obj, m.geom_ground
        self.per_finger = n_seg + 2                      # N + 1 segment boxes and the hook
        self.g_palm = 3 * self.per_finger + 1
        self.qadr_obj = int(ip.arr(m.jnt_qposadr)[ip.arr(m.body_jnt)[m.body_obj]])
        self.qadr_base = int(ip.arr(m.jnt_qposadr)[ip.arr(m.body_jnt)[m.body_base]])
        assert self.qadr_obj == m.dof_obj and self.gtype[self.g_ground] == PLANE
        assert all(self.gtype[g] == BOX for g in range(1, self.g_obj)) and self.g_palm == self.g_obj - 1
        # the object's geom frame is its body frame: the free-joint pose is the geom's pose
        assert not self.gpos[self.g_obj].any() and np.array_equal(self.gquat[self.g_obj], [1.0, 0.0, 0.0, 0.0])
        # the gripper's reset pose (it does not depend on the object)
        objs = (gm._lib.Object * 1)()
        objs[0].type, objs[0].mass, objs[0].friction = SPH, 0.1, 1.0
        objs[0].size[0] = objs[0].size[1] = objs[0].size[2] = 0.02
        self.q0 = self.reset_record(objs, 0)[1]["qpos"][0][:self.nq].copy()
        # the base slide: world z per unit of its coordinate
        q = self.q0.copy()
        q[self.qadr_base] += 1.0
        self.base_dz = float(self.fk_geoms(q)[self.g_palm][0][2] - self.fk_geoms(self.q0)[self.g_palm][0][2])
        assert abs(abs(self.base_dz) - 1.0) < 1e-6

    def reset_record(self, objs, i):
        o = ol.OracleEnv(self.model, self.cfg, objs, env_id=i)
        sp = self.gm.Spawn()
        sp.object_index, sp.x, sp.y, sp.zrot = i, float(FAR[0]), float(FAR[1]), 0.0
        o.reset(sp)
        rec = o.export_state()[None].copy()
        return rec, self.gm.env_state_view(rec)

    def finger_geom(self, f, k):
        """Geom id of finger f's k-th box from the top (k = N + 1: the hook)."""
        return 1 + f * self.per_finger + k

    def pair_index(self, g1, g2):
        a, b = (g1, g2) if (g1, g2) in self.pairs else (g2, g1)
        return self.pairs.index((a, b))

    def fk_geoms(self, q):
        """World (centre, rotation) of every geom from the natural-order kinematics."""
        xp, xq = ip.fk(self.M, q)
        out = []
        for g in range(self.ngeom):
            b = self.gbody[g]
            Rb = ip.quat2mat(xq[b]) if b > 0 else np.eye(3)
            out.append(((xp[b] if b > 0 else np.zeros(3)) + Rb @ self.gpos[g], Rb @ ip.quat2mat(self.gquat[g])))
        return out

    def gripper_q(self, base_z=0.0):
        """Reset pose with the base moved by base_z (world metres, negative = down)."""
        q = self.q0.copy()
        q[self.qadr_base] += base_z / self.base_dz
        return q

    def inner_face(self, geoms, g):
        """(axis, sign) of a finger box's face towards the gripper's axis (its thin side)."""
        c, R = geoms[g]
        return 1, (1.0 if np.dot(R[:2, 1], -c[:2]) > 0 else -1.0)


class Case:
    def __init__(self, name, family, otype, osize, c, R, kind=CLOSED, base_z=0.0, special=None, counts=None,
                 capacity=False, mass=0.1):
        self.name, self.family, self.otype, self.kind = name, family, otype, kind
        self.osize = np.resize(np.asarray(osize, float), 3)
        self.quat = mat2quat(R)
        self.c = np.asarray(c, float)
        self.R = ip.quat2mat(self.quat)        # what the engine's kinematics will see
        self.base_z, self.special, self.counts, self.capacity, self.mass = base_z, special or [], counts, capacity, mass
        self.expected = None                   # CLOSED: every contact of the state, in pair order

    def obj_struct(self, o):
        o.type, o.mass, o.friction = int(self.otype), self.mass, 1.0
        for k in range(3):
            o.size[k] = float(self.osize[k])


def expected_contacts(sc: Scene, case: Case):
    """Every contact of a CLOSED case in candidate-pair order: the generic closed forms for
    the plane and sphere pairs, the case's own entries (case.special) for box-box and MPR."""
    geoms = sc.fk_geoms(sc.gripper_q(case.base_z))
    out = []
    for a, b in sc.pairs:
        if a == sc.g_ground:                              # ground against the object or a gripper box
            if b == sc.g_obj:
                t, c, R, sz = case.otype, case.c, case.R, case.osize
            else:
                t, (c, R), sz = BOX, geoms[b], sc.gsize[b]
            pts = cf_plane_sphere(c, sz[0]) if t == SPH else cf_plane_box(c, R, sz) if t == BOX else \
                cf_plane_cyl(c, R, sz[0], sz[1])
            out += [con(a, b, d, p, Z) for d, p in pts]
        elif case.otype == SPH:                           # the sphere (geom1) against a gripper box
            r = cf_sphere_box(case.c, case.osize[0], geoms[a][0], geoms[a][1], sc.gsize[a])
            if r is not None:
                out.append(con(b, a, *r))
        else:
            out += [s for s in case.special if {s["g1"], s["g2"]} == {a, b}]
    assert all(any(s is o for o in out) for s in case.special), "a special contact names no candidate pair"
    return out


# ---------------------------------------------------------------- the table
def ground_cases(sc):
    cs = []
    at = lambda z: np.array([FAR[0], FAR[1], z])
    I = np.eye(3)
    r = 0.025
    cs.append(Case("sphere 2 mm deep", "plane", SPH, [r], at(r - 2e-3), I, counts=1))
    cs.append(Case("sphere tangent", "plane", SPH, [r], at(r), I, counts=0))
    cs.append(Case("sphere 1e-12 above", "plane", SPH, [r], at(r + 1e-12), I, counts=0))
    cs.append(Case("sphere 1e-12 below", "plane", SPH, [r], at(r - 1e-12), I, counts=1))
    hs = np.array([0.02, 0.015, 0.01])

    def lowest(R, pen):     # centre height that puts the box's lowest corner pen below the ground
        return -min(v[2] for v in box_vertices(np.zeros(3), R, hs)) - pen
    for name, R, pen, n in (("box flat", I, 1e-3, 4), ("box yawed", ip.rotz(0.7), 1e-3, 4),
                            ("box tilted about x", ip.rotx(0.2), 1e-3, 2),
                            ("box tilted about x and y", ip.rotx(0.2) @ ip.roty(0.15), 1e-3, 1),
                            ("box upside down", np.diag([1.0, -1.0, -1.0]), 1e-3, 4)):
        R = ip.quat2mat(mat2quat(R))
        cs.append(Case(name, "plane", BOX, hs, at(lowest(R, pen)), R, counts=n))
    # more than half sunk: all eight corners are below, the first four in index order are kept
    # (upright these are the deep ones, upside down the shallow ones)
    cs.append(Case("box sunk, 8 corners below", "plane", BOX, hs, at(-hs[2] - 2e-3), ip.rotz(0.3), counts=4))
    cs.append(Case("box sunk upside down", "plane", BOX, hs, at(-hs[2] - 2e-3), ip.rotz(0.3) @ np.diag([1.0, -1.0, -1.0]),
                   counts=4))
    cs.append(Case("box sunk and tilted, 6 corners below", "plane", BOX, hs, at(-hs[2]), ip.rotx(0.2), counts=4))
    rc, hh = 0.02, 0.03

    def cyl_low(R, pen):
        a = R[:, 2]
        return hh * abs(a[2]) + rc * np.sqrt(max(0.0, 1.0 - a[2] * a[2])) - pen
    for name, R, n in (("cylinder upright", I, 4), ("cylinder tilted 5e-7 (fallback frame)", ip.rotx(5e-7), 4),
                       ("cylinder tilted 2e-6 (rim frame)", ip.rotx(2e-6), 4),
                       ("cylinder tilted 2e-6 about a skew axis", ip.rotz(0.5) @ ip.rotx(2e-6), 4),
                       ("cylinder tilted 20 deg", ip.rotx(np.radians(20)), 1),
                       ("cylinder on its side", ip.roty(np.pi / 2), 2),
                       ("cylinder on its side, rolled", ip.rotz(0.4) @ ip.roty(np.pi / 2) @ ip.rotz(0.6), 2)):
        R = ip.quat2mat(mat2quat(R))
        cs.append(Case(name, "plane", CYL, [rc, hh], at(cyl_low(R, 1e-3)), R, counts=n))
    return cs


def sphere_cases(sc):
    geoms = sc.fk_geoms(sc.q0)
    cs = []
    g = sc.finger_geom(0, 4)
    (c, R), hs = geoms[g], sc.gsize[g]
    ax, sg = sc.inner_face(geoms, g)
    n = sg * R[:, ax]
    r = 0.01
    on_face = c + R @ np.array([0.002, 0.0, -0.003]) + n * hs[ax]       # a point on the inner face
    cs.append(Case("sphere 1 mm into a finger face", "sphere-box", SPH, [r], on_face + n * (r - 1e-3), np.eye(3), counts=1))
    # the long edge between the inner face and a side face, then the free top corner of the finger
    edge = c + R @ np.array([0.002, sg * hs[1], hs[2]])
    u = (n + R[:, 2]) / np.sqrt(2.0)
    cs.append(Case("sphere on a finger edge", "sphere-box", SPH, [r], edge + u * (r - 1e-3), np.eye(3), counts=1))
    g0 = sc.finger_geom(0, 0)
    (c0, R0), hs0 = geoms[g0], sc.gsize[g0]
    corner = c0 + R0 @ np.array([-hs0[0], sg * hs0[1], hs0[2]])
    u = (-R0[:, 0] + n + R0[:, 2]) / np.sqrt(3.0)
    cs.append(Case("sphere on a finger corner", "sphere-box", SPH, [r], corner + u * (r - 1e-3), np.eye(3), counts=1))
    # a corner shared by two segments: both boxes answer with the same point
    shared = c + R @ np.array([hs[0], sg * hs[1], hs[2]])
    cs.append(Case("sphere on the corner two segments share", "sphere-box", SPH, [r],
                   shared + (n + R[:, 2]) / np.sqrt(2.0) * (r - 1e-3), np.eye(3), counts=2))
    # centre inside a segment (nearest face: the inner one), r = 2 cm reaches both neighbours
    inside = c + R @ np.array([0.002, sg * (hs[1] - 0.001), 0.003])
    cs.append(Case("sphere centre inside a segment", "sphere-box", SPH, [0.02], inside, np.eye(3), counts=3))
    inside = c + R @ np.array([hs[0] - 0.0004, 0.0002, 0.003])
    cs.append(Case("sphere centre inside, nearest the end face", "sphere-box", SPH, [0.02], inside, np.eye(3), counts=2))
    # around the surface: 4e-13 outside (closer than 1e-12: no contact), 2e-12 outside (the
    # outside branch, depth ~ r), 1e-9 inside (the inside branch).  A centre exactly on the
    # face cannot be posed: the collider sees it through world coordinates, ~1e-17 to either
    # side, where "inside" gives a contact of depth r and "outside" none -- so the three cases
    # stand a factor of two or more off both thresholds (0 and 1e-12) instead.
    cs.append(Case("sphere centre 4e-13 off a face", "sphere-box", SPH, [r], on_face + n * 4e-13, np.eye(3), counts=0))
    cs.append(Case("sphere centre 2e-12 off a face", "sphere-box", SPH, [r], on_face + n * 2e-12, np.eye(3), counts=1))
    cs.append(Case("sphere centre 1e-9 under a face", "sphere-box", SPH, [r], on_face - n * 1e-9, np.eye(3), counts=1))
    (cp, Rp), hp = geoms[sc.g_palm], sc.gsize[sc.g_palm]
    down = -Rp[:, 0] if Rp[2, 0] > 0 else Rp[:, 0]
    cs.append(Case("sphere 1 mm into the palm", "sphere-box", SPH, [r],
                   cp + Rp @ np.array([0.0, 0.005, -0.004]) + down * (hp[0] + r - 1e-3), np.eye(3), counts=1))
    return cs


def box_cases(sc):
    geoms = sc.fk_geoms(sc.q0)
    cs = []
    g = sc.finger_geom(0, 4)
    (c, R), hs = geoms[g], sc.gsize[g]
    ax, sg = sc.inner_face(geoms, g)
    n = sg * R[:, ax]
    pen = 1e-3

    def under_face(case, fingers):
        for gf in fingers:
            a, s = sc.inner_face(geoms, gf)
            case.special += [con(gf, sc.g_obj, d, p, nn) for d, p, nn in
                             cf_vertices_under_face(geoms[gf][0], geoms[gf][1], sc.gsize[gf], a, s, case.c, case.R, case.osize)]
        return case
    # Flush faces are exactly parallel: the finger's axis and the object's then tie as the
    # separating axis and rounding picks the reference box (the same manifold, another
    # candidate order).  The object is tilted TILT about the finger's long axis, which makes
    # the finger's face the reference by ~1e-6 of penetration.
    a = 0.005
    off = R @ np.array([0.002, 0.0, -0.003])
    Rt = R @ ip.rotx(TILT)
    cs.append(under_face(Case("box flush on a finger face", "box-box", BOX, [a, a, a], c + off + n * (hs[ax] + a - pen), Rt,
                              counts=4), [g]))
    Rn = Rt @ ip.roty(np.radians(30))                      # about the object's axis along the face normal
    cs.append(under_face(Case("box turned 30 deg on a finger face", "box-box", BOX, [a, a, a],
                              c + off + n * (hs[ax] + a - pen), Rn, counts=4), [g]))
    # a bar turned 30 deg that overhangs the finger's width on both sides.  Across the tilt the
    # bar is the wider box, so its face is the reference (the other branch of the choice):
    # the manifold is the finger's face clipped to the bar's (bar-local x and z), each point
    # on the finger's face, its depth measured from the bar's face along the bar's axis
    bar = np.array([0.004, 0.004, 0.019])
    case = Case("bar turned 30 deg, clipped by the finger face", "box-box", BOX, bar, c + n * (hs[ax] + bar[1] - pen), Rn,
                counts=4)
    face = [np.array([sx * hs[0], sg * hs[1], sz * hs[2]]) for sx, sz in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    loc = [case.R.T @ (c + R @ v - case.c) for v in face]
    assert any(abs(p[0]) > bar[0] for p in loc) and all(abs(p[2]) < bar[2] for p in loc)
    nb = sg * case.R[:, 1]                                 # finger -> bar, along the bar's own axis
    for p in clip_polygon(loc, (0, 2), bar[[0, 2]]):
        depth = bar[1] + sg * p[1]
        assert depth > 0
        case.special.append(con(g, sc.g_obj, -depth, case.c + case.R @ p - 0.5 * depth * nb, nb))
    cs.append(case)
    # crossed edges: the finger's long edge (inner face / side face) against an edge of a
    # cube turned 45 deg, along the diagonal d between the two faces
    a = 0.008
    L, W = R[:, 0], R[:, 2]
    d = (n + W) / np.sqrt(2.0)
    e = np.cross(L, d)
    Ro = np.column_stack([(d + L) / np.sqrt(2.0), e, np.cross((d + L) / np.sqrt(2.0), e)])
    pen = 0.8e-3
    edge_mid = c + R @ np.array([0.001, sg * hs[1], hs[2]])
    case = Case("box on a finger edge, crossed edges", "box-box", BOX, [a, a, a], edge_mid + d * (a * np.sqrt(2.0) - pen), Ro,
                counts=1)
    case.special.append(con(g, sc.g_obj, -pen, edge_mid - 0.5 * pen * d, d))
    cs.append(case)
    # a wide box with one vertical edge in a face of finger 2 and another in finger 3
    g2, g3 = sc.finger_geom(1, 4), sc.finger_geom(2, 4)
    (c3, R3), h3 = geoms[g3], sc.gsize[g3]
    a3, s3 = sc.inner_face(geoms, g3)
    n3 = s3 * R3[:, a3]
    tip = c3 + n3 * (h3[a3] - pen)                         # the box's (+x, +y) edge passes through here
    hy, hz = 0.01, 0.008
    cs.append(under_face(Case("box edges in two fingers' faces", "box-box", BOX, [abs(tip[0]), hy, hz],
                              np.array([0.0, tip[1] - hy, tip[2]]), np.eye(3), counts=4), [g2, g3]))
    return cs


def cylinder_cases(sc):
    geoms = sc.fk_geoms(sc.q0)
    cs = []
    (cp, Rp), hp = geoms[sc.g_palm], sc.gsize[sc.g_palm]
    up_is_x = Rp[2, 0] > 0
    down = -Rp[:, 0] if up_is_x else Rp[:, 0]
    r, hh = 0.02, 0.03
    Rc = np.column_stack([Rp[:, 1], Rp[:, 2], Rp[:, 0]]) if np.linalg.det(np.column_stack([Rp[:, 1], Rp[:, 2], Rp[:, 0]])) > 0 \
        else np.column_stack([Rp[:, 2], Rp[:, 1], Rp[:, 0]])
    case = Case("cylinder cap flush on the palm", "mpr", CYL, [r, hh],
                cp + Rp @ np.array([0.0, 0.003, -0.002]) + down * (hp[0] + hh - 1e-3), Rc, counts=1)
    case.special.append(con(sc.g_obj, sc.g_palm, -1e-3, None, -down, mpr=True))
    cs.append(case)
    g = sc.finger_geom(0, 4)
    (c, R), hs = geoms[g], sc.gsize[g]
    ax, sg = sc.inner_face(geoms, g)
    n = sg * R[:, ax]
    r, hh = 0.015, 0.01
    Rs = np.column_stack([R[:, 1], R[:, 2], R[:, 0]])      # the cylinder's axis along the finger
    if np.linalg.det(Rs) < 0:
        Rs[:, 0] = -Rs[:, 0]
    for name, pen in (("cylinder side 1 mm into a finger face", 1e-3), ("cylinder side 2e-6 into a finger face", 2e-6),
                      ("cylinder side 1e-5 clear of a finger face", -1e-5)):
        case = Case(name, "mpr", CYL, [r, hh], c + R @ np.array([0.001, 0.0, -0.002]) + n * (hs[ax] + r - pen), Rs,
                    counts=1 if pen > 0 else 0)
        if pen > 0:
            case.special.append(con(sc.g_obj, g, -pen, None, -n, mpr=True))
        cs.append(case)
    # a rim on the finger's long edge: no clean closed form, the oracle's pair counts are pinned
    d = (n + R[:, 2]) / np.sqrt(2.0)
    edge_mid = c + R @ np.array([0.0, sg * hs[1], hs[2]])
    e = np.cross(R[:, 0], d)
    Rr = np.column_stack([e, np.cross((d + R[:, 0]) / np.sqrt(2.0), e), (d + R[:, 0]) / np.sqrt(2.0)])
    rim = -hh * Rr[:, 2] - r * Rr[:, 1]                    # the rim point nearest the edge, from the centre
    cs.append(Case("cylinder rim on a finger edge", "mpr", CYL, [r, hh], edge_mid - rim - d * 0.8e-3, Rr, kind=ORACLE))
    return cs


def hooks_base_z(sc, pen=1e-3):
    """Base offset that puts the lowest hook corner pen below the ground."""
    geoms = sc.fk_geoms(sc.q0)
    low = min(v[2] for f in range(3) for v in
              box_vertices(*geoms[sc.finger_geom(f, sc.n_seg + 1)], sc.gsize[sc.finger_geom(f, sc.n_seg + 1)]))
    return -(low + pen)


def capacity_cases(sc):
    cs = []
    # every finger geom and the palm inside one box: > 18 face-case lanes, > 32 candidates
    for z in (0.13, 0.2):
        cs.append(Case(f"engulfing box at z = {z}", "capacity", BOX, [0.2, 0.2, 0.12], [0.0, 0.0, z], np.eye(3),
                       kind=ORACLE, capacity=True, mass=1.0))
    return cs


def hook_case(sc):
    """Hooks of all three fingers 1 mm into the ground, a box resting on the ground."""
    hs = np.array([0.02, 0.015, 0.01])
    return Case("hooks in the ground, box on the ground", "batches", BOX, hs, [FAR[0], FAR[1], hs[2] - 1e-3], ip.rotz(0.3),
                base_z=hooks_base_z(sc), counts=10)


def make_cases(sc: Scene):
    if sc.n_seg == 8:
        cs = ground_cases(sc) + sphere_cases(sc) + box_cases(sc) + cylinder_cases(sc) + capacity_cases(sc) + \
            full_width_cases(sc) + [hook_case(sc)]
    else:
        cs = [hook_case(sc), capacity_cases(sc)[0]] + ground_cases(sc)[4:6] + \
            full_width_cases(sc, hooks_base_z(sc), [("slab on 4 segments, hooks in the ground (ncon 30, the last two from the second batch)", 4),
                              ("slab on 5 segments, hooks in the ground (32 from the first batch, 2 dropped in the second)", 5)])
    for c in cs:
        if c.kind == CLOSED:
            c.expected = expected_contacts(sc, c)
    return cs


def full_width_cases(sc, base_z=0.0, spans=None):
    """ncon at and near GM_MAX_CON without overflow: a slab standing on the ground, flush on
    finger 1's inner face over several segments (4 points per segment, clipped to each
    segment's face) -- the solve at full width on an ordinary problem."""
    geoms = sc.fk_geoms(sc.gripper_q(base_z))
    cs = []
    g = sc.finger_geom(0, sc.n_seg)
    (c, R), hs = geoms[g], sc.gsize[g]
    ax, sg = sc.inner_face(geoms, g)
    n = sg * R[:, ax]
    pen = 2e-4
    for name, nseg in spans or (("slab on 5 segments, the hook and the ground (ncon 28)", 5),
                                ("slab on 6 segments, the hook and the ground (ncon 32, no overflow)", 6)):
        top = geoms[sc.finger_geom(0, sc.n_seg - nseg + 1)][0][2] + 0.5 * hs[0]   # mid-way up the topmost touched segment
        hz = 0.5 * (top + pen)
        hx, hy = 0.01, 0.02
        # the slab's face towards finger 1, parallel to the segment faces but for TILT
        Rs = np.column_stack([R[:, 2] if np.linalg.det(np.column_stack([R[:, 2], n, -R[:, 0]])) > 0 else -R[:, 2], n, -R[:, 0]])
        Rs = Rs @ ip.rotz(TILT)            # (off the parallel-faces tie, see box_cases; local z is the finger's long axis)
        ctr = c + n * (hs[ax] + hy - pen)
        ctr = ctr + Rs[:, 2] * ((hz - pen - ctr @ Z) / Rs[2, 2])
        cs.append(Case(name, "capacity", BOX, [hx, hy, hz], ctr, Rs, kind=ORACLE, base_z=base_z, capacity=True, mass=0.5))
    return cs


# ---------------------------------------------------------------- records
def build_records(sc: Scene, cases):
    """(objects, records): one oracle reset record per case, qpos overwritten with the
    case's pose, qvel and the warm start zeroed."""
    gm = sc.gm
    objs = (gm._lib.Object * len(cases))()
    for i, c in enumerate(cases):
        c.obj_struct(objs[i])
    recs = []
    for i, c in enumerate(cases):
        rec, v = sc.reset_record(objs, i)
        q = sc.gripper_q(c.base_z)
        q[sc.qadr_obj:sc.qadr_obj + 3] = c.c
        q[sc.qadr_obj + 3:sc.qadr_obj + 7] = c.quat
        v["qpos"][0][:sc.nq] = q
        v["qvel"][0][:] = 0.0
        v["qacc_warm"][0][:] = 0.0
        assert int(v["obj_type"][0]) == c.otype and np.array_equal(v["obj_size"][0], c.osize)
        recs.append(rec[0])
    return objs, np.ascontiguousarray(np.stack(recs))


def oracle_pair_counts(sc: Scene, case: Case, tol=None, it=None):
    """Per candidate pair, or_collide's count on the independent FK poses (broadphase:
    the engine's bounding test is not applied, a separated pair simply returns 0)."""
    import test_physics_independent as tpi
    L = ol.lib()
    geoms = sc.fk_geoms(sc.gripper_q(case.base_z))
    tol = sc.m.mpr_tolerance if tol is None else tol
    it = sc.m.mpr_iterations if it is None else it
    out = []
    for a, b in sc.pairs:
        def geom(g):
            if g == sc.g_obj:
                return case.otype, case.osize, case.c, case.R
            if g == sc.g_ground:
                return PLANE, sc.gsize[g], np.zeros(3), np.eye(3)
            return BOX, sc.gsize[g], geoms[g][0], geoms[g][1]
        ga, gb = geom(a), geom(b)
        g1, g2 = a, b
        if ga[0] > gb[0] or (ga[0] == gb[0] and a > b):
            ga, gb, g1, g2 = gb, ga, b, a
        dist, _, _ = tpi.collide(L, ga[0], ga[1], ga[2], ga[3], gb[0], gb[1], gb[2], gb[3], tol=tol, it=it)
        out.append((g1, g2, len(dist)))
    return out
