"""The collision geometry's edge cases as problems of a batch: a point robot whose
sphere centre is its joint vector, one primitive and two waypoints per case.

pointbot: three prismatic joints x, y, z off the base and one sphere (radius
R_BOT) on link 3, so the sphere's centre is q and its linear jacobian the
identity.  A step pair with coll_lvs = 1e308 is one cast q_t -> q_t+1.  twobot:
two such branches off the root (parents [0, 1, 2, 0, 4, 5]), spheres on links 3
and 6 (radii R_BOT, R_BOT_B), self pair (3, 6), 6 dofs: q[:3] and q[3:] are the
two centres.

A case is a dict: name, family (static / swept / self / threshold_static /
threshold_swept / substate), prim (a 16-double record, None for self casts), a, b
(the two waypoints; a == b for a static case) and, where the geometry is
degenerate, what the kernels' convention gives: `normal` (stated exactly) and
`t_left` (the left end of a flat minimiser interval).  Threshold cases carry
`contacts` (1 or 0) and come in pairs, the true distance 1e-7 under and over
margin + buffer.  tests/test_geometry_reference.py validates every entry against
tests/geometry_reference.py and the oracle on the CPU.
"""
import numpy as np

import geometry_reference as gr
from trajopt_amd import abi, problems, robots

R_BOT, R_BOT_B = 0.05, 0.04
BIG_MARGIN = 10.0  # every pair is a contact
THR_MARGIN, THR_BUFFER = 0.1, 0.01
THRESHOLD = THR_MARGIN + THR_BUFFER
EPS = 1e-7
ONE_CAST = 1e308
DISCRETE, LVS_DISCRETE, LVS_CONTINUOUS = 2, 0, 1  # the coll_continuous encoding
COEFF = 20.0


# ------------------------------------------------------------------ robots
def _prismatic(prefix):
    return [(f"{prefix}_x", abi.JOINT_PRISMATIC, (0.0, 0.0, 0.0), (1, 0, 0), (-20.0, 20.0)),
            (f"{prefix}_y", abi.JOINT_PRISMATIC, (0.0, 0.0, 0.0), (0, 1, 0), (-20.0, 20.0)),
            (f"{prefix}_z", abi.JOINT_PRISMATIC, (0.0, 0.0, 0.0), (0, 0, 1), (-20.0, 20.0))]


def pointbot_chain():
    return robots._chain((0.0, 0.0, 0.0), _prismatic("point"))


def twobot_chain():
    return robots._chain((0.0, 0.0, 0.0), _prismatic("a") + _prismatic("b"), parents=[0, 1, 2, 0, 4, 5])


def _set_spheres(d, spheres):
    d.n_spheres = len(spheres)
    for s, (link, r) in enumerate(spheres):
        d.sphere_link[s], d.sphere_radius[s] = link, r
        for i in range(3):
            d.sphere_center[s][i] = 0.0


def make_desc(robot, kind, margin=BIG_MARGIN, buffer=0.0, lvs=ONE_CAST, first=0, last=-1, n_prims=1):
    """A config C descriptor (2 waypoints, on the PR2 arm's first 3 or 6 joints) with the
    point chain and its sphere table swapped in: no CartPose terms, no fixed collision
    step, no per-pair data, contact test ALL."""
    arm = {"pointbot": "right_arm_3dof", "twobot": "right_arm_6dof"}[robot]
    d = abi.ProblemDesc.from_buffer_copy(problems.make_workload("C", 1, n_steps=2, robot=arm).desc)
    d.n_cart = 0
    d.n_coll_pairs = d.n_coll_extra = 0
    if robot == "pointbot":
        d.chain = pointbot_chain()
        _set_spheres(d, [(3, R_BOT)])
        d.n_self_pairs = 0
    else:
        d.chain = twobot_chain()
        _set_spheres(d, [(3, R_BOT), (6, R_BOT_B)])
        d.n_self_pairs = 1
        d.self_pair[0][0], d.self_pair[0][1] = 3, 6
    d.n_prims = n_prims
    d.coll_enabled, d.coll_is_cnt, d.coll_continuous = 1, 0, kind
    d.coll_first_step, d.coll_last_step, d.coll_n_fixed = first, last, 0
    d.coll_margin, d.coll_coeff, d.coll_buffer, d.coll_lvs = margin, COEFF, buffer, lvs
    d.coll_contact_test = abi.CONTACT_ALL
    d.coll_max_contacts = 64
    return d


def make_workload(cases, kind, **kw):
    """The cases (all on one robot) as one batch: problem k is cases[k]."""
    robot = "twobot" if cases[0]["prim"] is None else "pointbot"
    assert all((c["prim"] is None) == (robot == "twobot") for c in cases)
    d = make_desc(robot, kind, n_prims=0 if robot == "twobot" else 1, **kw)
    x = np.array([[c["a"], c["b"]] for c in cases], dtype=np.float64)
    scene = (np.zeros((len(cases), 0, 16)) if robot == "twobot"
             else np.ascontiguousarray(np.stack([c["prim"][None] for c in cases])))
    return problems.Workload("geometry", d, x, np.zeros((len(cases), 0, 12)), scene, x.copy())


# ------------------------------------------------------------------ primitives
def sphere(c, r):
    rec = np.zeros(16)
    rec[0], rec[1:4], rec[4] = abi.PRIM_SPHERE, c, r
    return rec


def capsule(a, b, r):
    rec = np.zeros(16)
    rec[0], rec[1:4], rec[4:7], rec[7] = abi.PRIM_CAPSULE, a, b, r
    return rec


def box(c, R, h):
    rec = np.zeros(16)
    rec[0], rec[1:4], rec[4:13], rec[13:16] = abi.PRIM_BOX, c, np.asarray(R, dtype=float).reshape(9), h
    return rec


H = (0.1, 0.2, 0.3)
ROT = np.array([[2.0, -1.0, 2.0], [2.0, 2.0, -1.0], [-1.0, 2.0, 2.0]]) / 3.0  # a rotation, det +1
C_SPH = np.array([0.3, -0.2, 0.1])
SPH = sphere(C_SPH, 0.15)
SPH0 = sphere((0.0, 0.0, 0.0), 0.15)
CAPZ = capsule((0.0, 0.0, -0.25), (0.0, 0.0, 0.25), 0.05)
CAPS = capsule((0.1, -0.2, -0.25), (0.3, 0.1, 0.25), 0.04)
CAP0 = capsule((0.1, 0.2, 0.3), (0.1, 0.2, 0.3), 0.05)  # a == b
BOX0 = box((0.0, 0.0, 0.0), np.eye(3), H)
C_BOXR = np.array([0.3, -0.2, 0.1])
BOXR = box(C_BOXR, ROT, H)
# the threshold family
SPHT = sphere((0.0, 0.0, 0.0), 0.2)
BOXL = box((0.0, 0.0, 0.0), np.eye(3), (0.5, 0.01, 0.01))
CAPL = capsule((-0.5, 0.0, 0.0), (0.5, 0.0, 0.0), 0.02)


def _w(pl):
    """A point given in BOXR's frame, in the world."""
    return C_BOXR + ROT @ np.asarray(pl, dtype=float)


def _case(name, family, prim, a, b=None, **kw):
    a = np.asarray(a, dtype=np.float64)
    b = a.copy() if b is None else np.asarray(b, dtype=np.float64)
    return dict(name=name, family=family, prim=prim, a=a, b=b, normal=kw.pop("normal", None),
                t_left=kw.pop("t_left", None), **kw)


# ------------------------------------------------------------------ static
def _static():
    S = lambda name, prim, p, **kw: _case(name, "static", prim, p, **kw)  # noqa: E731
    Z = (0.0, 0.0, 1.0)
    out = [
        S("sphere_outside", SPH, C_SPH + (0.2, 0.1, -0.2)),
        S("sphere_inside", SPH, C_SPH + (0.03, -0.02, 0.01)),
        S("sphere_on_centre", SPH, C_SPH, normal=Z),
        S("capsule_on_axis", CAPZ, (0.0, 0.0, 0.125), normal=Z),
        S("capsule_on_endpoint", CAPZ, (0.0, 0.0, -0.25), normal=Z),
        S("capsule_beyond_cap_a", CAPZ, (0.05, 0.02, -0.4)),
        S("capsule_beyond_cap_b", CAPZ, (-0.03, 0.04, 0.45)),
        S("capsule_beside_shaft", CAPZ, (0.2, 0.1, 0.05)),
        S("capsule_slanted_beyond_cap_a", CAPS, (0.0, -0.3, -0.4)),
        S("capsule_slanted_beyond_cap_b", CAPS, (0.35, 0.2, 0.4)),
        S("capsule_slanted_beside_shaft", CAPS, (0.4, -0.2, 0.0)),
        S("capsule_a_eq_b_outside", CAP0, (0.3, 0.1, 0.2)),
        S("capsule_a_eq_b_on_point", CAP0, (0.1, 0.2, 0.3), normal=Z),
    ]
    local = [("outside_face", (0.25, 0.05, -0.1)), ("outside_edge", (0.2, 0.3, 0.1)),
             ("outside_corner", (0.2, 0.3, 0.45)),
             ("inside_face_px", (0.08, 0.05, 0.1)), ("inside_face_mx", (-0.08, 0.05, 0.1)),
             ("inside_face_py", (0.02, 0.17, 0.1)), ("inside_face_my", (0.02, -0.17, 0.1)),
             ("inside_face_pz", (0.02, 0.05, 0.27)), ("inside_face_mz", (0.02, 0.05, -0.27))]
    for name, pl in local:
        out.append(S(f"box_{name}", BOX0, pl))
        out.append(S(f"boxrot_{name}", BOXR, _w(pl)))
    d0 = 0.1 - 0.0625  # exact: the depths below tie bitwise (checked on the CPU)
    d1 = 0.2 - 0.125
    out += [
        # equal depth to two faces: the lower axis index wins
        S("box_tie_xy_mx", BOX0, (-0.0625, 0.2 - d0, 0.1), normal=(1.0, 0.0, 0.0), tie=(0, 1)),
        S("box_tie_xy_px", BOX0, (0.0625, -(0.2 - d0), 0.1), normal=(-1.0, 0.0, 0.0), tie=(0, 1)),
        S("box_tie_yz_my", BOX0, (0.0, -0.125, 0.3 - d1), normal=(0.0, 1.0, 0.0), tie=(1, 2)),
        # on the surface: the <= inside branch at depth 0
        S("box_on_face_px", BOX0, (0.1, 0.05, 0.1), normal=(-1.0, 0.0, 0.0), depth0=True),
        S("box_on_face_my", BOX0, (0.02, -0.2, 0.1), normal=(0.0, 1.0, 0.0), depth0=True),
        S("box_on_edge_xy", BOX0, (0.1, 0.2, 0.1), normal=(-1.0, 0.0, 0.0), depth0=True),
        S("box_on_edge_yz", BOX0, (0.02, -0.2, 0.3), normal=(0.0, 1.0, 0.0), depth0=True),
        S("box_on_corner", BOX0, (-0.1, 0.2, -0.3), normal=(1.0, 0.0, 0.0), depth0=True),
        S("box_on_centre", BOX0, (0.0, 0.0, 0.0), normal=(-1.0, 0.0, 0.0)),
    ]
    return out


# ------------------------------------------------------------------ swept
def _swept():
    W = lambda name, prim, a, b, **kw: _case(name, "swept", prim, a, b, **kw)  # noqa: E731
    Z = (0.0, 0.0, 1.0)
    c = C_SPH
    p0 = c + (0.2, 0.1, -0.2)
    d = 2.0 ** -10
    out = [
        # sphere
        W("sphere_a_eq_b", SPH, p0, p0, t_left=0.0),
        W("sphere_motion_1e-7", SPH, p0, p0 + (EPS, 0.0, 0.0)),
        W("sphere_closest_at_0", SPH, c + (0.25, 0.0, 0.0), c + (0.5, 0.2, 0.0)),
        W("sphere_closest_at_1", SPH, c + (0.5, 0.2, 0.0), c + (0.25, 0.0, 0.0)),
        W("sphere_closest_inside_cast", SPH, c + (0.25, -0.3, 0.05), c + (0.25, 0.3, 0.1)),
        W("sphere_through_centre", SPH0, (-0.4, 0.0, 0.0), (0.4, 0.0, 0.0), normal=Z),
        W("sphere_in_to_out", SPH, c + (0.05, -0.1, 0.0), c + (0.05, 0.4, 0.0)),
        W("sphere_out_to_in", SPH, c + (0.05, 0.4, 0.0), c + (0.05, -0.1, 0.0)),
        # capsule
        W("capsule_a_eq_b", CAPS, (0.4, -0.2, 0.0), (0.4, -0.2, 0.0), t_left=0.0),
        W("capsule_motion_1e-7", CAPS, (0.4, -0.2, 0.0), (0.4, -0.2 + EPS, EPS)),
        W("capsule_closest_at_0", CAPS, (0.4, -0.2, 0.0), (0.7, -0.5, 0.1)),
        W("capsule_closest_at_1", CAPS, (0.7, -0.5, 0.1), (0.4, -0.2, 0.0)),
        W("capsule_closest_inside_cast", CAPS, (0.5, -0.4, -0.2), (0.1, 0.3, 0.3)),
        W("capsule_beyond_cap_cast", CAPS, (0.0, -0.1, -0.45), (0.3, -0.5, -0.35)),
        W("capsule_through_axis", CAPZ, (-0.4, 0.0, 0.0), (0.4, 0.0, 0.0), normal=Z),
        W("capsule_in_to_out", CAPZ, (0.02, -0.01, 0.1), (0.3, 0.2, 0.4)),
        W("capsule_out_to_in", CAPZ, (0.3, 0.2, 0.4), (0.02, -0.01, 0.1)),
        W("capsule_zero_length_cast", CAP0, (0.4, 0.0, 0.2), (-0.1, 0.3, 0.5)),
        # parallel to the axis: every t over the shaft ties, the smaller wins
        W("capsule_parallel_over_shaft", CAPZ, (0.25, 0.0, -0.125), (0.25, 0.0, 0.125), t_left=0.0),
        W("capsule_parallel_entering_shaft", CAPZ, (0.25, 0.0, -0.75), (0.25, 0.0, 0.25), t_left=0.5),
        # box, identity rotation
        W("box_a_eq_b_outside", BOX0, (0.25, 0.05, -0.1), (0.25, 0.05, -0.1), t_left=0.0),
        W("box_a_eq_b_inside", BOX0, (0.08, 0.05, 0.1), (0.08, 0.05, 0.1), t_left=0.0),
        W("box_motion_1e-7_outside", BOX0, (0.25, 0.05, -0.1), (0.25 - EPS, 0.05 + EPS, -0.1)),
        W("box_motion_1e-7_inside", BOX0, (0.08, 0.05, 0.1), (0.08 - EPS, 0.05, 0.1)),
        W("box_closest_at_0", BOX0, (0.2, 0.3, 0.1), (0.5, 0.4, 0.3)),
        W("box_closest_at_1", BOX0, (0.5, 0.4, 0.3), (0.2, 0.3, 0.1)),
        W("box_closest_inside_cast", BOX0, (0.45, -0.1, 0.05), (-0.05, 0.4, 0.05)),
        W("box_through_centre", BOX0, (-0.4, -0.3, -0.2), (0.4, 0.3, 0.2), normal=(-1.0, 0.0, 0.0)),
        # deepest on the mid plane x = 0, where the +x and -x faces tie and the sign of the
        # normal hangs on the sign of a zero: the crossing is at a dyadic t (1/8, 7/8), so x is
        # exactly 0 there with or without fused multiply-adds, and the convention is stated
        W("box_in_to_out", BOX0, (0.0625, 0.05, 0.1), (-0.4375, 0.1, 0.1), normal=(-1.0, 0.0, 0.0)),
        W("box_out_to_in", BOX0, (-0.4375, 0.1, 0.1), (0.0625, 0.05, 0.1), normal=(-1.0, 0.0, 0.0)),
        W("box_in_to_out_face_switch", BOX0, (0.09, 0.0, 0.1), (0.02, 0.5, 0.1)),
        W("box_crossing", BOX0, (0.4, 0.1, 0.05), (-0.35, -0.3, -0.1)),
        W("box_inside_face_switch", BOX0, (0.08, -0.15, 0.0), (-0.02, 0.19, 0.1)),
        # grazing: through the edge / corner itself, and 2^-10 (1, 1[, 1]) off it
        W("box_grazing_edge_touch", BOX0, (0.1 + 0.125, 0.2 - 0.125, 0.0), (0.1 - 0.125, 0.2 + 0.125, 0.0)),
        W("box_grazing_edge_near", BOX0, (0.1 + d + 0.125, 0.2 + d - 0.125, 0.0), (0.1 + d - 0.125, 0.2 + d + 0.125, 0.0)),
        W("box_grazing_corner_touch", BOX0, (0.1 + 0.125, 0.2 - 0.125, 0.3), (0.1 - 0.125, 0.2 + 0.125, 0.3)),
        W("box_grazing_corner_near", BOX0, (0.1 + d + 0.125, 0.2 + d - 0.125, 0.3 + d),
          (0.1 + d - 0.125, 0.2 + d + 0.125, 0.3 + d)),
        # parallel to a face, in coordinates that make the left end of the flat minimum exact:
        # y runs -0.4 -> 0.4 (4 and 8 times the 0.1 of h); over the face |y| <= 0.2 from t = 1/4;
        # inside at x = 0 the x depth 0.1 is the smallest while 0.2 - |y| >= 0.1, from t = 3/8
        W("box_parallel_over_face", BOX0, (0.25, -0.4, 0.0), (0.25, 0.4, 0.0), t_left=0.25),
        W("box_parallel_past_edge", BOX0, (0.25, -0.4, 0.5), (0.25, 0.4, 0.5), t_left=0.25),
        W("box_parallel_inside", BOX0, (0.0, -0.4, 0.125), (0.0, 0.4, 0.125), t_left=0.375),
        # box, rotated
        W("boxrot_entering", BOXR, _w((0.4, 0.1, 0.05)), _w((0.03, -0.05, 0.1))),
        W("boxrot_crossing", BOXR, _w((0.4, 0.1, 0.05)), _w((-0.35, -0.3, -0.1))),
        W("boxrot_leaving", BOXR, _w((0.03, -0.05, 0.1)), _w((-0.2, 0.45, 0.2))),
        W("boxrot_inside_face_switch", BOXR, _w((0.08, -0.15, 0.0)), _w((-0.02, 0.19, 0.1))),
        W("boxrot_closest_inside_cast", BOXR, _w((0.45, -0.1, 0.05)), _w((-0.05, 0.4, 0.05))),
    ]
    return out


# ------------------------------------------------------------------ self casts (twobot)
def _self():
    def V(name, a0, a1, b0, b1, **kw):
        return _case(name, "self", None, tuple(a0) + tuple(b0), tuple(a1) + tuple(b1), **kw)

    return [
        V("both_still", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.25, 0.1, 0.0), (0.25, 0.1, 0.0), t_left=0.0),
        V("b_still", (0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.25, 0.125, 0.1), (0.25, 0.125, 0.1)),
        V("a_still", (0.25, 0.125, 0.1), (0.25, 0.125, 0.1), (0.0, 0.0, 0.0), (0.5, 0.0, 0.0), t_left=0.0),
        V("parallel_same_direction", (0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.0, 0.25, 0.0), (0.5, 0.25, 0.0), t_left=0.0),
        V("parallel_opposite_direction", (0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.5, 0.25, 0.0), (0.0, 0.25, 0.0), t_left=0.0),
        V("parallel_overlapping", (0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.25, 0.25, 0.0), (0.75, 0.25, 0.0), t_left=0.5),
        V("parallel_disjoint", (0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.75, 0.25, 0.0), (1.25, 0.25, 0.0)),
        V("crossing", (0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.25, -0.25, 0.125), (0.25, 0.25, 0.125)),
        V("crossing_skew", (0.0, 0.1, 0.0), (0.5, -0.1, 0.2), (0.3, -0.25, 0.3), (0.1, 0.25, 0.2)),
        V("closest_at_ends", (0.0, 0.0, 0.0), (0.2, 0.0, 0.0), (0.5, 0.1, 0.0), (0.3, 0.3, 0.1)),
        V("motion_1e-3", (0.0, 0.0, 0.0), (1e-3, 0.0, 0.0), (0.0005, 0.1, -0.0005), (0.0005, 0.1, 0.0005)),
        V("motion_1e-7", (0.0, 0.0, 0.0), (EPS, 0.0, 0.0), (0.0, 0.1, 0.0), (0.0, 0.1, EPS)),
        V("motion_1e-7_one_still", (0.0, 0.0, 0.0), (EPS, EPS, 0.0), (0.06, 0.08, 0.0), (0.06, 0.08, 0.0)),
    ]


# ------------------------------------------------------------------ threshold
def _threshold():
    out = []

    def pair(name, family, prim, at, b_at=None):
        for sign, n in ((-1.0, 1), (1.0, 0)):
            a = at(sign * EPS)
            out.append(_case(f"{name}_{'under' if n else 'over'}", family, prim, a, None if b_at is None else b_at(sign * EPS),
                             contacts=n, offset=sign * EPS))

    L = 0.2 + R_BOT + THRESHOLD  # centre distance at the threshold
    u = np.array([2.0, -1.0, 2.0]) / 3.0
    pair("static_sphere_x", "threshold_static", SPHT, lambda e: (L + e, 0.0, 0.0))
    pair("static_sphere_oblique", "threshold_static", SPHT, lambda e: (L + e) * u)
    pair("swept_sphere_interior", "threshold_swept", SPHT, lambda e: (L + e, -0.3, 0.0), lambda e: (L + e, 0.3, 0.0))
    pair("swept_sphere_at_0", "threshold_swept", SPHT, lambda e: (L + e, 0.0, 0.0), lambda e: (L + e + 0.3, 0.2, 0.0))
    pair("swept_sphere_at_1", "threshold_swept", SPHT, lambda e: (0.0, 0.4, L + e + 0.3), lambda e: (0.0, 0.0, L + e))
    pair("swept_sphere_motion_1e-7", "threshold_swept", SPHT, lambda e: (L + e, 0.0, 0.0), lambda e: (L + e, EPS, 0.0))
    # the loosest bounding spheres: a long thin box and a long capsule, beside the middle and past the tip
    yb = 0.01 + R_BOT + THRESHOLD
    xb = 0.5 + R_BOT + THRESHOLD
    pair("static_thin_box_beside", "threshold_static", BOXL, lambda e: (0.1, yb + e, 0.0))
    pair("static_thin_box_tip", "threshold_static", BOXL, lambda e: (xb + e, 0.0, 0.0))
    pair("swept_thin_box_beside", "threshold_swept", BOXL, lambda e: (-0.3, yb + e, 0.0), lambda e: (0.3, yb + e, 0.0))
    pair("swept_thin_box_tip", "threshold_swept", BOXL, lambda e: (xb + e, -0.2, 0.0), lambda e: (xb + e, 0.2, 0.0))
    yc = 0.02 + R_BOT + THRESHOLD
    xc = 0.5 + 0.02 + R_BOT + THRESHOLD
    pair("static_long_capsule_beside", "threshold_static", CAPL, lambda e: (0.1, yc + e, 0.0))
    pair("static_long_capsule_tip", "threshold_static", CAPL, lambda e: (xc + e, 0.0, 0.0))
    pair("swept_long_capsule_beside", "threshold_swept", CAPL, lambda e: (-0.3, 0.0, yc + e), lambda e: (0.3, 0.0, yc + e))
    pair("swept_long_capsule_tip", "threshold_swept", CAPL, lambda e: (xc + e, -0.2, 0.0), lambda e: (xc + e, 0.2, 0.0))
    return out


# ------------------------------------------------------------------ sub-states
SUB_LVS = 0.25  # a motion of 0.75: ceil(0.75 / 0.25) + 1 = 4 sub-states
SUBSTATE = [_case("through_box_4_substates", "substate", BOX0, (-0.3125, 0.0625, 0.03125), (0.4375, 0.0625, 0.03125)),
            _case("through_rotated_box_4_substates", "substate", BOXR, _w((-0.3125, 0.0625, 0.03125)),
                  _w((0.4375, 0.0625, 0.03125)))]

STATIC, SWEPT, SELF, THRESHOLD_CASES = _static(), _swept(), _self(), _threshold()
THRESHOLD_STATIC = [c for c in THRESHOLD_CASES if c["family"] == "threshold_static"]
THRESHOLD_SWEPT = [c for c in THRESHOLD_CASES if c["family"] == "threshold_swept"]
# for the kinds that look at each waypoint on its own (DISCRETE): the same states at waypoint 0
# and the robot far away at waypoint 1, so that a problem has exactly 1 or 0 contacts
THRESHOLD_STATIC_ALONE = [dict(c, name=c["name"] + "_alone", b=c["a"] + 3.0) for c in THRESHOLD_STATIC]
for _group in (STATIC, SWEPT, SELF, THRESHOLD_CASES, THRESHOLD_STATIC_ALONE, SUBSTATE):
    for _c in _group:
        _c["a"].setflags(write=False)
        _c["b"].setflags(write=False)
        if _c["prim"] is not None:
            _c["prim"].setflags(write=False)

# What a kernel cannot express (listed, not skipped at run time):
#   * the DISCRETE evaluator and CHECK_DISCRETE see one state at a time: they run STATIC,
#     THRESHOLD_STATIC and SELF's two waypoints; a cast's interior (the swept, self-cast
#     and sub-state families' subject) needs a step pair.
#   * thip_csets_* is the single-timestep set: the same.  thip_ccsets_* has no DISCRETE
#     type: static cases reach it as a == b casts (the swept family has them).
#   * thip_terms_run returns costs: a contact between margin and margin + buffer adds 0,
#     so the threshold pairs show in its slot only when the hinge's own threshold is the
#     one probed (margin = THRESHOLD, buffer 0: coeff * 1e-7 against exactly 0).


# ------------------------------------------------------------------ the reference's answers
def _radii(case):
    return (R_BOT, R_BOT_B) if case["prim"] is None else (R_BOT, 0.0)


def substates(case, n_states):
    """The waypoints' LinSpaced sub-states (in long double; the kernels' differ by an ulp)."""
    a, b = case["a"].astype(gr.LD), case["b"].astype(gr.LD)
    return [a + (b - a) * (gr.LD(i) / gr.LD(n_states - 1)) for i in range(n_states)]


def ref_static(case, p=None):
    """(distance, normal or None) of the state p (default: waypoint a)."""
    p = case["a"] if p is None else p
    if case["prim"] is None:
        ra, rb = _radii(case)
        v = gr._v(p[3:]) - gr._v(p[:3])
        L = gr._norm(v)
        return L - ra - rb, v / L
    return gr.sdf(p, case["prim"], R_BOT), gr.normal(p, case["prim"])


def ref_cast(case, a=None, b=None):
    """(minimum distance, a minimiser) of the cast a -> b (default: the two waypoints)."""
    a = case["a"] if a is None else a
    b = case["b"] if b is None else b
    if case["prim"] is None:
        ra, rb = _radii(case)
        val, s, _ = gr.self_cast_min(a[:3], b[:3], a[3:], b[3:], ra, rb)
        return val, s
    return gr.swept_min(a, b, case["prim"], R_BOT)


def ref_at(case, t, a=None, b=None):
    """The cast's distance with the robot sphere (self: side a) at time t -- self: the
    other side at its best -- and the normal there (None where the gradient is not defined)."""
    a = case["a"] if a is None else a
    b = case["b"] if b is None else b
    if case["prim"] is None:
        ra, rb = _radii(case)
        pa = gr._v(a[:3]) + gr.LD(t) * (gr._v(b[:3]) - gr._v(a[:3]))
        L, tb = gr.point_segment(pa, a[3:], b[3:])
        return L - ra - rb, gr.self_normal_at(a[:3], b[:3], a[3:], b[3:], t, tb), tb
    p = gr._v(a) + gr.LD(t) * (gr._v(b) - gr._v(a))
    return gr.sdf(p, case["prim"], R_BOT), gr.normal(p, case["prim"]), None


def well_conditioned(case, p):
    """The rule for a normal that can be compared at 1e-9: the centre at least 1e-3 from
    the closest point, the two smallest of a box's six face depths at least 1e-3 apart."""
    if case["prim"] is None:
        return True  # centres at least 0.05 apart in this family
    L, gap = gr.conditioning(p, case["prim"])
    return L >= 1e-3 and gap >= 1e-3


# ------------------------------------------------------------------ rows against the reference
TOL_DIST = 1e-12   # tests/test_gpu_dropin.py _check_rows' tolerance for row distances
TOL_TIME = 1e-12
TOL_NORMAL = 1e-9
CLEANUP = 1e-7     # cleanupAff: a row coefficient at or below it is dropped


def row_normal(case, row, single):
    """What the row says the normal is, and what the true normal n would give: on the point
    robot a_t + a_t+1 is -n on side a's dofs (self: +n on side b's), each part scaled by
    1 - cc_time / cc_time and dropped when at or below 1e-7."""
    D = 6 if case["prim"] is None else 3
    a0, a1 = row[8:8 + D], row[8 + D:8 + 2 * D]
    return -(a0 + a1)[:3], (a0 + a1)[3:6] if D == 6 else None


def _parts(n, T, single):
    n = np.asarray(n, dtype=np.float64)
    if single:
        return np.where(np.abs(n) > CLEANUP, n, 0.0)
    p0, p1 = (1.0 - T) * n, T * n
    return np.where(np.abs(p0) > CLEANUP, p0, 0.0) + np.where(np.abs(p1) > CLEANUP, p1, 0.0)


def _normal_diff(got, n, T, single):
    """max |got - expected| over the components the row can carry (a component of the
    normal under 1e-5 may have been cleaned up: it is compared at its own size)."""
    n = np.asarray(n, dtype=np.float64)
    slack = np.where((np.abs(n) < 1e-5) & (n != 0.0), np.abs(n), 0.0)
    return float(np.max(np.maximum(np.abs(got - _parts(n, T, single)) - slack, 0.0)))


def units_of(case, kind, n_states=2):
    """The contacts the reference expects of a case under an evaluator, in row order:
    (unit waypoint, sub-state, static state or None, cast (a, b) or None)."""
    if kind == DISCRETE:
        return [(0, 0, case["a"], None), (1, 0, case["b"], None)]
    st = [case["a"], case["b"]] if n_states == 2 else substates(case, n_states)
    if kind == LVS_DISCRETE:
        return [(0, i, st[i], None) for i in range(n_states)]
    return [(0, i, None, (st[i], st[i + 1])) for i in range(n_states - 1)]


def check_rows(rows, cases, kind, n_states=2, threshold=False, label="", loose=None):
    """Every problem's rows [n, 8 + 2 D + 1] against the reference: count, keys, distance,
    cc_time and the normal read off the row.  Returns the worst differences.  `loose`
    collects (problem, row) of the contacts whose normal is neither stated nor well
    conditioned: there the row must carry one of the normals the point can take
    (geometry_reference.near_normals), and which one hangs on the last bit of the point."""
    worst = dict(distance=0.0, time=0.0, normal=0.0, flat_time=0.0)
    single = kind == DISCRETE
    for b, (case, r) in enumerate(zip(cases, rows)):
        name = f"{label}{case['name']}"
        units = units_of(case, kind, n_states)
        if threshold:
            assert len(r) == case["contacts"], f"{name}: {len(r)} contacts, {case['contacts']} expected"
            units = [u for u in units
                     if float(ref_static(case, u[2])[0] if u[3] is None else ref_cast(case, *u[3])[0]) < THRESHOLD]
        assert len(r) == len(units), f"{name}: {len(r)} rows, {len(units)} expected"
        last = n_states - 1
        for k, (row, (t, sub, state, cast)) in enumerate(zip(r, units)):
            other = -2 if case["prim"] is None else 0
            assert [int(v) for v in row[:5]] == [t, 3, other, 0, sub], f"{name}: keys {row[:5]}"
            T = float(row[6])
            if cast is None:
                d_ref, n_ref = ref_static(case, state)
                assert T == (0.0 if single else sub / last), f"{name}: cc_time {T!r}"
                p_eval = state
            else:
                d_ref, t_ref = ref_cast(case, *cast)
                ts = T * last - sub
                assert 0.0 <= ts <= 1.0, f"{name}: cast time {ts!r}"
                d_at, n_ref, tb = ref_at(case, ts, *cast)
                if case["t_left"] is not None and n_states == 2:
                    worst["flat_time"] = max(worst["flat_time"], abs(ts - case["t_left"]))
                    assert abs(ts - case["t_left"]) <= TOL_TIME, f"{name}: t {ts!r}, flat from {case['t_left']!r}"
                dt = abs(float(d_at - d_ref))
                worst["time"] = max(worst["time"], dt)
                assert dt <= TOL_TIME, f"{name}: distance at the returned t {ts!r} is {dt:.3e} above the minimum (at {float(t_ref)!r})"
                p_eval = np.asarray(cast[0], dtype=gr.LD) + gr.LD(ts) * (np.asarray(cast[1], dtype=gr.LD) - np.asarray(cast[0], dtype=gr.LD))
            dd = abs(float(gr.LD(row[5]) - d_ref))
            worst["distance"] = max(worst["distance"], dd)
            assert dd <= TOL_DIST, f"{name}: distance {row[5]!r} vs {float(d_ref)!r} ({dd:.3e})"
            got_a, got_b = row_normal(case, row, single)
            if case["normal"] is not None and n_states == 2 and (cast is not None or case["family"] == "static"):
                # the stated convention, exactly (one rounding of the two parts' sum)
                assert n_ref is None or not well_conditioned(case, p_eval), f"{name}: a convention where the gradient exists"
                assert np.max(np.abs(got_a - np.array(case["normal"]))) <= 2.5e-16, f"{name}: normal {got_a}, stated {case['normal']}"
            elif n_ref is not None and well_conditioned(case, p_eval):
                dn = _normal_diff(got_a, n_ref.astype(np.float64), T, single)
                if got_b is not None:
                    Tb = T if cast is None else (sub + float(tb)) / last
                    dn = max(dn, _normal_diff(got_b, n_ref.astype(np.float64), Tb, single))
                worst["normal"] = max(worst["normal"], dn)
                assert dn <= TOL_NORMAL, f"{name}: normal {got_a} vs {n_ref} ({dn:.3e})"
            else:
                if loose is not None:
                    loose.append((b, k))
                can = None if case["prim"] is None else gr.near_normals(p_eval, case["prim"])
                if can is None:
                    assert abs(np.linalg.norm(got_a) - 1.0) <= 1e-6, f"{name}: normal {got_a} is no unit vector"
                else:
                    dn = min(_normal_diff(got_a, n.astype(np.float64), T, single) for n in can)
                    assert dn <= TOL_NORMAL, f"{name}: normal {got_a} is none of {can}"
    return worst


# ------------------------------------------------------------------ the launches
# (label, cases, evaluator, make_desc arguments, check_rows arguments): one batch each
SUITES = [
    ("static-discrete", STATIC, DISCRETE, {}, {}),
    ("static-as-cast", STATIC, LVS_CONTINUOUS, {}, {}),
    ("swept-one-cast", SWEPT, LVS_CONTINUOUS, {}, {}),
    ("swept-ends", SWEPT, LVS_DISCRETE, {}, {}),
    ("self-one-cast", SELF, LVS_CONTINUOUS, {}, {}),
    ("self-ends", SELF, LVS_DISCRETE, {}, {}),
    ("self-discrete", SELF, DISCRETE, {}, {}),
    ("substate-discrete", SUBSTATE, LVS_DISCRETE, dict(lvs=SUB_LVS), dict(n_states=4)),
    ("substate-cast", SUBSTATE, LVS_CONTINUOUS, dict(lvs=SUB_LVS), dict(n_states=4)),
    ("threshold-static", THRESHOLD_STATIC_ALONE, DISCRETE, dict(margin=THR_MARGIN, buffer=THR_BUFFER),
     dict(threshold=True)),
    ("threshold-static-as-cast", THRESHOLD_STATIC, LVS_CONTINUOUS, dict(margin=THR_MARGIN, buffer=THR_BUFFER),
     dict(threshold=True)),
    ("threshold-swept", THRESHOLD_SWEPT, LVS_CONTINUOUS, dict(margin=THR_MARGIN, buffer=THR_BUFFER),
     dict(threshold=True)),
]
