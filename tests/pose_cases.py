"""The CartPose error's rotation edges as problems of a batch: chains whose error
rotation a case can place exactly, one case per problem.

posebot: three prismatic joints x, y, z off the base, then three revolute joints
about z, y, x; identity base pose and joint origins; the tool link is link 6.  With
the revolute joints at 0 their rotation matrices are the exact identity, so the
error pose E = (base * target)^-1 * (FK * offset) has E.R = target.R^T bit for bit
on the device, in the oracle and in the reference: a case states E.R as a double
matrix and every side takes the logarithm of those very bits.  With an identity
target E.t = q[:3] bit for bit, which puts a translation component on a band edge.
tiltbot: the same six joints with a rotated base pose, rotated joint origins, the
middle revolute axis oblique ((-2, 1, 2) / 3 as rounded to double), and a source
offset with a rotation and a translation: nothing is exact there, every product
rounds.  posebot_dyn: posebot as a DynamicCartPose term whose target link is the
first revolute link (link 4), so the joints 0..3 move both frames.

A case is a dict: name, family, chain, band (a key of BANDS), offset (a key of
OFFSETS), q[6], target[12] and what the family states about it:
  branch      family 2: (Shoemake branch 'w' / 0 / 1 / 2, sign of Eigen's w)
  rot_exact   families 1, 3: the rotation error, bit for bit
  rot_signs   family 3's tied diagonal: the signs of the rotation error
  zero_exact  family 6: components that must be exactly 0 (on a band edge)
  either_sign the `*_pi_inexact` cases: a rotation by pi on a matrix that is not exactly
              symmetric -- rounding noise picks v or -v, both are accepted (at most 4)
  jump        family 8: the dofs whose untoleranced Jacobian columns (rows >= 3) carry
              the 2 pi / eps jump of the [0, 2 pi] form's seam
  column      family 6: (row, dof, value) of an FD column that straddles a band edge
Tolerance bands and the source offset live in the descriptor, so BATCHES groups the
cases by (chain, band, offset), at most 64 to a batch (the untoleranced posebot
cases take two).  tests/test_pose_reference.py validates every entry against
tests/pose_reference.py and the oracle on the CPU.
"""
import math

import numpy as np

import pose_reference as pr
from geometry_cases import ROT
from trajopt_amd import abi, problems, robots

PI = math.pi
POS_W, ROT_W = (1.0, 2.0, 0.5), (0.25, 4.0, 1.5)
WEIGHTS = np.array(POS_W + ROT_W)
TOOL, DYN_TARGET = 6, 4
OBLIQUE = (-2.0 / 3.0, 1.0 / 3.0, 2.0 / 3.0)  # |a0| == |a2| bitwise: a rotation about it ties R00 and R22
LIMIT = 200.0

TOL_ERR, TOL_JAC = 1e-12, 1e-9  # tests/test_gpu.py's bars, absolute
TOL_VALUE = 6 * WEIGHTS.max() * 1e-12

BANDS = {
    "none": None,
    "sym": (np.array([-0.02] * 3 + [-0.1] * 3), np.array([0.02] * 3 + [0.1] * 3)),
    "asym": (np.full(6, -0.1), np.full(6, 0.3)),
    "zero": (np.zeros(6), np.zeros(6)),
    "wide": (np.full(6, -0.5), np.full(6, 0.5)),
}


def pose12(R=None, t=(0.0, 0.0, 0.0)):
    T = np.zeros((3, 4))
    T[:, :3] = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
    T[:, 3] = t
    return T.reshape(12)


IDENT = pose12()
OFFSETS = {"ident": IDENT, "off": pose12(ROT.T, (0.05, -0.02, 0.03))}


def rot(axis, angle):
    """Eigen's AngleAxis::toRotationMatrix in double: the matrix a caller would upload."""
    return robots._axis_angle(axis, angle)


# ------------------------------------------------------------------ chains
def _chain(base12, joints):
    """joints: (type, origin[12], axis) for links 1.., a serial chain."""
    c = abi.Chain()
    c.n_links = len(joints) + 1
    c.is_tree = 0
    for i in range(12):
        c.base_pose[i] = base12[i]
    c.joint_dof[0] = -1
    for k, (jt, origin, axis) in enumerate(joints, start=1):
        c.parent[k] = k - 1
        c.joint_type[k] = jt
        c.joint_dof[k] = k - 1
        for i in range(12):
            c.joint_origin[k][i] = origin[i]
        for i in range(3):
            c.joint_axis[k][i] = axis[i]
        c.lower[k - 1], c.upper[k - 1] = -LIMIT, LIMIT
    c.n_dof = len(joints)
    return c


def posebot_chain():
    P, R = abi.JOINT_PRISMATIC, abi.JOINT_REVOLUTE
    return _chain(IDENT, [(P, IDENT, (1, 0, 0)), (P, IDENT, (0, 1, 0)), (P, IDENT, (0, 0, 1)),
                          (R, IDENT, (0, 0, 1)), (R, IDENT, (0, 1, 0)), (R, IDENT, (1, 0, 0))])


def tiltbot_chain():
    P, R = abi.JOINT_PRISMATIC, abi.JOINT_REVOLUTE
    return _chain(pose12(ROT, (0.3, -0.2, 0.5)),
                  [(P, pose12(ROT, (0.1, 0.0, -0.05)), (1, 0, 0)), (P, IDENT, (0, 1, 0)),
                   (P, pose12(ROT.T, (0.0, 0.2, 0.0)), (0, 0, 1)), (R, pose12(ROT @ ROT, (0.05, 0.1, 0.0)), (0, 0, 1)),
                   (R, pose12(None, (0.0, 0.0, 0.15)), OBLIQUE), (R, pose12(ROT.T, (0.2, -0.1, 0.05)), (1, 0, 0))])


CHAINS = {"posebot": posebot_chain(), "tiltbot": tiltbot_chain(), "posebot_dyn": posebot_chain()}


def target_link(chain_name):
    return DYN_TARGET if chain_name == "posebot_dyn" else 0


# ------------------------------------------------------------------ cases
Q_PRIS = (0.125, -0.25, 0.5)


def _case(name, family, chain, q, target, band="none", offset="ident", **kw):
    q = np.asarray(q, dtype=np.float64)
    target = np.asarray(target, dtype=np.float64)
    assert q.shape == (6,) and target.shape == (12,)
    q.setflags(write=False)
    target.setflags(write=False)
    return dict(name=name, family=family, chain=chain, q=q, target=target, band=band, offset=offset, **kw)


def _at(E_R, q_pris=Q_PRIS, t=(0.0, 0.0, 0.0)):
    """posebot at revolute 0 against the target whose transpose is E_R: (q, target)."""
    return tuple(q_pris) + (0.0, 0.0, 0.0), pose12(np.asarray(E_R).T, t)


AXES7 = [("px", (1, 0, 0)), ("mx", (-1, 0, 0)), ("py", (0, 1, 0)), ("my", (0, -1, 0)), ("pz", (0, 0, 1)),
         ("mz", (0, 0, -1)), ("oblique", OBLIQUE)]


def _zero_and_tiny():
    out = [_case("identity", "tiny", "posebot", *_at(np.eye(3)), rot_exact=(0.0, 0.0, 0.0))]
    for ang in (1e-200, 1e-17, 1e-12, 1e-9):
        for an, ax in AXES7:
            out.append(_case(f"tiny_{ang:g}_{an}", "tiny", "posebot", *_at(rot(ax, ang))))
    return out


DOMINANT = [(0, +1, (0.8, 0.36, 0.48)), (0, -1, (-0.8, 0.36, 0.48)), (1, +1, (0.48, 0.8, 0.36)),
            (1, -1, (0.48, -0.8, 0.36)), (2, +1, (0.36, 0.48, 0.8)), (2, -1, (0.36, 0.48, -0.8))]
BRANCH_ANGLES = [("below_120", 2 * PI / 3 - 1e-3), ("above_120", 2 * PI / 3 + 1e-3), ("2.5", 2.5),
                 ("pi_m1e-5", PI - 1e-5), ("pi_m1e-9", PI - 1e-9)]


def _branches():
    out = []
    for tn, th in BRANCH_ANGLES:
        for i, sg, ax in DOMINANT:
            branch = ("w", +1) if th < 2 * PI / 3 else (i, sg)
            out.append(_case(f"branch_{tn}_{'xyz'[i]}{'p' if sg > 0 else 'm'}", "branches", "posebot",
                             *_at(rot(ax, th)), branch=branch))
    return out


def _exactly_pi():
    pid = float(np.float64(PI))
    tied = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
    a = np.ones(3) / math.sqrt(3.0)
    return [
        _case("pi_about_x", "pi", "posebot", *_at(np.diag([1.0, -1.0, -1.0])), rot_exact=(pid, 0.0, 0.0)),
        _case("pi_about_y", "pi", "posebot", *_at(np.diag([-1.0, 1.0, -1.0])), rot_exact=(0.0, pid, 0.0)),
        _case("pi_about_z", "pi", "posebot", *_at(np.diag([-1.0, -1.0, 1.0])), rot_exact=(0.0, 0.0, pid)),
        # a tied diagonal (0, 0, -1): the first arg-max is x, the axis (1, 1, 0) / sqrt 2
        _case("pi_tied_diagonal", "pi", "posebot", *_at(tied), rot_signs=(1, 1, 0)),
        _case("a111_pi_inexact", "pi", "posebot", *_at(2.0 * np.outer(a, a) - np.eye(3)), either_sign=True),
    ]


JOINT_ANGLES = [("pi_m1e-9", PI - 1e-9), ("pi", PI), ("pi_p1e-9", PI + 1e-9), ("3.5", 3.5), ("5.0", 5.0),
                ("m3.0", -3.0), ("2pi", 2 * PI), ("2pi_p1e-9", 2 * PI + 1e-9), ("100", 100.0)]


def _tilt_target(q, D, offset="off"):
    """The tiltbot target at which the error rotation at q is D (to rounding): base^-1 FK(q) offset D^-1."""
    ch = CHAINS["tiltbot"]
    S = pr.fk(ch, q, TOOL) @ pr.pose44(OFFSETS[offset])
    Dm = np.eye(4, dtype=pr.LD)
    Dm[:3, :3] = np.asarray(D, dtype=pr.LD)
    T = pr.inverse(pr.pose44(ch.base_pose)) @ S @ pr.inverse(Dm)
    return np.asarray(T[:3, :], dtype=np.float64).reshape(12)


TILT_Q0 = (0.125, -0.25, 0.5, 0.0, 0.0, 0.37)  # the x joint off 0: the oblique joint's axis is in general position in E


def _beyond_pi():
    out = []
    tilt_home = _tilt_target(TILT_Q0, np.eye(3))
    for an, ang in JOINT_ANGLES:
        out.append(_case(f"joint_z_{an}", "joint", "posebot", Q_PRIS + (ang, 0.0, 0.0), IDENT))
        q = TILT_Q0[:4] + (ang, TILT_Q0[5])
        if an == "pi":
            # sin(pi as a double) = 1.2e-16 is the size of tiltbot's rounding: v or -v
            out.append(_case("tilt_joint_pi_inexact", "joint", "tiltbot", q, tilt_home, offset="off", either_sign=True))
        else:
            out.append(_case(f"tilt_joint_oblique_{an}", "joint", "tiltbot", q, tilt_home, offset="off"))
    for an, ang in JOINT_ANGLES[3:6]:
        out.append(_case(f"joint_y_{an}", "joint", "posebot", Q_PRIS + (0.0, ang, 0.0), IDENT))
        out.append(_case(f"joint_x_{an}", "joint", "posebot", Q_PRIS + (0.1, -0.2, ang), IDENT))
        out.append(_case(f"tilt_joint_z_{an}", "joint", "tiltbot", TILT_Q0[:3] + (ang, 0.3, -0.2), tilt_home, offset="off"))
    return out


def _translation():
    tgt = pose12(ROT, (6.0, -8.0, 0.5))  # 10 m from the origin
    tgt2 = pose12(rot(OBLIQUE, 2.0), (-8.0, 0.5, 6.0))
    out = [
        _case("far_target", "translation", "posebot", (6.01, -8.02, 0.53, 0.3, -0.2, 0.1), tgt, offset="off"),
        _case("far_target_2", "translation", "posebot", (-7.9, 0.45, 6.1, -1.0, 0.4, 2.0), tgt2, offset="off"),
        _case("near_target", "translation", "posebot", (0.01, -0.02, 0.03, 0.3, -0.2, 0.1), pose12(ROT, (0.05, 0.0, 0.0)),
              offset="off"),
    ]
    q = (6.0, -8.0, 0.5, 0.3, -0.2, 0.1)
    D = rot((0.36, 0.48, 0.8), 0.7)
    far = _tilt_target(q, D)
    far[3::4] += (0.01, -0.02, 0.03)
    out.append(_case("tilt_far_target", "translation", "tiltbot", q, far, offset="off"))
    q2 = (-8.0, 0.5, 6.0, -1.0, 0.4, 2.0)
    far2 = _tilt_target(q2, rot((-0.8, 0.36, 0.48), 2.5))
    far2[3::4] += (-0.03, 0.01, 0.02)
    out.append(_case("tilt_far_target_2", "translation", "tiltbot", q2, far2, offset="off"))
    return out


def _bands():
    """Identity target on posebot: err[:3] is q[:3] bit for bit, so a component sits on a
    band edge exactly (the edge's own double; no arithmetic touches it), one ulp outside
    or one ulp inside.  A rotation component comes out of a logarithm, which no input
    places to the ulp: it sits 1e-9 inside or outside, and on the degenerate band's edge
    as E.R = I (exactly 0) and 1e-200 outside."""
    out = []
    base = np.array([0.05, -0.15, 0.4, 0.0, 0.0, 0.0])
    for band, comp in (("sym", 0), ("asym", 1), ("zero", 2)):
        lo, hi = BANDS[band]
        for en, bound, outward in (("lower", lo[comp], -np.inf), ("upper", hi[comp], np.inf)):
            for pn, v in (("on", bound), ("ulp_outside", np.nextafter(bound, outward)),
                          ("ulp_inside", np.nextafter(bound, -outward))):
                if band == "zero" and pn == "ulp_inside":
                    continue  # lower == upper: the band has no inside
                if band == "zero" and en == "upper" and pn == "on":
                    continue  # the same point as the lower edge
                q = base.copy()
                q[comp] = v
                kw = dict(zero_exact=(comp,)) if pn != "ulp_outside" else dict(excess=(comp, float(v - bound)))
                out.append(_case(f"band_{band}_t{'xyz'[comp]}_{en}_{pn}", "bands", "posebot", q, IDENT, band=band, **kw))
        # a rotation component about axis `comp`, 1e-9 inside and outside each edge
        ax = np.eye(3)[comp]
        for en, bound, outward in (("lower", lo[3 + comp], -1.0), ("upper", hi[3 + comp], 1.0)):
            if band == "zero":
                continue
            for pn, d in (("inside", -1e-9), ("outside", 1e-9)):
                out.append(_case(f"band_{band}_r{'xyz'[comp]}_{en}_{pn}", "bands", "posebot",
                                 *_at(rot(ax, bound + outward * d), base[:3]), band=band))
    out.append(_case("band_zero_rot_on_edge", "bands", "posebot", *_at(np.eye(3), base[:3]), band="zero",
                     zero_exact=(3, 4, 5)))
    for an, ax in AXES7[4:]:
        out.append(_case(f"band_zero_rot_1e-200_{an}", "bands", "posebot", *_at(rot(ax, 1e-200), base[:3]), band="zero"))
    # an FD step that leaves the band: e0 inside, 4e-6 under the upper bound, e1 6e-6 outside
    q = base.copy()
    q[0] = 0.02 - 4e-6
    out.append(_case("band_sym_fd_leaves_tx", "bands", "posebot", q, IDENT, band="sym", column=(0, 0, 0.6)))
    q = base.copy()
    q[1] = 0.3 - 4e-6
    out.append(_case("band_asym_fd_leaves_ty", "bands", "posebot", q, IDENT, band="asym", column=(1, 1, 0.6)))
    q = base.copy()
    q[3] = 0.1 - 4e-6
    out.append(_case("band_sym_fd_leaves_rz", "bands", "posebot", q, IDENT, band="sym", column=(5, 3, 0.6)))
    q = base.copy()
    q[2] = -4e-6
    out.append(_case("band_zero_fd_crosses_tz", "bands", "posebot", q, IDENT, band="zero", column=(2, 2, 1.0)))
    return out


WRAP_ANGLES = [("pi_m1e-3", PI - 1e-3), ("pi_m5e-6", PI - 5e-6), ("pi_p1e-3", PI + 1e-3)]


def _wrap(band):
    """The error rotation about a joint's own axis next to pi: in the middle case the step
    of 1e-5 carries it over pi.  posebot: about z (dof 3) at all three angles, about y and
    x in the middle one; posebot_dyn: about y (dof 4), the first joint that moves the
    source alone, and about x."""
    out = []
    ex, ey, ez = np.eye(3)
    for an, ang in WRAP_ANGLES:
        out.append(_case(f"wrap_{band}_z_{an}", "wrap", "posebot", *_at(rot(ez, ang)), band=band))
        q, tgt = _at(rot(ey, ang), t=(0.02, -0.01, 0.03))
        out.append(_case(f"dyn_wrap_{band}_y_{an}", "wrap", "posebot_dyn", q, tgt, band=band))
    out.append(_case(f"wrap_{band}_y_pi_m5e-6", "wrap", "posebot", *_at(rot(ey, PI - 5e-6)), band=band))
    out.append(_case(f"wrap_{band}_x_pi_m5e-6", "wrap", "posebot", *_at(rot(ex, PI - 5e-6)), band=band))
    out.append(_case(f"wrap_{band}_z_by_joint", "wrap", "posebot", Q_PRIS + (PI - 5e-6, 0.0, 0.0), IDENT, band=band))
    q, tgt = _at(rot(ex, PI - 5e-6), t=(0.02, -0.01, 0.03))
    out.append(_case(f"dyn_wrap_{band}_x_pi_m5e-6", "wrap", "posebot_dyn", q, tgt, band=band))
    return out


def _seam(band):
    """The [0, 2 pi] form's seam at trace = 0 (120 degrees) where the axis component on the
    largest diagonal entry is negative.  The y joint (dof 4) carries E over it: about -y,
    E(q + eps) = rot(-y, theta - eps); about the oblique axis the trace falls by 0.577 eps.
    Untoleranced the columns of dof 4 jump by 2 pi / eps; toleranced they are smooth."""
    jump = dict(jump=(4,)) if band == "none" else {}
    tied_jump = dict(jump=(3, 5)) if band == "none" else {}
    ym, yp = (0.0, -1.0, 0.0), (0.0, 1.0, 0.0)
    c120 = 2 * PI / 3
    return [
        _case(f"seam_{band}_my_straddle", "seam", "posebot", *_at(rot(ym, c120 + 5e-6)), band=band, **jump),
        _case(f"seam_{band}_my_below", "seam", "posebot", *_at(rot(ym, c120 - 1e-3)), band=band),
        _case(f"seam_{band}_my_above", "seam", "posebot", *_at(rot(ym, c120 + 1e-3)), band=band),
        _case(f"seam_{band}_oblique_straddle", "seam", "posebot", *_at(rot(OBLIQUE, c120 - 1.5e-6)), band=band, **jump),
        # beyond trace = 0 with R00 == R22 bitwise: the first arg-max (x, negative) decides for E
        # itself.  The seam runs on wherever the arg-max changes between components of opposite
        # sign: the steps of the z and x joints move it to z (positive), so their columns jump
        _case(f"seam_{band}_oblique_tied_diagonal", "seam", "posebot", *_at(rot(OBLIQUE, c120 + 1e-3)), band=band,
              tied=(0, 2), **tied_jump),
        # the control: the same angles about +y
        _case(f"seam_{band}_py_straddle", "seam", "posebot", *_at(rot(yp, c120 - 5e-6)), band=band),
        _case(f"seam_{band}_py_below", "seam", "posebot", *_at(rot(yp, c120 - 1e-3)), band=band),
        _case(f"seam_{band}_py_above", "seam", "posebot", *_at(rot(yp, c120 + 1e-3)), band=band),
    ]


def _tilt_general():
    """tiltbot in general position on each side of the branch and band boundaries."""
    out = []
    q = (0.3, -0.1, 0.2, 0.4, -0.7, 1.1)
    for i, sg, ax in DOMINANT:
        for tn, th in BRANCH_ANGLES[:4]:
            tgt = _tilt_target(q, rot(ax, th))
            tgt[3::4] += (0.03, -0.01, 0.015)
            out.append(_case(f"tilt_branch_{tn}_{'xyz'[i]}{'p' if sg > 0 else 'm'}", "branches", "tiltbot", q, tgt,
                             offset="off"))
    for n, (ax, th) in enumerate([((0.8, 0.36, 0.48), 0.05), ((0.36, 0.48, -0.8), 0.15), ((0.48, -0.8, 0.36), 0.3),
                                  (OBLIQUE, 0.12)]):
        tgt = _tilt_target(q, rot(ax, th))
        tgt[3::4] += np.array([(0.01, -0.03, 0.05), (0.025, 0.015, -0.01), (-0.05, 0.01, 0.019), (0.0, 0.021, -0.03)][n])
        out.append(_case(f"tilt_band_sym_{n}", "bands", "tiltbot", q, tgt, band="sym", offset="off"))
    return out


CASES = (_zero_and_tiny() + _branches() + _exactly_pi() + _beyond_pi() + _translation() + _bands()
         + _wrap("none") + _wrap("wide") + _seam("none") + _seam("zero") + _tilt_general())
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _batches():
    """(label, chain, band, offset, cases): one per (chain, band, offset), split at 64."""
    groups = {}
    for c in CASES:
        groups.setdefault((c["chain"], c["band"], c["offset"]), []).append(c)
    out = []
    for (chain, band, offset), cases in groups.items():
        n = (len(cases) + 63) // 64
        per = (len(cases) + n - 1) // n
        for i in range(n):
            label = f"{chain}-{band}-{offset}" + (f"-{i + 1}" if n > 1 else "")
            out.append((label, chain, band, offset, cases[i * per:(i + 1) * per]))
    return out


BATCHES = _batches()
BATCH_IDS = [b[0] for b in BATCHES]


# ------------------------------------------------------------------ descriptors
def make_desc(chain, band, offset, is_cnt=False, n_steps=2):
    """A config A descriptor (one CartPose term) with the chain swapped in: the term at step 0
    on the tool link with all six coefficients non-zero, no fixed step, no spheres, no scene."""
    d = abi.ProblemDesc.from_buffer_copy(problems.make_workload("A", 1, n_steps=n_steps, robot="right_arm_6dof").desc)
    d.chain = CHAINS[chain]
    d.n_fixed = 0
    assert d.n_cart == 1 and d.coll_enabled == 0 and d.n_spheres == 0 and d.n_prims == 0
    d.cart_step[0] = 0
    d.cart_is_cnt[0] = 1 if is_cnt else 0
    d.cart_source_link[0] = TOOL
    d.cart_target_link[0] = target_link(chain)
    for i in range(12):
        d.cart_source_offset[0][i] = OFFSETS[offset][i]
    for i in range(3):
        d.cart_pos_coeffs[0][i], d.cart_rot_coeffs[0][i] = POS_W[i], ROT_W[i]
    d.cart_has_tol[0] = 0 if BANDS[band] is None else 1
    for i in range(6):
        d.cart_lower_tol[0][i] = 0.0 if BANDS[band] is None else BANDS[band][0][i]
        d.cart_upper_tol[0][i] = 0.0 if BANDS[band] is None else BANDS[band][1][i]
    return d


def make_workload(batch, is_cnt=False):
    """The batch as one workload: problem k is cases[k], at both of its two waypoints."""
    _, chain, band, offset, cases = batch
    d = make_desc(chain, band, offset, is_cnt)
    x = np.array([[c["q"], c["q"]] for c in cases], dtype=np.float64)
    tg = np.array([[c["target"]] for c in cases], dtype=np.float64)
    return problems.Workload("pose", d, x, tg, np.zeros((len(cases), 0, 16)), x.copy())


# ------------------------------------------------------------------ the reference's answers
_REF = {}


def reference(batch):
    """(err [B, 6], jac [B, 6, D]) of a batch in long double, made once and shared."""
    label, chain, band, offset, cases = batch
    if label not in _REF:
        ch = CHAINS[chain]
        out = [pr.linearize(ch, c["q"], TOOL, OFFSETS[offset], target_link(chain), c["target"], BANDS[band]) for c in cases]
        err, jac = np.array([o[0] for o in out]), np.array([o[1] for o in out])
        err.setflags(write=False)
        jac.setflags(write=False)
        _REF[label] = (err, jac)
    return _REF[label]


def check_case(c, e, J, e_ref, j_ref, name):
    """One case's err [6] and jac [6, D] (or None) against the reference's under the bars,
    and the conventions the case states, exactly.  Returns the gaps (error, jacobian)."""
    e = np.asarray(e, dtype=np.float64)
    assert np.all(np.isfinite(e)), f"{name}: err {e}"
    want = e_ref
    if c.get("either_sign") and np.abs(e[3:].astype(pr.LD) + want[3:]).max() < np.abs(e[3:].astype(pr.LD) - want[3:]).max():
        want = np.concatenate([want[:3], -want[3:]])
    ge = float(np.abs(e.astype(pr.LD) - want).max())
    assert ge <= TOL_ERR, f"{name}: err {e} vs {want.astype(np.float64)} ({ge:.3e})"
    if "rot_exact" in c:
        assert np.array_equal(e[3:], np.array(c["rot_exact"])), f"{name}: rotation error {e[3:]!r}, stated {c['rot_exact']}"
    if "rot_signs" in c:
        assert np.array_equal(np.sign(e[3:]), np.array(c["rot_signs"])), f"{name}: rotation error {e[3:]!r}"
    for i in c.get("zero_exact", ()):
        assert e[i] == 0.0, f"{name}: err[{i}] = {e[i]!r} on or inside the band's edge"
    if "excess" in c:
        i, v = c["excess"]
        assert e[i] == v, f"{name}: err[{i}] = {e[i]!r}, one ulp outside is {v!r}"
    gj = 0.0
    if J is not None:
        J = np.asarray(J, dtype=np.float64)
        assert np.all(np.isfinite(J)), f"{name}: jac {J}"
        gj = float(np.abs(J.astype(pr.LD) - j_ref).max())
        assert gj <= TOL_JAC, f"{name}: jac gap {gj:.3e}\n{J}\nvs\n{j_ref.astype(np.float64)}"
    return ge, gj


def check(batch, err, jac, label):
    """err [B, 6] and jac [B, 6, D] (or None) of a batch against the reference; returns the
    worst gaps (error, jacobian)."""
    cases = batch[4]
    e_ref, j_ref = reference(batch)
    gaps = [check_case(c, err[b], None if jac is None else jac[b], e_ref[b], j_ref[b], f"{label}/{c['name']}")
            for b, c in enumerate(cases)]
    return [max(g[0] for g in gaps), max(g[1] for g in gaps)]


def failing(batch, err, jac):
    """The names of the batch's cases that check_case refuses."""
    e_ref, j_ref = reference(batch)
    out = []
    for b, c in enumerate(batch[4]):
        try:
            check_case(c, err[b], jac[b], e_ref[b], j_ref[b], c["name"])
        except AssertionError:
            out.append(c["name"])
    return out


def ref_values(batch, is_cnt, err=None):
    """The term's value per problem from the reference's error (or from a given one)."""
    e = reference(batch)[0] if err is None else err
    return np.array([pr.value(e[b], WEIGHTS, is_cnt) for b in range(len(e))])
