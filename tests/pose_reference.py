"""A high-precision reference of the CartPose error and its forward-difference
Jacobian, independent of the kernels' and the oracle's branch structure
(tests/pose_cases.py is its case table).

Everything is np.longdouble (a 64-bit mantissa, 1e-19) on the doubles a case
holds:

  * FK: the product of the chain's double matrices as they stand; a revolute joint
    by Rodrigues' formula c I + s [a]x + (1 - c) a a^T on the axis as given (not
    renormalised); the inverse of a pose is (R^T, -R^T t).
  * the rotation logarithm: of the four quaternion candidates (w^2, x^2, y^2, z^2
    from the diagonal) the one with the largest pivot, the other three from the
    off-diagonal sums and differences, the sign turned to w >= 0;
    theta = 2 atan2(|v|, w), the rotation vector (v / |v|) theta.
  * the two conventions, as mathematics:
      [-pi, pi]   that vector.  At w == 0 exactly (theta = pi on an exactly symmetric
                  matrix) v and -v are the same rotation: the one whose component at
                  the first arg-max of the diagonal is positive (Eigen's w is +0).
      [0, 2 pi]   that vector when Eigen's w >= 0, otherwise (-a)(2 pi - theta).
                  Eigen's quaternion has w > 0 where the trace is positive and
                  otherwise its component at the first arg-max of the diagonal
                  positive: the sign of the trace and that index, both read off the
                  matrix rounded to double, are all that decide.
  * bands: e - lower below the band, e - upper above it, 0 inside and on its edges.
  * the forward difference: eps = 1e-5, q[p] + eps rounded to double; untoleranced
    the [0, 2 pi] form on both sides; toleranced the [-pi, pi] form on both sides,
    or the [0, 2 pi] form on both when a rotation component differs by more than pi,
    banded, then differenced.
  * values: a cost is sum |err_i| w_i, a constraint's violation sum |err_i w_i|.

`dtype=np.float64` runs the same FK in double: tests/test_pose_reference.py hangs
its double restatement of the kernels' branches (and the mutations of it) on those
matrices.
"""
import numpy as np

from trajopt_amd import abi

LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")
EPS = np.float64(1e-5)


def pose44(p12, dtype=LD):
    T = np.eye(4, dtype=dtype)
    T[:3, :] = np.asarray(list(p12), dtype=np.float64).reshape(3, 4).astype(dtype)
    return T


def rodrigues(axis, angle, dtype=LD):
    a = np.asarray(axis, dtype=dtype)
    th = dtype(angle)
    s, c = np.sin(th), np.cos(th)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=dtype)
    return c * np.eye(3, dtype=dtype) + s * K + (dtype(1) - c) * np.outer(a, a)


def inverse(T):
    out = np.eye(4, dtype=T.dtype)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def fk(chain, q, link, dtype=LD):
    """World pose of `link` at the joint values q: the joints on its path from the root."""
    path = []
    k = link
    while k > 0:
        path.append(k)
        k = chain.parent[k]
    T = pose44(chain.base_pose, dtype)
    for k in reversed(path):
        T = T @ pose44(chain.joint_origin[k], dtype)
        jt = chain.joint_type[k]
        if jt in (abi.JOINT_REVOLUTE, abi.JOINT_CONTINUOUS):
            M = np.eye(4, dtype=dtype)
            M[:3, :3] = rodrigues(list(chain.joint_axis[k]), np.float64(q[chain.joint_dof[k]]), dtype)
            T = T @ M
        elif jt == abi.JOINT_PRISMATIC:
            M = np.eye(4, dtype=dtype)
            M[:3, 3] = np.asarray(list(chain.joint_axis[k]), dtype=dtype) * dtype(np.float64(q[chain.joint_dof[k]]))
            T = T @ M
    return T


def error_pose(chain, q, src_link, src_off, tgt_link, tgt_off, dtype=LD):
    """E = (target frame)^-1 (source frame): the pose whose translation and rotation
    logarithm are the error."""
    Ss = fk(chain, q, src_link, dtype) @ pose44(src_off, dtype)
    Tb = fk(chain, q, tgt_link, dtype) if tgt_link > 0 else pose44(chain.base_pose, dtype)
    return inverse(Tb @ pose44(tgt_off, dtype)) @ Ss


# ------------------------------------------------------------------ the logarithm
def quaternion(R):
    """(w, v) of R with w >= 0, from the candidate with the largest pivot."""
    R = np.asarray(R, dtype=LD)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    piv = [LD(1) + tr] + [LD(1) + 2 * R[i, i] - tr for i in range(3)]
    m = int(np.argmax(piv))
    s = 2 * np.sqrt(piv[m])  # 4 |q_m|
    q = np.zeros(4, dtype=LD)
    if m == 0:
        q[0] = s / 4
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s
    else:
        i = m - 1
        j, k = (i + 1) % 3, (i + 2) % 3
        q[1 + i] = s / 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    if q[0] < 0:
        q = -q
    return q[0], q[1:]


def eigen_w_nonneg(R, w, v):
    """Whether Eigen's quaternion of R has w >= 0 (given the canonical (w, v), w >= 0):
    decided by the sign of the trace and the first arg-max of the diagonal of R as
    rounded to double."""
    Rd = np.asarray(R, dtype=np.float64).astype(LD)
    if Rd[0, 0] + Rd[1, 1] + Rd[2, 2] > 0:
        return True, None
    i = first_argmax(np.diag(Rd))
    return bool(w == 0 or v[i] > 0), i


def first_argmax(d):
    i = 0
    if d[1] > d[0]:
        i = 1
    if d[2] > d[i]:
        i = 2
    return i


def rotvec(R):
    """(the [-pi, pi] form, the [0, 2 pi] form) of the rotation vector of R."""
    w, v = quaternion(R)
    n = np.sqrt(np.sum(v * v))
    if n == 0:
        z = np.zeros(3, dtype=LD)
        return z, z.copy()
    nonneg, i = eigen_w_nonneg(R, w, v)
    if w == 0 and i is not None and v[i] < 0:
        v = -v  # theta = pi exactly: v and -v are one rotation, the convention picks
    theta = 2 * np.arctan2(n, w)
    a = v / n
    pm = a * theta
    return pm, (pm if nonneg else (-a) * (2 * PI - theta))


def exp(rv):
    rv = np.asarray(rv, dtype=LD)
    th = np.sqrt(np.sum(rv * rv))
    if th == 0:
        return np.eye(3, dtype=LD)
    return rodrigues(rv / th, th)


# ------------------------------------------------------------------ bands, error, FD, values
def bands(e, lower, upper):
    e = np.asarray(e, dtype=LD)
    lo, hi = np.asarray(lower, dtype=LD), np.asarray(upper, dtype=LD)
    return np.where(e < lo, e - lo, np.where(e > hi, e - hi, LD(0)))


def error(E, band=None):
    """err[6] of the error pose E: translation, then the [-pi, pi] rotation vector; banded."""
    e = np.concatenate([E[:3, 3], rotvec(E[:3, :3])[0]])
    return e if band is None else bands(e, *band)


def fd_column(E0, E1, band=None):
    """(banded error at E1) - (banded error at E0) as the Jacobian calculators take it."""
    pm0, tp0 = rotvec(E0[:3, :3])
    pm1, tp1 = rotvec(E1[:3, :3])
    if band is None:
        return np.concatenate([E1[:3, 3] - E0[:3, 3], tp1 - tp0])
    r0, r1 = (tp0, tp1) if np.any(np.abs(pm1 - pm0) > PI) else (pm0, pm1)
    e0 = bands(np.concatenate([E0[:3, 3], r0]), *band)
    e1 = bands(np.concatenate([E1[:3, 3], r1]), *band)
    return e1 - e0


def perturbed(q, p):
    qp = np.array(q, dtype=np.float64)
    qp[p] = np.float64(qp[p] + EPS)
    return qp


def linearize(chain, q, src_link, src_off, tgt_link, tgt_off, band=None):
    """err [6] and the forward-difference Jacobian [6, D] (long double)."""
    D = chain.n_dof
    E0 = error_pose(chain, q, src_link, src_off, tgt_link, tgt_off)
    J = np.zeros((6, D), dtype=LD)
    for p in range(D):
        E1 = error_pose(chain, perturbed(q, p), src_link, src_off, tgt_link, tgt_off)
        J[:, p] = fd_column(E0, E1, band) / LD(EPS)
    return error(E0, band), J


def value(err, weights, is_cnt):
    """A cost's value sum |err_i| w_i, a constraint's violation sum |err_i w_i|."""
    e, w = np.asarray(err, dtype=LD), np.asarray(weights, dtype=LD)
    return np.sum(np.abs(e * w)) if is_cnt else np.sum(np.abs(e) * w)
