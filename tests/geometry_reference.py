"""A high-precision reference of the collision geometry, independent of the
kernels' and the oracle's algorithm (tests/geometry_cases.py is its case table).

Everything is np.longdouble (a 64-bit mantissa, 1e-19) on the doubles a case
holds, from the textbook forms:

  * the signed distance of a point to a sphere, to a capsule (the clamped
    projection on its axis) and to a box, |max(|p| - h, 0)| + min(max_i(|p_i| -
    h_i), 0) in the box frame;
  * a swept minimum: the signed distance to a convex body is convex along a
    segment, so a golden-section search on [0, 1] and the two end values give
    its minimum -- no breakpoints, no candidate lists;
  * a self cast: min over s of the distance of a(s) to the other centre's
    segment, the inner parameter in closed form, the same search over s;
  * normals: the direction of the SDF's gradient at the evaluation point (per
    region), turned to the kernels' sign: from the robot sphere toward the
    primitive, d distance / d centre = -normal.

A primitive is its 16-double record (include/trajopt_hip.h THIP_PRIM_*).  The
robot sphere's radius is subtracted by the caller's `r`.
"""
import numpy as np

from trajopt_amd import abi

LD = np.longdouble
_INVPHI = (np.sqrt(LD(5)) - LD(1)) / LD(2)


def _v(a):
    return np.asarray(a, dtype=LD)


def _norm(v):
    return np.sqrt(np.sum(v * v))


def _box_frame(p, prim):
    R = _v(prim[4:13]).reshape(3, 3)
    return R.T @ (_v(p) - _v(prim[1:4])), R, _v(prim[13:16])


def _capsule_point(p, prim):
    """The point of the capsule's axis closest to p (a == b: a)."""
    a, b = _v(prim[1:4]), _v(prim[4:7])
    ab = b - a
    den = np.sum(ab * ab)
    if den == 0:
        return a
    t = min(max(np.sum((_v(p) - a) * ab) / den, LD(0)), LD(1))
    return a + t * ab


def sdf(p, prim, r=0.0):
    """Signed distance of a sphere (centre p, radius r) to the primitive's surface."""
    typ = int(prim[0])
    if typ == abi.PRIM_SPHERE:
        return _norm(_v(p) - _v(prim[1:4])) - LD(prim[4]) - LD(r)
    if typ == abi.PRIM_CAPSULE:
        return _norm(_v(p) - _capsule_point(p, prim)) - LD(prim[7]) - LD(r)
    pl, _, h = _box_frame(p, prim)
    q = np.abs(pl) - h
    return _norm(np.maximum(q, LD(0))) + min(np.max(q), LD(0)) - LD(r)


def normal(p, prim):
    """-grad sdf at p as a unit vector, or None where the gradient does not exist
    (the centre on a sphere's centre or a capsule's axis, on a box's surface, at
    equal depth to two faces): there a case states the kernels' convention."""
    typ = int(prim[0])
    if typ != abi.PRIM_BOX:
        s = _v(prim[1:4]) if typ == abi.PRIM_SPHERE else _capsule_point(p, prim)
        v = s - _v(p)
        L = _norm(v)
        return None if L == 0 else v / L
    pl, R, h = _box_frame(p, prim)
    q = np.abs(pl) - h
    if np.any(q > 0):  # outside: toward the clamped point
        g = np.where(q > 0, q * np.sign(pl), LD(0))
        return -(R @ (g / _norm(g)))
    if np.any(q == 0):
        return None
    order = np.argsort(q)
    if q[order[2]] == q[order[1]]:
        return None
    k = int(order[2])  # inside: out through the nearest face
    if pl[k] == 0:
        return None
    return -(np.sign(pl[k]) * R[:, k])


def conditioning(p, prim):
    """(distance of p to the closest point: a sphere's centre, a capsule's axis, the
    clamped point of a box when p is outside it; the gap of the two smallest of the
    six face depths when p is inside a box): the two lengths that say whether the
    normal at p is well conditioned."""
    typ = int(prim[0])
    if typ != abi.PRIM_BOX:
        s = _v(prim[1:4]) if typ == abi.PRIM_SPHERE else _capsule_point(p, prim)
        return float(_norm(s - _v(p))), np.inf
    pl, _, h = _box_frame(p, prim)
    q = np.abs(pl) - h
    if np.any(q > 0):
        return float(_norm(np.maximum(q, LD(0)))), np.inf
    d = np.sort(np.concatenate([h - pl, h + pl]))  # the six faces' depths
    return np.inf, float(d[1] - d[0])


def near_normals(p, prim, tol=1e-3):
    """Where the normal at p is not well conditioned: the normals it can take -- those of
    the box faces whose depth is within tol of the smallest when p is inside a box (which
    one depends on the last bit of p); None when any unit vector can come out (p within tol
    of the closest point itself)."""
    if int(prim[0]) != abi.PRIM_BOX:
        return None
    pl, R, h = _box_frame(p, prim)
    if np.any(np.abs(pl) - h > 0):
        return None
    depth = np.concatenate([h - pl, h + pl])  # faces +x +y +z -x -y -z
    return [-(R[:, k % 3] if k < 3 else -R[:, k % 3]) for k in range(6) if depth[k] - depth.min() <= tol]


def _golden(f, lo=LD(0), hi=LD(1), iters=100):
    """min of a convex f on [lo, hi]: (value, argument); the ends are candidates too."""
    a, b = LD(lo), LD(hi)
    c, d = b - _INVPHI * (b - a), a + _INVPHI * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(iters):
        if fc <= fd:
            b, d, fd = d, c, fc
            c = b - _INVPHI * (b - a)
            fc = f(c)
        else:
            a, c, fc = c, d, fd
            d = a + _INVPHI * (b - a)
            fd = f(d)
    best = min((fc, c), (fd, d), (f(LD(lo)), LD(lo)), (f(LD(hi)), LD(hi)), key=lambda e: (e[0], e[1]))
    return best


def swept_min(a, b, prim, r=0.0):
    """(min over t in [0, 1] of sdf(a + t (b - a)), a minimiser)."""
    a, b = _v(a), _v(b)
    return _golden(lambda t: sdf(a + t * (b - a), prim, r))


def point_segment(p, b0, b1):
    """(distance, parameter) of p to the segment b0 -> b1."""
    p, b0, b1 = _v(p), _v(b0), _v(b1)
    db = b1 - b0
    den = np.sum(db * db)
    t = LD(0) if den == 0 else min(max(np.sum((p - b0) * db) / den, LD(0)), LD(1))
    return _norm(p - (b0 + t * db)), t


def self_cast_min(a0, a1, b0, b1, ra=0.0, rb=0.0):
    """(min over (s, t) of |a(s) - b(t)| - ra - rb, s, t)."""
    a0, a1 = _v(a0), _v(a1)
    val, s = _golden(lambda s: point_segment(a0 + s * (a1 - a0), b0, b1)[0])
    return val - LD(ra) - LD(rb), s, point_segment(a0 + s * (a1 - a0), b0, b1)[1]


def self_normal_at(a0, a1, b0, b1, s, t):
    """Unit vector from a(s) to b(t)."""
    v = _v(b0) + LD(t) * (_v(b1) - _v(b0)) - (_v(a0) + LD(s) * (_v(a1) - _v(a0)))
    return v / _norm(v)
