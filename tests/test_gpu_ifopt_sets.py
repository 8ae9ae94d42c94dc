"""trajopt_ifopt's fixed-size discrete collision sets (thip_csets_*,
coll_sets.hip) and CartPos sets (thost_tsqp_eval_kin) on the GPU.

Collision sets are checked against a numpy restatement of the selection rule
written here (expected_sets): the candidates' distances, normals and contact
points come from oracle.sphere_prim (self pairs: the closed form of two
spheres), their gradients from a numpy geometric jacobian over robots.fwd_kin,
and both are tied to oracle.collision_rows on a DISCRETE descriptor (distance
within 1e-12, the linearised row a_t within the oracle's own 1e-7 clean-up of
small coefficients, which is why a_t itself is not the reference).  Values and
rows agree within 1e-12 x the coefficient scale (tests/test_gpu_terms.py's
tolerance for collision slots); keys and counts are exact.
"""
import functools

import numpy as np
import pytest

from trajopt_amd import abi, problems, robots, tsqp
from trajopt_amd.runtime import CollisionSets, HipError, TermEvaluator

pytestmark = pytest.mark.gpu

TOL = 1e-12


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


# ------------------------------------------------------------------ numpy model
def link_jacobian(chain, T, link, point):
    """Linear jacobian [3, D] of world point `point` rigidly attached to `link`."""
    J = np.zeros((3, chain.n_dof))
    k = link
    while k > 0:
        jt = chain.joint_type[k]
        if jt != abi.JOINT_FIXED:
            a = T[k][:3, :3] @ np.array(list(chain.joint_axis[k]))
            J[:, chain.joint_dof[k]] = a if jt == abi.JOINT_PRISMATIC else np.cross(a, point - T[k][:3, 3])
        k = chain.parent[k] if chain.is_tree else k - 1
    return J


def self_pairs(desc):
    """(sphere a, sphere b) of the enabled self-collision link pairs."""
    out = []
    for k in range(desc.n_self_pairs):
        a, b = desc.self_pair[k][0], desc.self_pair[k][1]
        out += [(i, j) for i in range(desc.n_spheres) if desc.sphere_link[i] == a
                for j in range(desc.n_spheres) if desc.sphere_link[j] == b]
    return out


def candidates(oracle_mod, desc, scene, q):
    """Every candidate at joint values q: (key, pair, distance, d distance / dq, both links active)."""
    ch = desc.chain
    T = robots.fwd_kin(ch, q)
    ctr = [T[desc.sphere_link[s]][:3, :3] @ np.array(list(desc.sphere_center[s])) + T[desc.sphere_link[s]][:3, 3]
           for s in range(desc.n_spheres)]
    out = []
    for s in range(desc.n_spheres):
        link, r = desc.sphere_link[s], desc.sphere_radius[s]
        for p in range(desc.n_prims):
            d, n, pt = oracle_mod.sphere_prim(ctr[s], r, scene[p])
            g = -(n @ link_jacobian(ch, T, link, pt))
            out.append(((link, p, s, -1), (link, p), d, g, False))
    for s, sb in self_pairs(desc):
        la, lb = desc.sphere_link[s], desc.sphere_link[sb]
        v = ctr[sb] - ctr[s]
        L = float(np.sqrt(v @ v))
        n = v / L
        d = L - desc.sphere_radius[s] - desc.sphere_radius[sb]
        pa, pb = ctr[s] + desc.sphere_radius[s] * n, ctr[sb] - desc.sphere_radius[sb] * n
        g = -(n @ link_jacobian(ch, T, la, pa)) + n @ link_jacobian(ch, T, lb, pb)
        out.append(((la, -1 - lb, s, sb), (la, -1 - lb), d, g, True))
    return out


def expected_sets(cands, margin, coeff, buffer, overrides, R, D):
    """The selection and ordering rule: filter, error descending with ties by key,
    the first R rows; padded rows (-buffer, zero row, coefficient 1, key -1)."""
    sets = []
    for key, pair, d, g, both in cands:
        m, cf = overrides.get(pair, (margin, coeff))
        if pair in overrides and abs(cf) <= 1e-6:
            continue  # a pair set to a zero coefficient is dropped
        if not d <= m + buffer:
            continue
        err = m - d
        grad = (g / 2 if both else g) if err + buffer > 0 else np.zeros(D)
        sets.append((-err, key, err, cf, -grad))
    sets.sort(key=lambda e: (e[0], e[1]))
    values, jac, coeffs = np.full(R, -buffer), np.zeros((R, D)), np.ones(R)
    keys = np.full((R, 4), -1, dtype=np.int32)
    for i, (_, key, err, cf, row) in enumerate(sets[:R]):
        values[i], jac[i], coeffs[i], keys[i] = err, row, cf, key
    return values, jac, coeffs, len(sets), keys, [e[2] for e in sets]


def run_sets(desc, scene, x, cfg):
    """Two runs of a fresh object (they must agree bitwise): values, jac, coeffs, counts, keys."""
    cs = CollisionSets(desc, len(x), scene, cfg)
    try:
        out = cs.run(x)
        again = cs.run(x)
        for a, b in zip(out, again):
            assert a.tobytes() == b.tobytes(), "two runs differ"
    finally:
        cs.close()
    return out


def check_node(got, exp, scale, tie_ok=False):
    """One node's rows against the restatement.  tie_ok: rows whose errors agree
    within 1e-12 may have swapped places, at most one pair of rows."""
    values, jac, coeffs, count, keys = got
    ev, ej, ec, en, ek, _ = exp
    print(f"count {count} expected {en}\nvalues {values!r}\n expect {ev!r}\nkeys {keys.tolist()}\n expect {ek.tolist()}")
    assert count == en
    order = list(range(len(ev)))
    if tie_ok and not np.array_equal(keys, ek):
        swapped = [i for i in order if not np.array_equal(keys[i], ek[i])]
        assert len(swapped) == 2 and abs(ev[swapped[0]] - ev[swapped[1]]) <= TOL, swapped
        order[swapped[0]], order[swapped[1]] = swapped[1], swapped[0]
    assert np.array_equal(keys, ek[order])
    print(f"max |dv| {np.abs(values - ev[order]).max():.3e} max |dJ| {np.abs(jac - ej[order]).max():.3e}")
    assert np.abs(values - ev[order]).max() <= TOL * scale
    assert np.abs(jac - ej[order]).max() <= TOL * scale
    assert np.array_equal(coeffs, ec[order])


def no_near_ties(errs, R, but=()):
    """The restatement's errors have no two within 1e-9 among the rows that decide
    the first R (rounding cannot reorder them), apart from the pairs in `but`."""
    e = np.array(errs[:R + 1])
    for i in range(len(e) - 1):
        if (i, i + 1) not in but:
            assert e[i] - e[i + 1] > 1e-9, (i, e[i], e[i + 1])


# ------------------------------------------------------------------ spherebot
def spherebot_desc(n_steps=1, n_prims=1):
    """spherebot (trajopt_common/data/spherebot.urdf): two prismatic joints (x, then
    y) and a 0.5 m sphere on the last link."""
    d = abi.ProblemDesc()
    d.n_steps = n_steps
    d.chain = robots._chain((0.0, 0.0, 0.0), [
        ("spherebot_x_joint", abi.JOINT_PRISMATIC, (0.0, 0.0, 0.0), (1, 0, 0), (-20.0, 20.0)),
        ("spherebot_y_joint", abi.JOINT_PRISMATIC, (0.0, 0.0, 0.0), (0, 1, 0), (-20.0, 20.0)),
        ("spherebot_link_joint", abi.JOINT_FIXED, (0.0, 0.0, 0.0), None, None)])
    d.n_spheres = 1
    d.sphere_link[0] = 3
    d.sphere_radius[0] = 0.5
    d.n_prims = n_prims
    return d


def sphere_rec(center, radius):
    rec = np.zeros(16)
    rec[0] = abi.PRIM_SPHERE
    rec[1:4] = center
    rec[4] = radius
    return rec


# collision_unit.cpp:101-158 transcribed to spheres (the robot's 0.5 m sphere
# against a 0.5 m sphere at the origin; TrajOptCollisionConfig(0.1, 1), buffer
# 0.01): pose, value, row
SPHEREBOT_POSES = [
    ((-1.9, 0.0), -0.01, (0.0, 0.0)),   # outside the buffer
    ((-1.0, 0.0), 0.1, (1.0, 0.0)),     # touching: within the margin
    ((0.0, 1.0), 0.1, (0.0, -1.0)),
    ((-0.9, 0.0), 0.2, (1.0, 0.0)),     # in collision
]


@pytest.mark.parametrize("R", [1, 3])
def test_spherebot_fewer_sets_than_rows(R):
    d = spherebot_desc()
    scene = np.stack([sphere_rec((0.0, 0.0, 0.0), 0.5)[None]] * len(SPHEREBOT_POSES))
    x = np.array([p for p, _, _ in SPHEREBOT_POSES]).reshape(len(SPHEREBOT_POSES), 1, 2)
    values, jac, coeffs, counts, keys = run_sets(d, scene, x, abi.CsetsConfig(0.1, 1.0, 0.01, R, 0, 0))
    for b, (_, value, row) in enumerate(SPHEREBOT_POSES):
        n = 0 if value < 0 else 1
        print(b, values[b, 0], jac[b, 0], counts[b, 0], keys[b, 0].tolist())
        assert counts[b, 0] == n
        assert abs(values[b, 0, 0] - value) <= 1e-6
        assert np.abs(jac[b, 0, 0] - np.array(row)).max() <= 1e-6
        assert list(keys[b, 0, 0]) == ([3, 0, 0, -1] if n else [-1] * 4)
        # padded rows: -buffer, a zero row, coefficient 1
        assert np.all(values[b, 0, n:] == -0.01) and np.all(jac[b, 0, n:] == 0.0)
        assert np.all(coeffs[b, 0] == 1.0) and np.all(keys[b, 0, n:] == -1)


# ------------------------------------------------------------------ PR2, config C
MARGIN, COEFF, BUFFER = 0.05, 20.0, 0.15


def distinct_radii(d):
    """The arm model puts two equal spheres on one point (the second sphere of a
    link and the first of the next, where the joint origins coincide): their
    contacts would tie to rounding.  Every sphere gets its own radius here, so
    that only the tie test has a tie."""
    for s in range(d.n_spheres):
        d.sphere_radius[s] += 1e-3 * (s + 1)
    return d


@functools.lru_cache(maxsize=None)
def config_c(n_extra=0):
    """Config C (right_arm, 14 spheres, the 10-primitive scene), 3 nodes, one
    problem; n_extra more primitives: copies of the scene's first ones shifted by
    multiples of (0.011, -0.007, 0.005)."""
    wl = problems.make_workload("C", 1, n_steps=3)
    d = distinct_radii(abi.ProblemDesc.from_buffer_copy(wl.desc))
    scene = wl.scene[0]
    if n_extra:
        more = scene[:n_extra].copy()
        for k in range(n_extra):
            if more[k, 0] == abi.PRIM_CAPSULE:
                more[k, 4:7] += (k + 1) * np.array([0.011, -0.007, 0.005])
            more[k, 1:4] += (k + 1) * np.array([0.011, -0.007, 0.005])
        scene = np.concatenate([scene, more])
        d.n_prims = len(scene)
    scene.setflags(write=False)
    return d, scene, wl.init.copy()


def check_all_nodes(oracle_mod, d, scene, x, cfg, overrides=None, tie_nodes=()):
    R, D = cfg.max_num_cnt, d.chain.n_dof
    got = run_sets(d, scene[None], x, cfg)
    exps = []
    for u in range(cfg.last_step - cfg.first_step + 1):
        cands = candidates(oracle_mod, d, scene, x[0, cfg.first_step + u])
        exp = expected_sets(cands, cfg.margin, cfg.coeff, cfg.margin_buffer, overrides or {}, R, D)
        if u not in tie_nodes:
            no_near_ties(exp[5], R)
        check_node(tuple(a[0, u] for a in got), exp, max(abs(cfg.coeff), 1.0), tie_ok=u in tie_nodes)
        exps.append(exp)
    return got, exps


@pytest.mark.parametrize("n_extra", [0, 7], ids=["10prims", "17prims"])
def test_truncation(oracle_mod, n_extra):
    """More sets than rows, R = 3.  The candidates are 14 spheres x primitives plus
    8 self sphere pairs: 148 with 10 primitives, 246 with 17 (no multiple of 64,
    still one pass of the 256-thread block), so the 17-primitive case also runs
    19 primitives (274: a second pass, the running top R carried across)."""
    d, scene, x = config_c(n_extra)
    cfg = abi.CsetsConfig(MARGIN, COEFF, BUFFER, 3, 0, 2)
    got, exps = check_all_nodes(oracle_mod, d, scene, x, cfg)
    total = d.n_spheres * d.n_prims + len(self_pairs(d))
    print("candidates per node", total)
    assert total % 64 != 0
    assert all(e[3] > 3 for e in exps), [e[3] for e in exps]
    if n_extra:
        d2, scene2, _ = config_c(9)
        assert d2.n_spheres * d2.n_prims + len(self_pairs(d2)) > 256
        check_all_nodes(oracle_mod, d2, scene2, x, cfg)


def test_restatement_against_oracle_rows(oracle_mod):
    """The numpy candidates against oracle.collision_rows on a DISCRETE descriptor:
    distance within 1e-12, value = margin - d, row = -a_t (a_t drops
    coefficients below 1e-7, hence the 2e-7 bar on rows)."""
    d, scene, x = config_c(0)
    dd = abi.ProblemDesc.from_buffer_copy(d)
    dd.coll_enabled, dd.coll_continuous, dd.coll_margin, dd.coll_buffer = 1, 2, 1e3, 0.0
    dd.coll_first_step, dd.coll_last_step, dd.coll_n_fixed, dd.n_coll_pairs, dd.n_coll_extra = 0, 2, 0, 0, 0
    dd.coll_contact_test = abi.CONTACT_ALL
    wl = problems.Workload("rows", dd, x, np.zeros((1, dd.n_cart, 12)), scene[None], x)
    rows = oracle_mod.collision_rows(wl, 0, x[0], cap=4096)
    D = d.chain.n_dof
    for t in range(3):
        # the oracle's rows name a self contact's other side by its sphere: other = -1 - sphere_b
        cands = {(c[0][0], c[0][1] if c[0][3] < 0 else -1 - c[0][3], c[0][2]): c
                 for c in candidates(oracle_mod, d, scene, x[0, t])}
        rt = rows[rows[:, 0] == t]
        assert len(rt) == len(cands)
        for r in rt:
            c = cands[(int(r[1]), int(r[2]), int(r[3]))]
            assert abs(c[2] - r[5]) <= TOL
            assert np.abs(c[3] - r[8:8 + D]).max() <= 2e-7


def test_zero_coefficient_and_pair_margin(oracle_mod):
    """Per-pair overrides: a zero-coefficient pair's contact never appears, and a
    pair with its own margin and coefficient carries them."""
    d0, scene, x = config_c(0)
    base = abi.CsetsConfig(MARGIN, COEFF, BUFFER, 3, 0, 2)
    _, exps = check_all_nodes(oracle_mod, d0, scene, x, base)
    # the pair of node 0's first row loses its coefficient; the pair of its second row gets its own data
    (l0, p0, _, _), (l1, p1, _, _) = (tuple(int(v) for v in exps[0][4][i]) for i in (0, 1))
    assert (l0, p0) != (l1, p1) and p0 >= 0 and p1 >= 0
    d = abi.ProblemDesc.from_buffer_copy(d0)
    d.n_coll_pairs = 0
    problems.add_coll_pair(d, l0, p0, 0.3, 0.0)
    problems.add_coll_pair(d, l1, p1, 0.08, 7.0)
    problems.add_coll_pair(d, l1, p1, 0.5, 3.0, term=1)  # another term's entry: not read
    ov = problems.pair_overrides(d)
    got, exps2 = check_all_nodes(oracle_mod, d, scene, x, base, overrides=ov)
    keys = got[4][0]
    assert not any((int(k[0]), int(k[1])) == (l0, p0) for k in keys.reshape(-1, 4))
    hit = [(u, i) for u in range(3) for i in range(3) if (int(keys[u, i, 0]), int(keys[u, i, 1])) == (l1, p1)]
    assert hit and all(got[2][0, u, i] == 7.0 for u, i in hit)


def test_zero_gradient_pair():
    """error_with_buffer <= 0 gives a zero row (weight zero) while another pair is
    kept: spherebot against two spheres, the first pair's margin override puts it
    exactly on its contact distance (0.5 = 0.25 + 0.25, exact in binary)."""
    d = spherebot_desc(n_prims=2)
    problems.add_coll_pair(d, 3, 0, 0.25, 2.0)
    scene = np.stack([sphere_rec((0.0, 0.0, 0.0), 0.5), sphere_rec((3.0, 1.1, 0.0), 0.5)])[None]
    x = np.array([[[1.5, 0.0]]])  # d = 0.5 from the first, ~0.86 from the second
    values, jac, coeffs, counts, keys = run_sets(d, scene, x, abi.CsetsConfig(1.0, 1.0, 0.25, 2, 0, 0))
    print(values, jac, coeffs, counts, keys)
    assert counts[0, 0] == 2
    assert keys[0, 0].tolist() == [[3, 1, 0, -1], [3, 0, 0, -1]]
    assert values[0, 0, 1] == -0.25 and np.all(jac[0, 0, 1] == 0.0) and coeffs[0, 0, 1] == 2.0
    assert values[0, 0, 0] > 0 and np.abs(jac[0, 0, 0]).max() > 0.1 and coeffs[0, 0, 0] == 1.0


def test_exact_tie_follows_the_key():
    """Two mirror-image primitives give two sets the same error, bitwise: the order
    follows the key (primitive 0 before primitive 1, whichever comes first in
    memory)."""
    d = spherebot_desc(n_prims=3)
    for order in ([0, 1, 2], [1, 0, 2]):
        prims = [sphere_rec((0.0, 0.75, 0.0), 0.5), sphere_rec((0.0, -0.75, 0.0), 0.5),
                 sphere_rec((-3.0, 0.0, 0.0), 0.5)]
        scene = np.stack([prims[i] for i in order])[None]
        x = np.array([[[0.5, 0.0]]])
        # the restatement's tie is bitwise: sqrt(0.25 + 0.5625) both times
        c = np.array([0.5, 0.0, 0.0])
        dist = [float(np.sqrt(((p[1:4] - c) ** 2).sum())) - 1.0 for p in scene[0]]
        assert dist[0] == dist[1]
        values, jac, coeffs, counts, keys = run_sets(d, scene, x, abi.CsetsConfig(0.2, 1.0, 0.05, 2, 0, 0))
        print(values, jac, keys)
        assert counts[0, 0] == 2
        assert keys[0, 0].tolist() == [[3, 0, 0, -1], [3, 1, 0, -1]]
        assert values[0, 0, 0] == values[0, 0, 1] == 0.2 - dist[0]
        sy = 1.0 if order[0] == 0 else -1.0  # primitive 0 lies at +y or -y
        assert jac[0, 0, 0, 1] == -jac[0, 0, 1, 1] and jac[0, 0, 0, 1] * sy > 0
        assert jac[0, 0, 0, 0] == jac[0, 0, 1, 0]


def test_exact_tie_follows_the_key_not_the_candidate_order():
    """Two robot spheres mirrored in y against two primitives mirrored in y: sphere 0
    against primitive 1 ties bitwise with sphere 1 against primitive 0.  The
    candidates are scanned sphere-major, so (sphere 0, primitive 1) comes first in
    the pool, while the key order (link, other, sphere) puts primitive 0's contact
    first: a tie break by pool position would give the other order.  The other two
    pairs are 0.6 m apart, outside margin + buffer."""
    d = spherebot_desc(n_prims=2)
    d.n_spheres = 2
    for s, y in enumerate((0.5, -0.5)):
        d.sphere_link[s], d.sphere_radius[s] = 3, 0.5
        d.sphere_center[s][0], d.sphere_center[s][1], d.sphere_center[s][2] = 0.0, y, 0.0
    scene = np.stack([sphere_rec((1.5, -0.75, 0.0), 0.5), sphere_rec((1.5, 0.75, 0.0), 0.5)])[None]
    x = np.array([[[0.5, 0.0]]])
    ctr = [np.array([0.5, 0.5, 0.0]), np.array([0.5, -0.5, 0.0])]
    dist = {(s, p): float(np.sqrt(((scene[0, p, 1:4] - ctr[s]) ** 2).sum())) - 1.0 for s in (0, 1) for p in (0, 1)}
    assert dist[0, 1] == dist[1, 0] and dist[0, 1] < 0.2 and min(dist[0, 0], dist[1, 1]) > 0.25  # a bitwise tie
    values, jac, coeffs, counts, keys = run_sets(d, scene, x, abi.CsetsConfig(0.2, 1.0, 0.05, 2, 0, 0))
    print(values, jac, keys)
    assert counts[0, 0] == 2
    assert keys[0, 0].tolist() == [[3, 0, 1, -1], [3, 1, 0, -1]]
    assert values[0, 0, 0] == values[0, 0, 1] and abs(values[0, 0, 0] - (0.2 - dist[0, 1])) <= TOL
    # sphere 1 (at -y) is pushed up by primitive 0 below it: the distance grows with y, the row is -gradient
    assert jac[0, 0, 0, 1] == -jac[0, 0, 1, 1] and jac[0, 0, 0, 1] < 0
    assert jac[0, 0, 0, 0] == jac[0, 0, 1, 0] and jac[0, 0, 0, 0] > 0


@functools.lru_cache(maxsize=None)
def config_e():
    wl = problems.make_workload("E", 1, n_steps=3)
    scene = wl.scene[0]
    scene.setflags(write=False)
    return distinct_radii(abi.ProblemDesc.from_buffer_copy(wl.desc)), scene, wl.init.copy()


def test_self_pair_half_sum(oracle_mod):
    """both_arms with the inter-arm pairs enabled, at a pose where spheres of the
    two arms are within the margin: the row is minus half the sum of the two
    links' gradients."""
    d, scene, x = config_e()
    x = x.copy()
    x[0, 1] = 0.0
    x[0, 1, 0], x[0, 1, 7], x[0, 1, 3] = -0.55, 0.5, -0.3  # the shoulder pans turn the arms toward each other
    cfg = abi.CsetsConfig(0.05, 10.0, 0.05, 4, 1, 1)
    got, exps = check_all_nodes(oracle_mod, d, scene, x, cfg)
    keys = got[4][0, 0]
    selfrows = [i for i in range(4) if keys[i, 3] >= 0]
    assert selfrows, keys.tolist()
    i = selfrows[0]
    assert keys[i, 1] == -1 - d.sphere_link[keys[i, 3]] and d.sphere_link[keys[i, 2]] == keys[i, 0]
    # both arms' joints carry the row
    assert np.abs(got[1][0, 0, i, :7]).max() > 1e-3 and np.abs(got[1][0, 0, i, 7:]).max() > 1e-3


def test_batch_independence():
    """Batch 5 of identical problems: identical slices, equal to the batch-1 result, bitwise."""
    d, scene, x = config_c(7)
    cfg = abi.CsetsConfig(MARGIN, COEFF, BUFFER, 3, 0, 2)
    one = run_sets(d, scene[None], x, cfg)
    five = run_sets(d, np.repeat(scene[None], 5, axis=0), np.repeat(x, 5, axis=0), cfg)
    for a, b in zip(one, five):
        for k in range(5):
            assert b[k].tobytes() == a[0].tobytes()


def test_refusals_on_the_device_path():
    d, scene, x = config_c(0)
    cs = CollisionSets(d, 1, scene[None], abi.CsetsConfig(MARGIN, COEFF, BUFFER, 3, 0, 2))
    try:
        with pytest.raises(HipError, match="x has"):
            cs.run(x[:, :2])
    finally:
        cs.close()


# ------------------------------------------------------------------ CartPos sets
def _pose12(xyz, rpy):
    cr, sr, cp, sp, cy, sy = (f(a) for a in rpy for f in (np.cos, np.sin))
    R = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                  [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                  [-sp, cp * sr, cp * cr]])
    return np.concatenate([R, np.array(xyz)[:, None]], axis=1).reshape(12)


ROBOT_FRAMES = {  # robot: (chain root link, tool frame, an arm link, its chain index, the tool's chain index)
    "right_arm": ("torso_lift_link", "r_gripper_tool_frame", "r_forearm_roll_link", 6, 11),
    "torso_right_arm": ("base_link", "r_gripper_tool_frame", "r_forearm_roll_link", 7, 12),
}
TOOL_OFFSET = _pose12((0.02, -0.01, 0.03), (0.1, -0.2, 0.3))
GOAL = _pose12((0.55, -0.3, 0.25), (0.4, 0.9, -0.6))
ARM_OFFSET = _pose12((0.05, 0.0, -0.02), (-0.3, 0.2, 0.1))
ANCHOR = _pose12((0.35, -0.45, 0.1), (0.2, -0.1, 0.7))


def cart_case(robot, nodes):
    """A source-active and a target-active CartPos set on each node of `nodes`
    (static frames at the chain root, so the evaluator's static pose is the offset
    itself), with the equivalent CartPose workload: the active frame is the
    term's source link, the static pose its target."""
    root, tool, arm, arm_idx, tool_idx = ROBOT_FRAMES[robot]
    n_nodes = max(nodes) + 1
    cart, links = [], []
    for n in nodes:
        cart.append(dict(node=n, source_frame=tool, target_frame=root, source_offset=TOOL_OFFSET, target_offset=GOAL))
        links.append((n, tool_idx, TOOL_OFFSET, GOAL))
        cart.append(dict(node=n, source_frame=root, target_frame=arm, source_offset=ANCHOR, target_offset=ARM_OFFSET))
        links.append((n, arm_idx, ARM_OFFSET, ANCHOR))
    d = problems.base_desc(n_nodes, robot)
    d.n_cart = len(links)
    for k, (n, link, off, _) in enumerate(links):
        problems._add_cart(d, k, n, True, link)
        for i in range(12):
            d.cart_source_offset[k][i] = off[i]
    D = d.chain.n_dof
    lo, hi, _ = robots.chain_limits(d.chain)
    rng = np.random.default_rng(5)
    x = np.clip(rng.normal(0, 0.6, (1, n_nodes, D)), np.maximum(lo, -2.0), np.minimum(hi, 2.0))
    targets = np.stack([t for _, _, _, t in links])[None]
    wl = problems.Workload("cartpos", d, x, targets, np.zeros((1, 0, 16)), x)
    return tsqp.make_spec(x[0], []), tsqp.make_kin_spec(robot, cart=cart), wl, x


@pytest.mark.parametrize("nodes", [(0,), (0, 2)], ids=["1node", "3nodes_sets_on_0_and_2"])
@pytest.mark.parametrize("robot", ["right_arm", "torso_right_arm"])
def test_cartpos_against_the_oracle_and_the_cartpose_evaluator(oracle_mod, robot, nodes):
    spec, kin, wl, x = cart_case(robot, nodes)
    D = wl.n_dof
    r = tsqp.eval_kin(spec, kin, x)
    assert list(r["set_rows"]) == [6] * (2 * len(nodes)) and r["launches"] == (1, 0)
    eo, jo = oracle_mod.linearize(wl, x)
    te = TermEvaluator(wl)
    try:
        for k in range(wl.desc.n_cart):
            n = wl.desc.cart_step[k]
            vals, jac = r["values"][0, 6 * k:6 * k + 6], r["jac"][0, 6 * k:6 * k + 6]
            print(robot, k, "max |dv|", np.abs(vals - eo[0, k]).max(), "max |dJ|", np.abs(jac[:, n * D:(n + 1) * D] - jo[0, k]).max())
            # tests/test_gpu.py test_cartpose_linearization_parity's tolerances
            np.testing.assert_allclose(vals, eo[0, k], rtol=0, atol=1e-12)
            np.testing.assert_allclose(jac[:, n * D:(n + 1) * D], jo[0, k], rtol=0, atol=1e-9)
            other = np.delete(jac, np.s_[n * D:(n + 1) * D], axis=1)
            assert not other.any()  # only the node's own columns
            # the shared device function: bitwise thip_eval_cart_pose's values for the same term
            e1, j1 = te.cart_pose(k, x[:, n])
            assert vals.tobytes() == e1[0].tobytes() and jac[:, n * D:(n + 1) * D].tobytes() == j1[0].tobytes()
    finally:
        te.close()
    assert np.abs(eo).max() > 0.05 and not r["lower"].any() and not r["upper"].any() and np.all(r["coeffs"] == 1.0)


def test_cartpos_world_static_frame(oracle_mod):
    """A static frame outside the chain (base_footprint): its world pose goes into
    the chain root on the host, so the values agree with numpy FK to rounding."""
    spec, _, wl, x = cart_case("right_arm", (0,))
    kin = tsqp.make_kin_spec("right_arm", cart=[dict(node=0, source_frame="r_gripper_tool_frame",
                                                     target_frame="base_footprint", target_offset=GOAL)])
    r = tsqp.eval_kin(spec, kin, x)
    T = robots.fwd_kin(wl.desc.chain, x[0, 0])[11]
    E = np.linalg.inv(robots._to44(GOAL)) @ T
    np.testing.assert_allclose(r["values"][0, :3], E[:3, 3], rtol=0, atol=1e-12)


# ------------------------------------------------------------------ prefetch
def test_one_launch_per_x_and_a_query_at_another_x(oracle_mod):
    """3 CartPos sets and one collision evaluator over 3 nodes: one CartPos launch
    and one collision launch per x; every set returns each x's own values; a set
    asked at joint values that were not prefetched relaunches for itself and the
    kept results stay right."""
    d, scene, x0 = config_c(0)
    root, tool, arm, _, _ = ROBOT_FRAMES["right_arm"]
    cart = [dict(node=n, source_frame=tool, target_frame=root, target_offset=GOAL) for n in range(3)]
    coll = [dict(first=0, last=2, margin=MARGIN, coeff=COEFF, buffer=BUFFER, max_num_cnt=3)]
    kin = tsqp.make_kin_spec("right_arm", cart=cart, coll=coll, prims=scene)
    spec = tsqp.make_spec(x0[0], [])
    one = tsqp.eval_kin(spec, kin, x0)
    assert one["launches"] == (1, 1) and list(one["set_rows"]) == [6, 6, 6, 3, 3, 3]
    x1 = x0 + 0.05 * np.random.default_rng(3).standard_normal(x0.shape)
    probe = x1[0, 1]
    two = tsqp.eval_kin(spec, kin, np.concatenate([x0, x1, x0]), probe_q=probe)
    assert two["launches"] == (3 + 3, 3)  # three x, then three single-set probes
    alone = tsqp.eval_kin(spec, kin, x1)
    for key in ("values", "jac", "coeffs"):
        assert two[key][0].tobytes() == one[key][0].tobytes() == two[key][2].tobytes()
        assert two[key][1].tobytes() == alone[key][0].tobytes()
    assert np.abs(two["values"][1] - two["values"][0]).max() > 1e-3
    # the probe: every CartPos set at node 1's joint values of x1 -- set 1's own values there
    for k in range(3):
        assert two["probe"][6 * k:6 * k + 6].tobytes() == alone["values"][0, 6:12].tobytes()
    assert np.isnan(two["probe"][18:]).all()


def test_kin_collision_set_without_fixed_sparsity():
    """fixed_sparsity = false: getJacobian stops after the rows in use.  Spherebot
    against its environment's three spheres at poses with 0, 1 and 3 sets, R = 3:
    the dense rows equal the fixed-sparsity ones, rows past the sets are zero with
    value -buffer, and a row past them keeps its last coefficient (1 until a set
    has used it)."""
    xs = np.array([[[5.0, 5.0]], [[1.1, 0.0]], [[-0.75, 0.75]]])
    spec = tsqp.make_spec(xs[0], [])
    out = {}
    for fixed in (False, True):
        coll = [dict(first=0, margin=0.2, coeff=4.0, buffer=0.05, max_num_cnt=3, fixed_sparsity=fixed)]
        out[fixed] = tsqp.eval_kin(spec, tsqp.make_kin_spec("manipulator", coll=coll), xs)
    r = out[False]
    print(r["values"], r["jac"], r["coeffs"])
    for key in ("values", "jac", "coeffs"):
        assert r[key].tobytes() == out[True][key].tobytes()
    assert list(r["set_rows"]) == [3]
    for ix, n in enumerate((0, 1, 3)):
        assert np.all(r["values"][ix, n:3] == -0.05) and not r["jac"][ix, n:3].any()
        assert np.all(r["values"][ix, :n] > -0.05) and np.all(np.abs(r["jac"][ix, :n]).max(axis=1) > 0.1)
    assert abs(r["values"][1, 0] - 0.1) <= 1e-12 and np.abs(r["jac"][1, 0] - [-1.0, 0.0]).max() <= 1e-12
    assert r["coeffs"][:, :3].tolist() == [[1.0, 1.0, 1.0], [4.0, 1.0, 1.0], [4.0, 4.0, 4.0]]


def test_kin_collision_sets_match_the_device_rows(oracle_mod):
    """DiscreteCollisionConstraint through the host classes: the rows of
    thip_csets_run for the environment's model (the built-in arm spheres), the
    jacobian in the node's columns, all R x n_dof entries with fixed_sparsity."""
    d0, scene, x0 = config_c(0)
    d = abi.ProblemDesc.from_buffer_copy(problems.make_workload("C", 1, n_steps=3).desc)  # the built-in radii
    coll = [dict(first=1, last=2, margin=MARGIN, coeff=COEFF, buffer=BUFFER, max_num_cnt=3, penalty=tsqp.HINGE)]
    r = tsqp.eval_kin(tsqp.make_spec(x0[0], []), tsqp.make_kin_spec("right_arm", coll=coll, prims=scene), x0)
    values, jac, coeffs, counts, _ = run_sets(d, scene[None], x0, abi.CsetsConfig(MARGIN, COEFF, BUFFER, 3, 1, 2))
    D = 7
    for u, n in enumerate((1, 2)):
        assert r["values"][0, 3 * u:3 * u + 3].tobytes() == values[0, u].tobytes()
        assert r["jac"][0, 3 * u:3 * u + 3, n * D:(n + 1) * D].tobytes() == jac[0, u].tobytes()
        assert r["coeffs"][0, 3 * u:3 * u + 3].tobytes() == coeffs[0, u].tobytes()
        assert counts[0, u] > 3
    assert np.all(np.isneginf(r["lower"])) and not r["upper"].any()
