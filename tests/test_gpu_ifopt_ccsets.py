"""trajopt_ifopt's fixed-size continuous collision sets (thip_ccsets_*,
coll_sets_cont.hip) on the GPU, and ContinuousCollisionConstraint through
thost_tsqp_eval_kin.

The device rows are checked against the numpy restatement of tests/ccsets_model.py,
whose contact list tests/test_ifopt_ccsets_frontdoor.py ties to
oracle.collision_rows.  Values and rows agree within 1e-12 x max(|coeff|, 1)
(tests/test_gpu_terms.py's tolerance for collision slots); keys, counts and
coefficients are exact.  Every comparison first asserts on the restatement that
no two rank-deciding selection values are within 1e-9, the spheres have distinct
radii, and two runs of a fresh object agree bitwise.
"""
import functools
import math

import numpy as np
import pytest

import ccsets_model as cm
from trajopt_amd import abi, problems, robots, tsqp
from trajopt_amd.runtime import ContinuousCollisionSets, HipError

pytestmark = pytest.mark.gpu

TOL = 1e-12
MARGIN, COEFF, BUFFER = 0.05, 20.0, 0.15
ETYPES = [cm.LVS_DISCRETE, cm.CONTINUOUS, cm.LVS_CONTINUOUS]
ETYPE_IDS = ["lvs_discrete", "continuous", "lvs_continuous"]


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


# ------------------------------------------------------------------ helpers
def run_sets(desc, scene, x, cfg, seg_fixed=None):
    """Two runs of a fresh object (they must agree bitwise): values, jac, coeffs, counts, keys."""
    cs = ContinuousCollisionSets(desc, len(x), scene, cfg, seg_fixed)
    try:
        out = cs.run(x)
        again = cs.run(x)
        for a, b in zip(out, again):
            assert a.tobytes() == b.tobytes(), "two runs differ"
    finally:
        cs.close()
    return out


def no_near_ties(Es, R):
    """No two of the selection values that decide the first R rows are within 1e-9."""
    e = [v for v in Es[:R + 1]]
    for i in range(len(e) - 1):
        if math.isinf(e[i]) and math.isinf(e[i + 1]):
            continue
        assert e[i] - e[i + 1] > 1e-9, (i, e[i], e[i + 1])


def check_segment(got, exp, scale):
    values, jac, coeffs, count, keys = got
    ev, ej, ec, en, ek = exp[:5]
    print(f"count {count} expected {en}\nvalues {values!r}\n expect {ev!r}\nkeys {keys.tolist()}\n expect {ek.tolist()}")
    print(f"max |dv| {np.abs(values - ev).max():.3e} max |dJ| {np.abs(jac - ej).max():.3e} max |J| {np.abs(ej).max():.3e}")
    assert count == en
    assert np.array_equal(keys, ek)
    assert np.abs(values - ev).max() <= TOL * scale
    assert np.abs(jac - ej).max() <= TOL * scale
    assert np.array_equal(coeffs, ec)


def check_problem(oracle_mod, d, scene, x, cfg, seg_fixed=None, overrides=None):
    """One problem's device rows against the restatement, segment by segment."""
    exps, cnts = cm.expected(oracle_mod, d, scene, x[0], cfg, seg_fixed, overrides)
    for exp in exps:
        no_near_ties(exp[5], cfg.max_num_cnt)
    got = run_sets(d, scene[None], x, cfg, seg_fixed)
    for u, exp in enumerate(exps):
        check_segment(tuple(a[0, u] for a in got), exp, max(abs(cfg.coeff), 1.0))
    return got, exps, cnts


def spherebot_desc(n_steps=2, n_prims=1):
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


def distinct_radii(d):
    """The arm model puts two equal spheres on one point: their contacts would tie
    to rounding.  Every sphere gets its own radius."""
    for s in range(d.n_spheres):
        d.sphere_radius[s] += 1e-3 * (s + 1)
    return d


@functools.lru_cache(maxsize=None)
def config_c(n_extra=0):
    """Config C (right_arm, 14 spheres, the 10-primitive scene), 3 nodes, one problem;
    n_extra more primitives: copies of the scene's first ones shifted by multiples of
    (0.011, -0.007, 0.005).  Also an lvs length that gives every segment 3 to 8 sub-states."""
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
    x = wl.init.copy()
    lvs = max(float(np.linalg.norm(x[0, t + 1] - x[0, t])) for t in range(2)) / 6.5
    return d, scene, x, lvs


def ccfg(R, etype, lvs, first=0, last=2, margin=MARGIN, coeff=COEFF, buffer=BUFFER):
    return abi.CcsetsConfig(margin, coeff, buffer, R, first, last, etype, lvs)


def substates_in_range(cnts, etype):
    for cnt in cnts:
        n_sub = cnt if etype == cm.LVS_DISCRETE else cnt - 1
        assert n_sub == 1 if etype == cm.CONTINUOUS else 3 <= n_sub <= 8, cnts


# ------------------------------------------------------------------ spherebot hand values
SPHEREBOT_CASES = [
    # x0, x1, seg_fixed, count, value, end-0 row, end-1 row
    ((-1.0, 0.9), (1.0, 0.9), 0, 1, 0.2, (0.0, -0.5), (0.0, -0.5)),
    ((-1.0, 0.9), (1.0, 0.9), 1, 1, 0.2, (0.0, 0.0), (0.0, -0.5)),
    ((-1.0, 0.9), (1.0, 0.9), 2, 1, 0.2, (0.0, -0.5), (0.0, 0.0)),
    ((0.0, 0.9), (2.0, 0.9), 0, 1, 0.2, (0.0, -1.0), (0.0, 0.0)),   # closest at the start: Time0
    ((0.0, 0.9), (2.0, 0.9), 1, 0, -0.01, (0.0, 0.0), (0.0, 0.0)),  # vars0 fixed: the contact is removed
    ((-1.0, 3.0), (1.0, 3.0), 0, 0, -0.01, (0.0, 0.0), (0.0, 0.0)),  # outside the buffer
]


@pytest.mark.parametrize("R", [1, 3])
def test_spherebot_hand_values(R):
    """One 0.5 m robot sphere against a 0.5 m sphere at the origin, margin 0.1, coeff 1,
    buffer 0.01, CONTINUOUS (one cast)."""
    d = spherebot_desc()
    scene = sphere_rec((0.0, 0.0, 0.0), 0.5)[None, None]
    for x0, x1, fx, n, value, row0, row1 in SPHEREBOT_CASES:
        x = np.array([[x0, x1]])
        values, jac, coeffs, counts, keys = run_sets(d, scene, x, ccfg(R, cm.CONTINUOUS, 1.0, 0, 1, 0.1, 1.0, 0.01), [fx])
        print(x0, x1, fx, values[0, 0], jac[0, 0].tolist(), counts[0, 0], keys[0, 0].tolist())
        assert counts[0, 0] == n
        assert abs(values[0, 0, 0] - value) <= 1e-9
        assert np.abs(jac[0, 0, 0, 0] - np.array(row0)).max() <= 1e-9
        assert np.abs(jac[0, 0, 0, 1] - np.array(row1)).max() <= 1e-9
        assert list(keys[0, 0, 0]) == ([3, 0, 0, -1] if n else [-1] * 4)
        # padded rows: -buffer, a zero row, coefficient 1, key -1
        assert np.all(values[0, 0, n:] == -0.01) and np.all(jac[0, 0, n:] == 0.0)
        assert np.all(coeffs[0, 0] == 1.0) and np.all(keys[0, 0, n:] == -1)


# ------------------------------------------------------------------ config C against the restatement
@pytest.mark.parametrize("R", [3, 64])
@pytest.mark.parametrize("seg_fixed", [None, (1, 2)], ids=["free", "first_vars0_second_vars1_fixed"])
@pytest.mark.parametrize("etype", ETYPES, ids=ETYPE_IDS)
def test_config_c_against_the_restatement(oracle_mod, etype, seg_fixed, R):
    d, scene, x, lvs = config_c(0)
    got, exps, cnts = check_problem(oracle_mod, d, scene, x, ccfg(R, etype, lvs), seg_fixed)
    substates_in_range(cnts, etype)
    if R == 3:
        assert all(e[3] > R for e in exps), [e[3] for e in exps]  # more sets than rows
    else:
        assert all(0 < e[3] < R for e in exps), [e[3] for e in exps]
    # the weighted average is exercised: a selected set with contacts at two or more sub-states
    multi = [max(e[6][:R], default=0) for e in exps]
    print("contacts of the largest selected set per segment", multi)
    if etype != cm.CONTINUOUS:
        assert max(multi) >= 2
    assert max(np.abs(e[1]).max() for e in exps) > 1e-2


def test_more_than_256_keys(oracle_mod):
    """19 primitives: 14 x 19 + 8 = 274 keys, a second pass with the running top R carried over."""
    d, scene, x, lvs = config_c(9)
    total = d.n_spheres * d.n_prims + len(cm.self_pairs(d))
    assert total > 256 and total % 256 != 0
    _, exps, cnts = check_problem(oracle_mod, d, scene, x, ccfg(3, cm.LVS_CONTINUOUS, lvs))
    substates_in_range(cnts, cm.LVS_CONTINUOUS)
    assert all(e[3] > 3 for e in exps)


# ------------------------------------------------------------------ config E: self pairs
@functools.lru_cache(maxsize=None)
def config_e():
    """both_arms, 2 nodes around a pose where spheres of the two arms are within the
    margin (the shoulder pans turn the arms toward each other)."""
    wl = problems.make_workload("E", 1, n_steps=2)
    d = distinct_radii(abi.ProblemDesc.from_buffer_copy(wl.desc))
    scene = wl.scene[0]
    scene.setflags(write=False)
    x = np.zeros((1, 2, d.chain.n_dof))
    x[0, :, 0], x[0, :, 7], x[0, :, 3] = -0.55, 0.5, -0.3
    x[0, 0] -= 0.04 * np.cos(np.arange(d.chain.n_dof))
    x[0, 1] += 0.04 * np.sin(1.0 + np.arange(d.chain.n_dof))
    lvs = float(np.linalg.norm(x[0, 1] - x[0, 0])) / 5.5
    return d, scene, x, lvs


@pytest.mark.parametrize("etype", [cm.LVS_CONTINUOUS, cm.LVS_DISCRETE], ids=["lvs_continuous", "lvs_discrete"])
def test_config_e_self_pairs(oracle_mod, etype):
    """Self pairs with both links moved by joints; for LVS_CONTINUOUS the two sides'
    cc_type can differ."""
    d, scene, x, lvs = config_e()
    cfg = ccfg(4, etype, lvs, 0, 1, 0.05, 10.0, 0.05)
    got, exps, cnts = check_problem(oracle_mod, d, scene, x, cfg)
    substates_in_range(cnts, etype)
    keys = got[4][0, 0]
    selfrows = [i for i in range(4) if keys[i, 3] >= 0]
    assert selfrows, keys.tolist()
    i = selfrows[0]
    assert keys[i, 1] == -1 - d.sphere_link[keys[i, 3]] and d.sphere_link[keys[i, 2]] == keys[i, 0]
    # both arms' joints carry the row at both ends
    J = got[1][0, 0, i]
    assert np.abs(J[:, :7]).max() > 1e-3 and np.abs(J[:, 7:]).max() > 1e-3


# ------------------------------------------------------------------ per-pair overrides
def test_zero_coefficient_and_pair_margin(oracle_mod):
    """A zero-coefficient pair forms no set; a pair with its own margin and coefficient carries them."""
    d0, scene, x, lvs = config_c(0)
    base = ccfg(3, cm.LVS_CONTINUOUS, lvs)
    _, exps, _ = check_problem(oracle_mod, d0, scene, x, base)
    (l0, p0, _, _), (l1, p1, _, _) = (tuple(int(v) for v in exps[0][4][i]) for i in (0, 1))
    assert (l0, p0) != (l1, p1) and p0 >= 0 and p1 >= 0
    d = abi.ProblemDesc.from_buffer_copy(d0)
    d.n_coll_pairs = 0
    problems.add_coll_pair(d, l0, p0, 0.3, 0.0)
    problems.add_coll_pair(d, l1, p1, 0.08, 7.0)
    problems.add_coll_pair(d, l1, p1, 0.5, 3.0, term=1)  # another term's entry: not read
    got, _, _ = check_problem(oracle_mod, d, scene, x, base, overrides=problems.pair_overrides(d))
    keys = got[4][0]
    assert not any((int(k[0]), int(k[1])) == (l0, p0) for k in keys.reshape(-1, 4))
    hit = [(u, i) for u in range(2) for i in range(3) if (int(keys[u, i, 0]), int(keys[u, i, 1])) == (l1, p1)]
    assert hit and all(got[2][0, u, i] == 7.0 for u, i in hit)


# ------------------------------------------------------------------ exact tie
def test_exact_tie_follows_the_key_not_the_candidate_order():
    """Two robot spheres mirrored in y against two primitives mirrored in y, the segment
    along x between them: sphere 0 against primitive 1 ties bitwise with sphere 1 against
    primitive 0.  The keys are scanned sphere-major, so (sphere 0, primitive 1) comes
    first in the pool while the key order puts primitive 0's set first.  The other two
    pairs stay 0.25 m apart, outside margin + buffer."""
    d = spherebot_desc(n_prims=2)
    d.n_spheres = 2
    for s, y in enumerate((0.5, -0.5)):
        d.sphere_link[s], d.sphere_radius[s] = 3, 0.5
        d.sphere_center[s][0], d.sphere_center[s][1], d.sphere_center[s][2] = 0.0, y, 0.0
    scene = np.stack([sphere_rec((1.5, -0.75, 0.0), 0.5), sphere_rec((1.5, 0.75, 0.0), 0.5)])[None]
    x = np.array([[[0.5, 0.0], [2.5, 0.0]]])  # the closest points at t = 0.5, exactly
    values, jac, coeffs, counts, keys = run_sets(d, scene, x, ccfg(2, cm.CONTINUOUS, 1.0, 0, 1, 0.1, 1.0, 0.05))
    print(values, jac, keys)
    assert counts[0, 0] == 2
    assert keys[0, 0].tolist() == [[3, 0, 1, -1], [3, 1, 0, -1]]
    assert values[0, 0, 0] == values[0, 0, 1] and abs(values[0, 0, 0] - (0.1 + 0.75)) <= TOL
    for e in range(2):
        # sphere 1 (at -y) is pushed up by primitive 0 below it
        assert jac[0, 0, 0, e, 1] == -jac[0, 0, 1, e, 1] and abs(jac[0, 0, 0, e, 1] + 0.5) <= TOL
        assert jac[0, 0, 0, e, 0] == jac[0, 0, 1, e, 0] == 0.0


# ------------------------------------------------------------------ batch
def test_batch_independence():
    """A batch of 3 different problems and the same batch permuted: permuted rows, bitwise."""
    d, scene, x, lvs = config_c(7)
    rng = np.random.default_rng(11)
    xs = np.concatenate([x, x + 0.03 * rng.standard_normal(x.shape), x + 0.03 * rng.standard_normal(x.shape)])
    scenes = np.stack([scene, scene + 0.0, scene + 0.0])
    scenes[1, :, 1] += 0.01
    scenes[2, :, 2] -= 0.01
    cfg = ccfg(3, cm.LVS_CONTINUOUS, lvs)
    a = run_sets(d, scenes, xs, cfg, [1, 0])
    perm = [2, 0, 1]
    b = run_sets(d, scenes[perm], xs[perm], cfg, [1, 0])
    for u, v in zip(a, b):
        for k, src in enumerate(perm):
            assert v[k].tobytes() == u[src].tobytes()
    assert a[0][0].tobytes() != a[0][1].tobytes()
    one = run_sets(d, scenes[1:2], xs[1:2], cfg, [1, 0])
    for u, v in zip(a, one):
        assert v[0].tobytes() == u[1].tobytes()


# ------------------------------------------------------------------ sub-state cap
def test_substate_cap_is_an_error_return():
    """A segment of 40 m with an lvs length of 1 mm needs 40,001 states, more than
    THIP_CCSETS_MAX_SUBSTATES: the run names problem 0, segment 0, its rows are padded,
    and the object stays usable."""
    d = spherebot_desc()
    scene = sphere_rec((0.0, 0.0, 0.0), 0.5)[None, None]
    cs = ContinuousCollisionSets(d, 1, scene, ccfg(2, cm.LVS_CONTINUOUS, 1e-3, 0, 1, 0.1, 1.0, 0.01))
    try:
        with pytest.raises(HipError) as e:
            cs.run(np.array([[[-20.0, 0.0], [20.0, 0.0]]]))
        assert "problem 0 segment 0" in str(e.value) and "4096" in str(e.value), str(e.value)
        values, jac, coeffs, counts, keys = cs.run(np.array([[[-0.002, 0.9], [0.002, 0.9]]]))
        assert counts[0, 0] == 1 and abs(values[0, 0, 0] - 0.2) <= 1e-9
        with pytest.raises(HipError, match="x has"):
            cs.run(np.zeros((1, 1, 2)))
    finally:
        cs.close()


# ------------------------------------------------------------------ the host classes
@pytest.mark.parametrize("etype", [cm.LVS_CONTINUOUS, cm.LVS_DISCRETE], ids=["lvs_continuous", "lvs_discrete"])
def test_kin_continuous_sets_match_the_device_rows(etype):
    """ContinuousCollisionConstraint through the host classes: the rows of thip_ccsets_run
    for the environment's model (the built-in arm spheres), the jacobian in the two nodes'
    columns, one launch for both segments; the first segment's vars0 and the last
    segment's vars1 fixed."""
    _, scene, x0, lvs = config_c(0)
    d = abi.ProblemDesc.from_buffer_copy(problems.make_workload("C", 1, n_steps=3).desc)  # the built-in radii
    ccoll = [dict(first=0, last=2, margin=MARGIN, coeff=COEFF, buffer=BUFFER, max_num_cnt=3, penalty=tsqp.HINGE,
                  evaluator_type=etype, lvs_length=lvs, fixed_first=True, fixed_last=True)]
    r = tsqp.eval_kin(tsqp.make_spec(x0[0], []), tsqp.make_kin_spec("right_arm", ccoll=ccoll, prims=scene), x0)
    assert list(r["set_rows"]) == [3, 3] and r["launches"] == (0, 1)
    values, jac, coeffs, counts, _ = run_sets(d, scene[None], x0, ccfg(3, etype, lvs), [1, 2])
    D = 7
    for u in range(2):
        rows = slice(3 * u, 3 * u + 3)
        assert r["values"][0, rows].tobytes() == values[0, u].tobytes()
        for e in range(2):
            n = u + e
            assert r["jac"][0, rows, n * D:(n + 1) * D].tobytes() == jac[0, u, :, e].tobytes()
        other = np.delete(r["jac"][0, rows], np.s_[u * D:(u + 2) * D], axis=1)
        assert not other.any()
        assert r["coeffs"][0, rows].tobytes() == coeffs[0, u].tobytes()
        assert counts[0, u] > 3
    assert not jac[0, 0, :, 0].any() and not jac[0, 1, :, 1].any()  # the fixed ends
    assert np.abs(jac[0, 0, :, 1]).max() > 1e-2 and np.abs(jac[0, 1, :, 0]).max() > 1e-2
    assert np.all(np.isneginf(r["lower"])) and not r["upper"].any()


def test_kin_continuous_set_without_fixed_sparsity():
    """fixed_sparsity = false gives the same dense rows; rows past the sets are zero with
    value -buffer, and a row past them keeps its last coefficient."""
    xs = np.array([[[5.0, 5.0], [5.5, 5.0]], [[0.6, 0.0], [1.1, 0.0]]])
    spec = tsqp.make_spec(xs[0], [])
    out = {}
    for fixed in (False, True):
        ccoll = [dict(first=0, last=1, margin=0.2, coeff=4.0, buffer=0.05, max_num_cnt=3, fixed_sparsity=fixed,
                      evaluator_type=cm.LVS_CONTINUOUS, lvs_length=0.1)]
        out[fixed] = tsqp.eval_kin(spec, tsqp.make_kin_spec("manipulator", ccoll=ccoll), xs)
    r = out[False]
    print(r["values"], r["jac"], r["coeffs"])
    for key in ("values", "jac", "coeffs"):
        assert r[key].tobytes() == out[True][key].tobytes()
    assert list(r["set_rows"]) == [3] and r["launches"] == (0, 2)
    assert np.all(r["values"][0] == -0.05) and not r["jac"][0].any() and np.all(r["coeffs"][0] == 1.0)
    n = int((r["values"][1] > -0.05).sum())
    assert n >= 1 and np.all(r["coeffs"][1, :n] == 4.0) and np.all(r["coeffs"][1, n:] == 1.0)
    assert np.abs(r["jac"][1, 0]).max() > 0.1
