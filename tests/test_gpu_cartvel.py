"""The CartVel term on the device (thip_eval_cart_vel_all, cart_vel_kernel) and
through the host loop: values and the analytic jacobian against the numpy FK of
trajopt_amd/robots.py (the fixture tests/golden/cartvel_pr2.npz and the same few
lines of numpy restated here), the jacobian's exact structure, independence of
the batch, horizons longer than one 64-waypoint pass, create-time validation,
and solves of a reaching problem whose tool step the term bounds.

The oracle does not read the cvel table: nothing here is compared against it."""
import ctypes as C
import functools
import json
import time
from pathlib import Path

import numpy as np
import pytest

from trajopt_amd import abi, host, problems
from trajopt_amd.robots import PR2_TOOL_LINK, ROBOTS, fwd_kin
from trajopt_amd.runtime import HipError, TermEvaluator

pytestmark = pytest.mark.gpu

ROBOT_NAMES = ("right_arm", "torso_right_arm", "both_arms")
CHUNK = 64  # waypoints per pass of cart_vel_kernel (kCvChunk)
CNT_TOL = 1e-4  # BasicTrustRegionSQPParameters::cnt_tolerance


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


# ------------------------------------------------------------------ numpy restatement
def _pos(chain, q, link):
    return fwd_kin(chain, q)[link][:3, 3]


def np_cart_vel(chain, x, terms):
    """x [B, N, D], terms [(link, first, last, d)] -> err [B, P, 6]."""
    out = []
    for b in range(x.shape[0]):
        rows = []
        for link, first, last, d in terms:
            p = np.array([_pos(chain, x[b, t], link) for t in range(first, last + 2)])
            for i in range(last - first + 1):
                rows.append(np.concatenate([(p[i + 1] - p[i]) - d, (p[i] - p[i + 1]) - d]))
        out.append(rows)
    return np.array(out)


def _workload(robot, x, terms):
    d = problems.base_desc(x.shape[1], robot)
    wl = problems.Workload("cart_vel", d, np.ascontiguousarray(x), np.zeros((x.shape[0], 0, 12)),
                           np.zeros((x.shape[0], 0, 16)), x.copy())
    for link, first, last, disp in terms:
        problems.with_cart_vel(wl, link, first, last, disp, is_cnt=True)
    return wl


def _golden_case(golden, robot):
    g = golden("cartvel_pr2")
    links, disps = g[f"{robot}_links"], g[f"{robot}_d"]
    terms = [(int(links[k]), int(f), int(l), float(disps[k])) for k, (f, l) in enumerate(g["term_steps"])]
    return g, g[f"{robot}_x"], terms


@functools.lru_cache(maxsize=None)
def _device_values(robot):
    """(err, jac) of the fixture's batch of 3, evaluated once per robot."""
    g = dict(np.load(Path(__file__).resolve().parent / "golden" / "cartvel_pr2.npz"))
    links, disps = g[f"{robot}_links"], g[f"{robot}_d"]
    terms = [(int(links[k]), int(f), int(l), float(disps[k])) for k, (f, l) in enumerate(g["term_steps"])]
    ev = TermEvaluator(_workload(robot, g[f"{robot}_x"], terms))
    err, jac = ev.cart_vel(g[f"{robot}_x"])
    ev.close()
    return err, jac


# ------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("robot", ROBOT_NAMES)
def test_values_against_the_numpy_fk(golden, robot):
    g, x, terms = _golden_case(golden, robot)
    assert x.shape[:2] == (3, 4) and [t[1:3] for t in terms] == [(0, 2), (1, 2)]
    if robot == "right_arm":  # the reference's own derivative-test point is a waypoint
        assert (x[0, 0] == g["ref_point"]).all()
    if robot == "both_arms":
        assert terms[0][0] == 22 and terms[1][0] <= 11  # right tool, then a left-arm link
    err, jac = _device_values(robot)
    chain = ROBOTS[robot][0]()
    ref = np_cart_vel(chain, x, terms)
    d_fix, d_np = np.abs(err - g[f"{robot}_err"]).max(), np.abs(err - ref).max()
    d_jac = np.abs(jac - g[f"{robot}_jac_fd"]).max()
    print(f"{robot}: |err - fixture| {d_fix:.3e}, |err - numpy| {d_np:.3e}, |jac - central differences| {d_jac:.3e}")
    assert err.shape == (3, 5, 6) and jac.shape == (3, 5, 6, 2 * chain.n_dof)
    assert d_fix <= 1e-12 and d_np <= 1e-12
    # central differences, h = 1e-6: truncation h^2 |p'''| / 6 <= 3e-13 for a reach under
    # 1.5 m, rounding eps |p| / h ~ 3e-10
    assert d_jac <= 1e-8


# ------------------------------------------------------------------ 2. structure
@pytest.mark.parametrize("robot", ROBOT_NAMES)
def test_jacobian_structure_is_exact(golden, robot):
    g, x, terms = _golden_case(golden, robot)
    err, jac = _device_values(robot)
    chain = ROBOTS[robot][0]()
    D = chain.n_dof
    assert (jac[:, :, 3:6].view(np.int64) == (-jac[:, :, 0:3]).view(np.int64)).all()
    # the linear jacobian of each waypoint, recovered from the pair that starts there
    # (-J0) and from the pair that ends there (+J1): the same bits
    pair_terms = [k for k, (_, f, l, _) in enumerate(terms) for _ in range(f, l + 1)]
    for p in range(1, len(pair_terms)):
        if pair_terms[p] == pair_terms[p - 1]:
            assert (jac[:, p, 0:3, :D] == -jac[:, p - 1, 0:3, D:]).all()
    # columns of joints off the link's path are zero in both halves
    for p, k in enumerate(pair_terms):
        link = terms[k][0]
        on = set()
        while link > 0:
            if chain.joint_type[link] != abi.JOINT_FIXED:
                on.add(chain.joint_dof[link])
            link = chain.parent[link]
        off = [j for j in range(D) if j not in on]
        assert off or k == 0  # the mid-chain link always has joints past it
        for half in (0, D):
            assert (jac[:, p][:, :, [half + j for j in off]] == 0.0).all()
        # the shoulder joints move every link here
        first_on = min(on)
        assert (np.abs(jac[:, p, 0:3, first_on]).max(axis=1) > 1e-3).all()
    if robot == "right_arm":
        # the forearm link (term 1, pairs 3 and 4): the wrist columns, in both halves
        assert (jac[:, 3:5][..., [5, 6, 12, 13]] == 0.0).all()
    if robot == "both_arms":
        # the right tool (term 0) does not see the left arm; the left forearm (term 1) sees
        # neither its own wrist nor any of the right arm
        assert (jac[:, 0:3][..., list(range(0, 7)) + list(range(14, 21))] == 0.0).all()
        assert (jac[:, 3:5][..., list(range(5, 14)) + list(range(19, 28))] == 0.0).all()
    # err[0:3] + err[3:6] = -2 d: each half rounds a value below 2 d (the fixture keeps
    # |dp| <= d), the sum rounds once more
    for p, k in enumerate(pair_terms):
        d = terms[k][3]
        assert (np.abs(err[:, p, 0:3] + err[:, p, 3:6] + 2 * d) <= 4 * np.spacing(d)).all()


# ------------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("robot", ("right_arm", "both_arms"))
def test_bitwise_independent_of_the_batch_and_repeatable(golden, robot):
    _, x, terms = _golden_case(golden, robot)
    err, jac = _device_values(robot)
    ev = TermEvaluator(_workload(robot, x, terms))
    err2, jac2 = ev.cart_vel(x)
    err3, none = ev.cart_vel(x, jac=False)
    ev.close()
    assert none is None
    assert (err2.view(np.int64) == err.view(np.int64)).all() and (jac2.view(np.int64) == jac.view(np.int64)).all()
    assert (err3.view(np.int64) == err.view(np.int64)).all()
    for b in range(3):
        ev1 = TermEvaluator(_workload(robot, x[b:b + 1], terms))
        e1, j1 = ev1.cart_vel(x[b:b + 1])
        ev1.close()
        assert (e1[0].view(np.int64) == err[b].view(np.int64)).all()
        assert (j1[0].view(np.int64) == jac[b].view(np.int64)).all()


# ------------------------------------------------------------------ 4. chunking
def test_horizon_longer_than_two_passes():
    """N = 2 * 64 + 2: two full 64-waypoint passes and a remainder of two waypoints."""
    n = 2 * CHUNK + 2
    chain = ROBOTS["right_arm"][0]()
    rng = np.random.default_rng(7)
    q0 = rng.uniform(-0.5, 0.5, size=(2, 1, 7)) + np.array([-0.8, 0.4, -1.2, -1.2, 0.3, -0.8, 0.2])
    x = q0 + np.cumsum(rng.uniform(-0.02, 0.02, size=(2, n, 7)), axis=1)
    terms = [(PR2_TOOL_LINK, 0, n - 2, 0.05)]
    ev = TermEvaluator(_workload("right_arm", x, terms))
    err, jac = ev.cart_vel(x)
    ev.close()
    ref = np_cart_vel(chain, x, terms)
    assert err.shape == (2, n - 1, 6)
    diff = np.abs(err - ref).max(axis=(0, 2))
    print(f"N = {n}: max |err - numpy| {diff.max():.3e} (pair {int(diff.argmax())})")
    assert diff.max() <= 1e-12
    # the pairs that join two passes (waypoints 63|64 and 127|128) carry the same jacobians
    for p in (CHUNK - 1, 2 * CHUNK - 1):
        assert (jac[:, p, 0:3, 7:] == -jac[:, p + 1, 0:3, :7]).all()
        assert (jac[:, p, 0:3, :7] == -jac[:, p - 1, 0:3, 7:]).all()


# ------------------------------------------------------------------ 5. validation
def _create_error(desc, hip):
    ev = C.c_void_p()
    rc = hip.thip_eval_create(0, C.byref(desc), 1, C.byref(ev))
    assert rc == -1 and not ev.value  # THIP_E_INVALID: refused before any device call
    return hip.thip_eval_last_error(None).decode()


def test_create_validates_the_table(hip):
    x = np.zeros((1, 6, 7))
    ok = _workload("right_arm", x, [(PR2_TOOL_LINK, 0, 4, 0.1)])
    TermEvaluator(ok).close()
    msg = _create_error(_workload("right_arm", x, [(PR2_TOOL_LINK, 0, 5, 0.1)]).desc, hip)
    assert "last_step + 1 = 6" in msg and "n_steps - 1 = 5" in msg, msg
    fixed = _workload("right_arm", x, [(1, 0, 4, 0.1)])
    fixed.desc.chain.joint_type[1] = abi.JOINT_FIXED  # link 1 no longer moves
    fixed.desc.chain.joint_dof[1] = -1
    msg = _create_error(fixed.desc, hip)
    assert "link 1 is not moved by a joint" in msg, msg
    for bad, needle in (((0, 0, 4, 0.1), "link 0 outside"), ((PR2_TOOL_LINK, 3, 3, 0.1), "first_step 3, last_step 3"),
                        ((PR2_TOOL_LINK, 0, 4, float("inf")), "max_displacement is not finite")):
        msg = _create_error(_workload("right_arm", x, [bad]).desc, hip)
        assert needle in msg, msg
    with pytest.raises(HipError, match="CartVel term 0"):
        TermEvaluator(_workload("right_arm", x, [(PR2_TOOL_LINK, -1, 4, 0.1)]))


# ------------------------------------------------------------------ 6 - 8. solves
N_SOLVE, PAIRS = 10, (3, 4, 5)
START = np.array([-0.9, 0.2, -1.0, -0.8, 0.2, -0.5, 0.1])
GOALS = [np.array([0.2, 0.7, -1.7, -1.7, 0.6, -1.1, 0.5]),
         np.array([0.1, 0.8, -1.5, -1.8, 0.4, -0.9, 0.3]),
         np.array([0.3, 0.6, -1.9, -1.6, 0.7, -1.2, 0.6])]


def _solve_text(goal, term=None, as_cost=False):
    init = [(START + (goal - START) * t / (N_SOLVE - 1)).tolist() for t in range(N_SOLVE)]
    doc = {
        "basic_info": {"n_steps": N_SOLVE, "manip": "right_arm", "fixed_timesteps": [0]},
        "costs": [{"type": "joint_vel", "params": {"coeffs": [1.0] * 7, "targets": [0.0] * 7}}],
        "constraints": [{"type": "joint_pos", "params": {"coeffs": [1.0] * 7, "targets": goal.tolist(),
                                                         "first_step": N_SOLVE - 1, "last_step": N_SOLVE - 1}}],
        "init_info": {"type": "given_traj", "data": init},
    }
    if term is not None:
        (doc["costs"] if as_cost else doc["constraints"]).append(term)
    return json.dumps(doc)


def _cart_vel_term(d):
    return {"type": "cart_vel", "params": {"link": "r_gripper_tool_frame", "first_step": PAIRS[0],
                                           "last_step": PAIRS[-1], "max_displacement": d}}


def _tool_steps(x):
    """per-axis |dp| of the tool over pairs 3 to 5: [3, 3]."""
    chain = ROBOTS["right_arm"][0]()
    p = np.array([_pos(chain, x[t], PR2_TOOL_LINK) for t in range(PAIRS[0], PAIRS[-1] + 2)])
    return np.abs(np.diff(p, axis=0))


@functools.lru_cache(maxsize=None)
def _unconstrained(k):
    x, res, native = host.solve_json(_solve_text(GOALS[k]))
    assert native and res.status == 0
    chain = ROBOTS["right_arm"][0]()
    assert np.linalg.norm(_pos(chain, x[-1], PR2_TOOL_LINK) - _pos(chain, x[0], PR2_TOOL_LINK)) >= 0.3
    return x, float(_tool_steps(x).max())


def test_solve_with_the_constraint(hip):
    x0, u = _unconstrained(0)
    d = 0.4 * u
    t0 = time.perf_counter()
    x, res, native = host.solve_json(_solve_text(GOALS[0], _cart_vel_term(d)))
    wall = time.perf_counter() - t0
    steps = _tool_steps(x)
    print(f"u {u:.4f} m, bound {d:.4f} m, constrained max step {steps.max():.6f} m, status "
          f"{abi.OPT_STATUS[res.status]}, {res.n_sqp_iters} SQP iterations, {res.n_qp_solves} QPs, {wall:.2f} s")
    assert not native  # the host loop with device-evaluated terms
    assert res.status == 0, abi.OPT_STATUS[res.status]  # OPT_CONVERGED
    assert (steps <= d + CNT_TOL).all(), steps
    assert (x[0] == START).all()
    assert np.abs(x[-1] - GOALS[0]).max() <= CNT_TOL
    # the term objects' own violations: joint_pos, then one CartVel constraint per pair
    _, _, _, viols = host.solve_json_batch_terms([_solve_text(GOALS[0], _cart_vel_term(d))], drop_in=True)
    assert viols.shape == (1, 1 + len(PAIRS)) and (viols[0, 1:] <= CNT_TOL).all(), viols
    # by construction the unconstrained solution breaks the bound by 2.5 x
    assert _tool_steps(x0).max() >= 2.4 * d


def test_solve_with_the_cost(hip):
    x0, u = _unconstrained(0)
    d = 0.4 * u
    text = _solve_text(GOALS[0], _cart_vel_term(d), as_cost=True)
    xs, res, costs, viols = host.solve_json_batch_terms([text], drop_in=True)
    x = xs[0]
    over0 = np.maximum(_tool_steps(x0) - d, 0.0).sum()
    over = np.maximum(_tool_steps(x) - d, 0.0).sum()
    print(f"sum of excess over pairs 3..5: unconstrained {over0:.6f} m, with the cost {over:.6f} m, status "
          f"{abi.OPT_STATUS[res[0].status]}")
    assert over < over0
    # joint_vel, then one CartVel cost per pair: sum |err| over its six rows
    chain = ROBOTS["right_arm"][0]()
    ref = np.abs(np_cart_vel(chain, x[None], [(PR2_TOOL_LINK, PAIRS[0], PAIRS[-1], d)])[0]).sum(axis=1)
    assert costs.shape == (1, 1 + len(PAIRS))
    assert np.abs(costs[0, 1:] - ref).max() <= 1e-9, (costs[0, 1:], ref)


def test_batch_equals_single_solves_bitwise(hip):
    texts = []
    for k in range(3):
        _, u = _unconstrained(k)
        texts.append(_solve_text(GOALS[k], _cart_vel_term(0.4 * u)))
    xb, resb = host.solve_json_batch(texts)
    for k in range(3):
        x, res, native = host.solve_json(texts[k])
        assert not native and res.status == resb[k].status
        assert (x.view(np.int64) == xb[k].view(np.int64)).all(), f"problem {k}: max |dx| {np.abs(x - xb[k]).max():.3e}"
