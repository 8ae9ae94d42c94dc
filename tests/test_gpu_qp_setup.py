"""The QP set-up's row-parallel Ruiz column norms and in-register block Cholesky
against the code they replace (MI355X).

build_and_scale (csrc/sqp_kernel.hip) takes the hinge rows' share of each Ruiz
column norm from a per-column maximum that the passes writing A_HC fold as they
go, and the CartPose rows' share with the loads issued together; factor() and
twisted_factor_half<8> factor and invert the narrow (D <= 8) diagonal blocks in
registers (chol_inv_block_reg).  abi.DEBUG_SETUP_REF makes the same binary walk
every row of a column serially and run the Cholesky through LDS with one lane
per row, which is what every call did before.  The norms are maxima of absolute
values, exact and independent of the order, and the Cholesky keeps every term
and its order, so every case solves its workload both ways and asks for
identical bits: the trajectories with np.array_equal, every Result field and
every QP trace record.

A case proves something only if its run goes through what the set-up feeds, so
each case also asserts from the QP trace that
  * some QP ended with rho != rho0 (a second factorisation of the scaled data);
  * some QP was polished (the delta factor);
and, for the cases with hinge rows, that the last QP of some problem had more
than 8 hinge rows in one step pair (the rows-per-pair table I_HPTR of the
workspace) and that the run met contacts at all (Result.n_contact_rows).  A
shape that misses one of these gets another first_problem, never a weaker
assertion.

Shapes: config B at n_steps 3, 4 and 32 (no hinge rows: the CartPose rows'
share alone; halves of 1/1, 2/1 and 16/15 blocks around the middle block, the
first block of a half without a coupling); config A (a CartPose constraint, 10
waypoints); config C (hinge rows) at batch 8, on the 8-dof torso_right_arm
(the full octet: no identity padding), and problem 833 alone, whose hundreds of hinge rows in one pair leave A_HC in HBM
(also checked against the oracle); and config C at 50 waypoints, which runs the
generic-step build of the kernel (sqp_kernel_gen).  Chains narrower than the
lane octet (robots.ROBOTS' right_arm_<k>dof: chol_inv_block_reg pads inside the
octet): config B on 1 dof at 3 waypoints and on 3 dofs, config C on 5 dofs, and
config B on 2 dofs with a JointAccEqCost -- waypoint-pair blocks of 4 dofs on the
generic-step build (the in-register Cholesky at sD = 4 with dense couplings).
"""
import ctypes as C

import numpy as np
import pytest

from parity import check_parity
from trajopt_amd import abi, problems
from trajopt_amd.runtime import BatchTrustRegionSQP

pytestmark = pytest.mark.gpu

I_HPTR = 8  # csrc/layout.hpp IArr: CSR of the hinge rows by step pair (N + 1)

# id -> (config, batch, make_workload keywords, hinge rows, generic-step build)
CASES = {
    "B-n3": ("B", 4, dict(n_steps=3, first_problem=4), False, False),
    "B-n4": ("B", 4, dict(n_steps=4, first_problem=0), False, False),
    "B-n32": ("B", 4, dict(n_steps=32, first_problem=0), False, False),
    "A-4": ("A", 4, dict(first_problem=0), False, False),
    "C-8": ("C", 8, dict(first_problem=0), True, False),
    "C-torso": ("C", 4, dict(robot="torso_right_arm", first_problem=0), True, False),
    "C-833": ("C", 1, dict(first_problem=833), True, False),
    "C-n50": ("C", 4, dict(n_steps=50, first_problem=0), True, True),
    "B-d1-n3": ("B", 4, dict(n_steps=3, robot="right_arm_1dof", first_problem=0), False, False),
    "B-d3": ("B", 4, dict(robot="right_arm_3dof", first_problem=0), False, False),
    "C-d5": ("C", 8, dict(robot="right_arm_5dof", first_problem=0), True, False),
    "B-acc-d2": ("B+acc", 4, dict(robot="right_arm_2dof", first_problem=0), False, True),
}
ORACLE_CASES = ("C-833",)


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()  # raises if the HIP library is missing
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


def make(cfg, batch, kw):
    """CASES' workload; '<config>+acc' adds a JointAccEqCost (waypoint-pair blocks)."""
    if cfg.endswith("+acc"):
        return problems.with_joint_acc(problems.make_workload(cfg[:-4], batch, **kw))
    return problems.make_workload(cfg, batch, **kw)


def solve(wl, path):
    """(x, results, per-problem QP trace, layout, most hinge rows of one step pair in a
    problem's last QP) of wl under thip_debug_set_path(path)."""
    lib = abi.load_hip()
    assert lib.thip_debug_set_path(path) == 0
    try:
        s = BatchTrustRegionSQP(wl, device=0)
        s.enable_trace(512)
        x, res = s.optimize()
        tr = s.get_trace()
        lay = s.layout()
        _, iws, _, ioff = s.debug_values()
        hp = iws[:, ioff[I_HPTR]: ioff[I_HPTR] + wl.n_steps + 1]
        pair_rows = int(np.diff(hp, axis=1).max())
        s.close()
    finally:
        lib.thip_debug_set_path(0)
    return x, res, tr, lay, pair_rows


def result_fields(r):
    out = {}
    for name, ctype in abi.Result._fields_:
        v = getattr(r, name)
        out[name] = list(v) if isinstance(v, C.Array) else v
    return out


def exercised(res, tr, pair_rows, hinge):
    """The conditions of the module docstring (QP trace record: 1 rho0, 4 polish_status, 5 final rho)."""
    qps = [rec for t in tr for rec in t]
    out = {
        "a QP that ended with rho != rho0": any(rec[5] != rec[1] for rec in qps),
        "a polished QP": any(rec[4] != 0 for rec in qps),
    }
    if hinge:
        out["a contact row"] = any(r.n_contact_rows > 0 for r in res)
        out["a step pair of more than 8 hinge rows"] = pair_rows > 8
    return out


@pytest.fixture(scope="module")
def runs():
    """Each case's row-parallel and serial solves, made once and shared."""
    cache = {}

    def get(name):
        if name not in cache:
            cfg, batch, kw, _, _ = CASES[name]
            wl = make(cfg, batch, kw)
            cache[name] = (wl, solve(wl, 0), solve(wl, abi.DEBUG_SETUP_REF))
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_setup_matches_serial_loops(runs, name):
    _, _, _, hinge, gen = CASES[name]
    wl, (x0, r0, t0, lay0, rows0), (x1, r1, t1, lay1, _) = runs(name)
    assert lay0 == lay1, f"{name}: the switch changed the solve layout ({lay0} vs {lay1})"
    assert lay0["gen"] == int(gen), f"{name}: runs the wrong build of the kernel ({lay0}), the case is vacuous"
    for b, t in enumerate(t0):
        assert len(t) == r0[b].n_qp_solves, f"{name}: problem {b}'s QP trace is cut short ({len(t)} records)"
    missing = [what for what, ok in exercised(r0, t0, rows0, hinge).items() if not ok]
    assert not missing, f"{name}: the run has no {'; no '.join(missing)}: choose another first_problem"
    assert np.array_equal(x0, x1), f"{name}: max |x - x serial| = {np.abs(x0 - x1).max():.3e}"
    for b in range(wl.batch):
        assert result_fields(r0[b]) == result_fields(r1[b]), f"{name}: problem {b}'s Result differs"
        assert np.array_equal(t0[b], t1[b]), f"{name}: problem {b}'s QP trace differs"


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_hbm_hinge_rows_problem_meets_parity(runs, oracle_mod, name):
    wl, (x0, r0, _, _, _), _ = runs(name)
    check_parity(wl, oracle_mod, x0, r0, label=f"qp-setup-{name}")
