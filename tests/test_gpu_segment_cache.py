"""The ADMM segment's kept packs against the rebuild-every-call path (MI355X).

The segment builds its chain pack once per factorisation and its hinge-row
set-up once per QP (Ctl::qp_stamp / fac_stamp in csrc/sqp_kernel.hip);
abi.DEBUG_SEG_REBUILD makes the same binary rebuild both at every call, which is
what every call did before.  No arithmetic differs between the two, so every
case solves its workload both ways and asks for identical bits: the trajectories
with np.array_equal and every Result field.

A case proves something only if its run meets what a stale pack would get
wrong, so each case also asserts from the QP trace that
  * some QP ran more than 25 iterations (check_termination = 25: a second
    segment call, the first one that reuses anything);
  * some QP ended with rho != rho0 (a refactorisation inside a QP: a stale
    chain pack or a stale 1 / (DG + rho w^2));
  * some problem solved more QPs than it made SQP iterations (a second QP on one
    convexification);
  * some polished QP is followed by another QP of its problem (polish's
    factor() overwrote the factor the pack was built from);
and that the context runs the segment at all (layout()["seg_ok"]).  A shape that
misses one of these gets another first_problem, never a weaker assertion.

Shapes: config B (no hinge rows: the chain pack alone) at n_steps 3, 4 and 32 --
tw_mid = N / 2, so the halves are 1/1, 2/1 and 16/15: the shortest and the
unequal halves, which rely on pad slots zeroed once per factorisation, and all
kCpkSteps steps (n_steps = 2, a missing half, runs on the segment but solves
every problem 0..95 in one QP of at most 75 iterations with no rho update, so
it can meet only the first condition and is left out); config C (hinge rows) at
batch 8 and on
the 8-dof torso_right_arm (the full lane octet); and config C's problems 435 and
833 alone, whose ~436 and ~758 mean hinge rows put the hinge pack in HBM with
A_HCT in LDS, and both in HBM.  Those two are also checked against the oracle.
Chains narrower than the lane octet (robots.ROBOTS' right_arm_<k>dof: blocks
padded with identity from 1, 3 and 5 dofs up to 8 lanes): config B on 1 dof at 3
waypoints and on 3 dofs, config C on 5 dofs.
"""
import ctypes as C

import numpy as np
import pytest

from parity import check_parity
from trajopt_amd import abi, problems
from trajopt_amd.runtime import BatchTrustRegionSQP

pytestmark = pytest.mark.gpu

CHECK_TERMINATION = 25

# id -> (config, batch, make_workload keywords)
CASES = {
    "B-n3": ("B", 4, dict(n_steps=3, first_problem=4)),
    "B-n4": ("B", 4, dict(n_steps=4, first_problem=0)),
    "B-n32": ("B", 4, dict(n_steps=32, first_problem=0)),
    "C-8": ("C", 8, dict(first_problem=0)),
    "C-torso": ("C", 4, dict(robot="torso_right_arm", first_problem=0)),
    "C-435": ("C", 1, dict(first_problem=435)),
    "C-833": ("C", 1, dict(first_problem=833)),
    # chains narrower than the lane octet; windows with a rejected step (problems 102 and 43:
    # none of problems 0..95 on 1 dof and 0..31 on 3 dofs solves a second QP on one convexification)
    "B-d1-n3": ("B", 4, dict(n_steps=3, robot="right_arm_1dof", first_problem=100)),
    "B-d3": ("B", 4, dict(robot="right_arm_3dof", first_problem=40)),
    "C-d5": ("C", 8, dict(robot="right_arm_5dof", first_problem=0)),
}
ORACLE_CASES = ("C-435", "C-833")


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()  # raises if the HIP library is missing
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


def solve(wl, path):
    """(x, results, per-problem QP trace, layout) of wl under thip_debug_set_path(path)."""
    lib = abi.load_hip()
    assert lib.thip_debug_set_path(path) == 0
    try:
        s = BatchTrustRegionSQP(wl, device=0)
        s.enable_trace(512)
        x, res = s.optimize()
        tr = s.get_trace()
        lay = s.layout()
        s.close()
    finally:
        lib.thip_debug_set_path(0)
    return x, res, tr, lay


def result_fields(r):
    out = {}
    for name, ctype in abi.Result._fields_:
        v = getattr(r, name)
        out[name] = list(v) if isinstance(v, C.Array) else v
    return out


def exercised(res, tr):
    """The four conditions of the module docstring, from the QP trace (record:
    1 rho0, 2 iterations, 4 polish_status, 5 final rho)."""
    qps = [rec for t in tr for rec in t]
    return {
        "a QP of more than 25 iterations": any(rec[2] > CHECK_TERMINATION for rec in qps),
        "a QP that ended with rho != rho0": any(rec[5] != rec[1] for rec in qps),
        "a problem with n_qp_solves > n_sqp_iters": any(r.n_qp_solves > r.n_sqp_iters for r in res),
        "a polished QP followed by another QP": any(rec[4] != 0 for t in tr for rec in t[:-1]),
    }


@pytest.fixture(scope="module")
def runs():
    """Each case's kept and rebuilt solves, made once and shared."""
    cache = {}

    def get(name):
        if name not in cache:
            cfg, batch, kw = CASES[name]
            wl = problems.make_workload(cfg, batch, **kw)
            cache[name] = (wl, solve(wl, 0), solve(wl, abi.DEBUG_SEG_REBUILD))
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_kept_packs_match_rebuild(runs, name):
    wl, (x0, r0, t0, lay0), (x1, r1, t1, lay1) = runs(name)
    assert lay0["seg_ok"] == 1 and lay1["seg_ok"] == 1, f"{name}: not on the segment ({lay0}), the case is vacuous"
    for b, t in enumerate(t0):
        assert len(t) == r0[b].n_qp_solves, f"{name}: problem {b}'s QP trace is cut short ({len(t)} records)"
    missing = [what for what, ok in exercised(r0, t0).items() if not ok]
    assert not missing, f"{name}: the run has no {'; no '.join(missing)}: choose another first_problem"
    assert np.array_equal(x0, x1), f"{name}: max |x kept - x rebuilt| = {np.abs(x0 - x1).max():.3e}"
    for b in range(wl.batch):
        assert result_fields(r0[b]) == result_fields(r1[b]), f"{name}: problem {b}'s Result differs"
        assert np.array_equal(t0[b], t1[b]), f"{name}: problem {b}'s QP trace differs"


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_hbm_hinge_pack_problems_meet_parity(runs, oracle_mod, name):
    wl, (x0, r0, _, _), _ = runs(name)
    check_parity(wl, oracle_mod, x0, r0, label=f"segment-cache-{name}")
