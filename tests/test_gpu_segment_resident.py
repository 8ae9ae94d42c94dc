"""The resident ADMM segment against the return-at-every-check path (MI355X).

The segment's residual epilogue computes the third test of both infeasibility
certificates (max |D^-1 P dx|, and max |D^-1 A' dy| when the first two primal
tests pass), check_termination rejects a certificate on them without the full
function, and the segment decides for itself -- with the functions qp_solve()
uses -- whether qp_solve() would only say "carry on with the same rho"; then it
runs the next 25 iterations in place, without write-back and set-up
(csrc/sqp_kernel.hip: term_decide, admm_next_stop, admm_segment).
abi.DEBUG_SEG_RETURN makes the same binary ignore the third-test values and
return at every check, which is what every call did before.  No arithmetic that
reaches a result differs, so every case solves its workload both ways and asks
for identical bits: x, every Result field and every QP trace.

A case proves something only if its run exercises the change, so each case also
asserts, from the QP trace and get_profile(), that
  * the segment was entered fewer times than with the switch (slot 39);
  * fewer full dual-infeasibility checks ran than with the switch, and some ran
    with it (slot 28);
  * some QP ran more than 50 iterations (a stop passed in place) and some QP
    ended with rho != rho0 (a leave and a re-entry around a refactorisation);
  * the context runs the segment at all (layout()["seg_ok"]).
A shape that misses one of these gets another first_problem, never a weaker
assertion.

Shapes: config B (no hinge rows) at n_steps 3 and 32 (halves 1/1 and 16/15);
config C at batch 8 and on the 8-dof torso_right_arm (the full lane octet);
config C's problem 833 alone (hinge pack and A_HCT in HBM), also checked
against the oracle; and an infeasible config B (the fixed first waypoint 0.3
above joint 3's upper limit) at both lengths: every QP ends primal infeasible
(trace status 3) after a few hundred iterations and the run ends with status 4
-- the path on which all three precomputed tests pass and the full function
alone decides.  Chains narrower than the lane octet (robots.ROBOTS'
right_arm_<k>dof): config B on 1 dof at 3 waypoints and on 3 dofs, config C on
5 dofs.
"""
import ctypes as C

import numpy as np
import pytest

from parity import check_parity
from trajopt_amd import abi, problems
from trajopt_amd.runtime import BatchTrustRegionSQP

pytestmark = pytest.mark.gpu

CHECK_TERMINATION = 25
SLOT_DUAL_FULL = 28
SLOT_SEG_ENTRIES = 39
ST_PINF = 3  # QP trace status: primal infeasible
OPT_FAILED = 4  # Result.status (abi.OPT_STATUS)

# id -> (config, batch, make_workload keywords, infeasible)
CASES = {
    "B-n3": ("B", 4, dict(n_steps=3, first_problem=4), False),
    "B-n32": ("B", 4, dict(n_steps=32, first_problem=0), False),
    "C-8": ("C", 8, dict(first_problem=0), False),
    "C-torso": ("C", 4, dict(robot="torso_right_arm", first_problem=0), False),
    "C-833": ("C", 1, dict(first_problem=833), False),
    "B-n3-infeasible": ("B", 2, dict(n_steps=3, first_problem=0), True),
    "B-n32-infeasible": ("B", 2, dict(n_steps=32, first_problem=0), True),
    # chains narrower than the lane octet (pads of 7, 5 and 3 lanes)
    "B-d1-n3": ("B", 4, dict(n_steps=3, robot="right_arm_1dof", first_problem=0), False),
    "B-d3": ("B", 4, dict(robot="right_arm_3dof", first_problem=0), False),
    "C-d5": ("C", 8, dict(robot="right_arm_5dof", first_problem=0), False),
}
ORACLE_CASES = ("C-833",)


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()  # raises if the HIP library is missing
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


def make(cfg, batch, kw, infeasible):
    wl = problems.make_workload(cfg, batch, **kw)
    if infeasible:
        wl.init[:, wl.desc.fixed_steps[0], 3] = wl.desc.chain.upper[3] + 0.3
    return wl


def solve(wl, path):
    """(x, results, per-problem QP trace, layout, profile counters) of wl under thip_debug_set_path(path)."""
    lib = abi.load_hip()
    assert lib.thip_debug_set_path(path) == 0
    try:
        s = BatchTrustRegionSQP(wl, device=0)
        s.enable_trace(512)
        s.enable_profile(True)
        x, res = s.optimize()
        tr = s.get_trace()
        lay = s.layout()
        pf = s.get_profile()
        s.close()
    finally:
        lib.thip_debug_set_path(0)
    return x, res, tr, lay, pf


def result_fields(r):
    out = {}
    for name, ctype in abi.Result._fields_:
        v = getattr(r, name)
        out[name] = list(v) if isinstance(v, C.Array) else v
    return out


@pytest.fixture(scope="module")
def runs():
    """Each case's resident and return-at-every-check solves, made once and shared."""
    cache = {}

    def get(name):
        if name not in cache:
            cfg, batch, kw, infeasible = CASES[name]
            wl = make(cfg, batch, kw, infeasible)
            cache[name] = (wl, solve(wl, 0), solve(wl, abi.DEBUG_SEG_RETURN))
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_resident_matches_return_at_every_check(runs, name):
    wl, (x0, r0, t0, lay0, pf0), (x1, r1, t1, lay1, pf1) = runs(name)
    assert lay0["seg_ok"] == 1 and lay1["seg_ok"] == 1, f"{name}: not on the segment ({lay0}), the case is vacuous"
    for b, t in enumerate(t0):
        assert len(t) == r0[b].n_qp_solves, f"{name}: problem {b}'s QP trace is cut short ({len(t)} records)"
    # the run exercises the change (QP trace record: 1 rho0, 2 iterations, 3 status, 5 final rho)
    qps = [rec for t in t0 for rec in t]
    ent0, ent1 = int(pf0[:, SLOT_SEG_ENTRIES].sum()), int(pf1[:, SLOT_SEG_ENTRIES].sum())
    dual0, dual1 = int(pf0[:, SLOT_DUAL_FULL].sum()), int(pf1[:, SLOT_DUAL_FULL].sum())
    print(f"{name}: segment entries {ent0} vs {ent1} with the switch, full dual checks {dual0} vs {dual1}, "
          f"{len(qps)} QPs, longest {max(rec[2] for rec in qps):.0f} iterations")
    assert 0 < ent0 < ent1, f"{name}: segment entries {ent0} resident, {ent1} with the switch"
    assert dual1 > 0 and dual0 < dual1, f"{name}: full dual checks {dual0} resident, {dual1} with the switch"
    assert any(rec[2] > 2 * CHECK_TERMINATION for rec in qps), f"{name}: no QP of more than 50 iterations"
    assert any(rec[5] != rec[1] for rec in qps), f"{name}: no QP that ended with rho != rho0"
    # identical bits
    assert x0.shape == x1.shape and x0.tobytes() == x1.tobytes(), \
        f"{name}: max |x resident - x returning| = {np.abs(x0 - x1).max():.3e}"
    for b in range(wl.batch):
        assert result_fields(r0[b]) == result_fields(r1[b]), f"{name}: problem {b}'s Result differs"
        # (bytes, not values: an infeasible QP's record holds the NaN of its solution's norm)
        assert t0[b].shape == t1[b].shape and t0[b].tobytes() == t1[b].tobytes(), \
            f"{name}: problem {b}'s QP trace differs at (QP, field) {np.argwhere(~((t0[b] == t1[b]) | (np.isnan(t0[b]) & np.isnan(t1[b])))).tolist()}"
    if CASES[name][3]:
        for tr in (t0, t1):
            for b, t in enumerate(tr):
                assert len(t) > 0 and all(rec[3] == ST_PINF for rec in t), \
                    f"{name}: problem {b}'s QP statuses {[int(rec[3]) for rec in t]}, not all primal infeasible"
        for res in (r0, r1):
            assert all(r.status == OPT_FAILED for r in res), f"{name}: statuses {[r.status for r in res]}"


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_hbm_hinge_pack_problem_meets_parity(runs, oracle_mod, name):
    wl, (x0, r0, _, _, _), _ = runs(name)
    check_parity(wl, oracle_mod, x0, r0, label=f"segment-resident-{name}")
