"""The SQP driver's sparsity fingerprint taken by the whole workgroup against
thread 0's serial walk of A (MI355X).

After every QP set-up sqp_optimize (csrc/sqp_kernel.hip) asks what OSQPModel
asks (quirk Q2): do n, m, nnz and the compared byte prefixes of A's column
pointers and row indices equal those of the previous set-up?  The answer
decides whether the QP is warm-started.  pattern_fingerprint_wg answers with
one thread per column, a scan of the columns' entry counts and an
order-independent 64-bit sum (csrc/pattern_fp.hpp; the index arithmetic is
checked on the host by tests/test_pattern_fp.py); abi.DEBUG_FP_REF makes the
same binary run the serial walk every call ran before.  Only the yes / no is
used, so every case solves its workload both ways and asks for identical bits:
the trajectories with np.array_equal, every Result field and every QP trace
record.

A case proves something only if both answers occur in its run, so each case
also asserts from the QP trace (record field 0: warm start, field 15: the
step's decision, 2 = rejected) that after some problem's first QP there is a
warm-started QP and a cold one.  A QP that follows a rejected step or a failed
QP reuses the set-up and is warm-started whatever the fingerprint says; only a
QP that follows an accepted or converged step opens a new SQP iteration with a
new set-up.  So the cases marked below (those whose runs hold one, on either
path: the traces are the same) also assert a warm-started QP among the latter,
which is an "equal" from the fingerprint itself; every cold QP after the first
is an "unequal" from it.

Shapes: config B (no hinge rows) at 3 and 30 waypoints; config C (hinge rows)
at batch 8, on the 8-dof torso_right_arm, at 3 waypoints on problems 4..7 (one
without a hinge row; the pointer prefix ends among the aux or hinge columns),
problem 833 alone (hundreds of hinge rows in a step pair), and at 50 waypoints,
which runs the generic-step build (sqp_kernel_gen; 350 x columns on 256
threads: two column chunks).  Chains narrower than the lane octet
(robots.ROBOTS' right_arm_<k>dof): config B on 2 dofs at 3 waypoints and on 3
dofs, config C on 5 dofs.  The 1-dof chain is left to the other two-path
modules: its single Jacobian column never changes pattern (no cold QP after the
first in any of problems 0..4095 of config B at 3 waypoints, by the oracle's QP
trace), so "both answers occur" cannot hold on it; 2 dofs is the narrowest chain
on which it does.
"""
import ctypes as C

import numpy as np
import pytest

from trajopt_amd import abi, problems
from trajopt_amd.runtime import BatchTrustRegionSQP

pytestmark = pytest.mark.gpu

# id -> (config, batch, make_workload keywords, generic-step build, the run holds a warm-started QP that
# opens an SQP iteration)
CASES = {
    "B-n3": ("B", 4, dict(n_steps=3), False, True),
    "B-n30": ("B", 4, dict(n_steps=30), False, True),
    "C-8": ("C", 8, dict(), False, True),
    "C-torso": ("C", 4, dict(robot="torso_right_arm"), False, False),
    "C-n3": ("C", 4, dict(n_steps=3, first_problem=4), False, True),
    "C-833": ("C", 1, dict(first_problem=833), False, False),
    "C-n50": ("C", 4, dict(n_steps=50), True, True),
    "B-d2-n3": ("B", 4, dict(n_steps=3, robot="right_arm_2dof"), False, True),
    "B-d3": ("B", 4, dict(robot="right_arm_3dof"), False, True),
    "C-d5": ("C", 8, dict(robot="right_arm_5dof"), False, True),
}


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


def warm_counts(tr):
    """(warm, cold) QPs after each problem's first, and the same among the QPs that
    open a new SQP iteration (their predecessor's step was accepted or converged)."""
    later = [rec[0] for t in tr for rec in t[1:]]
    decided = [t[k][0] for t in tr for k in range(1, len(t)) if t[k - 1][15] in (1.0, 3.0)]
    return (sum(v == 1 for v in later), sum(v == 0 for v in later),
            sum(v == 1 for v in decided), sum(v == 0 for v in decided))


@pytest.fixture(scope="module")
def runs():
    """Each case's workgroup and serial solves, made once and shared."""
    cache = {}

    def get(name):
        if name not in cache:
            cfg, batch, kw, _, _ = CASES[name]
            wl = problems.make_workload(cfg, batch, **kw)
            cache[name] = (wl, solve(wl, 0), solve(wl, abi.DEBUG_FP_REF))
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_fingerprint_matches_serial_walk(runs, name):
    _, _, _, gen, own_equal = CASES[name]
    wl, (x0, r0, t0, lay0), (x1, r1, t1, lay1) = runs(name)
    assert lay0 == lay1, f"{name}: the switch changed the solve layout ({lay0} vs {lay1})"
    assert lay0["gen"] == int(gen), f"{name}: runs the wrong build of the kernel ({lay0}), the case is vacuous"
    for b, t in enumerate(t0):
        assert len(t) == r0[b].n_qp_solves, f"{name}: problem {b}'s QP trace is cut short ({len(t)} records)"
    warm, cold, dwarm, dcold = warm_counts(t0)
    print(f"{name}: after the first QP {warm} warm, {cold} cold; decided by the fingerprint {dwarm} warm, {dcold} cold")
    assert warm > 0 and cold > 0, f"{name}: {warm} warm and {cold} cold QPs after the first: one answer never occurs"
    assert dcold > 0 and (dwarm > 0 or not own_equal), (f"{name}: of the QPs that open an SQP iteration {dwarm} are "
                                                        f"warm and {dcold} cold")
    assert np.array_equal(x0, x1), f"{name}: max |x - x serial| = {np.abs(x0 - x1).max():.3e}"
    for b in range(wl.batch):
        assert result_fields(r0[b]) == result_fields(r1[b]), f"{name}: problem {b}'s Result differs"
        assert np.array_equal(t0[b], t1[b]), f"{name}: problem {b}'s QP trace differs"
