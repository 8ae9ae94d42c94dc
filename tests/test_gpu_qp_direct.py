"""The generic QP kernel (csrc/qp_csc.hip) measured directly against the OSQP
oracle, one QP at a time, on the catalogue of tests/qp_cases.py (MI355X).

The catalogue is proved on the CPU first (tests/test_qp_cases.py): every case
returns the same status, iterations, polish status and rho updates from ten
roundings of the oracle, so there is no "oracle is unstable" escape here.

Rules applied to every device solve (check_solve):
  * discrete parity: status, setup_error, iter and polish_status equal the
    oracle's; rho at exit within 10 x the oracle's own rerun spread of rho;
    x and y all NaN for the infeasible statuses;
  * unpolished outputs: x, y, prim_res and dual_res within 10 x the oracle's
    rerun spread of each (a draw from the same rounding distribution lies
    outside an n-point envelope with probability 2 / (n + 2); the factor 10
    covers the ten-point envelope's own sampling error);
  * polished outputs: the error of x and of y against the long-double KKT
    solution (x*, y*) at most max(10 x the oracle's error against it,
    cond_1(K_active) 2^-53 |(x*, y*)|_inf), the forward-error bound of the
    reduced KKT solve; prim_res and dual_res at most max(10 x the oracle's,
    that bound);
  * status 1: OSQP's termination guarantee recomputed in long double from the
    device's (x, y).
No tolerance comes from the device.  Each case runs through its own thip_qp
object, and a test that needs a storage tier asserts from thip_qp_shape that
the object is in it: a case in the wrong tier fails as vacuous.
"""
import numpy as np
import pytest

import qp_cases
import qp_reference as R
from qp_cases import CASES
from qp_device import E_STATE, GpuQp

pytestmark = pytest.mark.gpu

GAPS = []  # (label, quantity, device gap, tolerance): tools/qp_direct_gaps.py reads it
TIER_CASE = {1: "mixed12", 2: "tier2", 3: "tier3_polished"}


@pytest.fixture(scope="module", autouse=True)
def _built(oracle_mod):
    from trajopt_amd import abi

    abi.load_hip()  # raises when the library was not built
    return oracle_mod


def _gap(label, what, gap, tol):
    GAPS.append((label, what, float(gap), float(tol)))
    print(f"{label:34s} {what:9s} gap {gap:.3e} tol {tol:.3e}")
    return gap <= tol


def check_solve(label, case, got, ref, spread, star):
    """One device solve `got` = (x, y, info) of `case` against the oracle's exact run
    `ref`, its rerun spreads and (polished solves) the long-double reference."""
    x, y, info = got
    xo, yo, io = ref
    bad = []
    for k in ("status", "setup_error", "iter", "polish_status"):
        if info[k] != io[k]:
            bad.append(f"{k} {info[k]} != oracle {io[k]}")
    print(f"{label:34s} status {info['status']} iter {info['iter']} polish {info['polish_status']} rho {info['rho']:.6g}")
    if io["status"] == -1:
        assert not bad, (label, bad)
        return
    if not _gap(label, "rho", abs(info["rho"] - io["rho"]), 10 * spread["rho"]):
        bad.append("rho")
    if io["status"] in (3, 4, 5, 6):
        if not (np.isnan(x).all() and np.isnan(y).all()):
            bad.append("x, y are not all NaN")
        assert not bad, (label, bad)
        return
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        bad.append("x or y is not finite")
        assert not bad, (label, bad)
    if io["polish_status"] == 1:
        for what, g, o, s in (("x", x, xo, star.x), ("y", y, yo, star.y)):
            if not _gap(label, what + " - " + what + "*", R.err_inf(g, s), max(10 * R.err_inf(o, s), star.forward)):
                bad.append(what)
        for what in ("prim_res", "dual_res"):
            if not _gap(label, what, abs(info[what]), max(10 * abs(io[what]), star.forward)):
                bad.append(what)
    else:
        for what, g, o in (("x", x, xo), ("y", y, yo)):
            if not _gap(label, what, R.err_inf(g, o), 10 * spread[what]):
                bad.append(what)
        for what in ("prim_res", "dual_res"):
            if not _gap(label, what, abs(info[what] - io[what]), 10 * spread[what]):
                bad.append(what)
    if io["status"] == 1:
        prim, ptol, dual, dtol = R.termination_gaps(case, x, y)
        if not (_gap(label, "term prim", prim, ptol) and _gap(label, "term dual", dual, dtol)):
            bad.append("termination guarantee")
    assert not bad, (label, bad)


def check_case(name, got, label=None):
    rr = R.reruns(name)
    polished = rr.info["status"] == 1 and rr.info["polish_status"] == 1
    check_solve(label or name, CASES[name], got, rr.runs[0], rr.spread, R.kkt_star(name) if polished else None)


def same_bits(a, b):
    (xa, ya, ia), (xb, yb, ib) = a, b
    return np.array_equal(xa, xb, equal_nan=True) and np.array_equal(ya, yb, equal_nan=True) and ia == ib


def solve_alone(name, level_solve=False):
    c = CASES[name]
    qp = GpuQp(c, 1, level_solve=level_solve)
    try:
        assert qp.tier() == c.tier, (name, qp.shape())
        return qp.solve([c], qp_cases.settings_of(c))[0], qp.shape()
    finally:
        qp.close()


@pytest.fixture(scope="module")
def alone():
    """Every catalogue case solved once through its own batch-1 object."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = solve_alone(name)
        return cache[name]

    return get


# ------------------------------------------------------------------ every case
@pytest.mark.parametrize("name", list(CASES))
def test_case_against_oracle(alone, name):
    got, shape = alone(name)
    c = CASES[name]
    if c.tier == 1:
        assert shape[4] == 1
    elif c.tier == 2:
        assert shape[4] == 0 and shape[5] > 0
    else:
        assert shape[5] == 0 and shape[0] > 8192
        print(f"{name}: N {shape[0]} entries of L {shape[1]} tree levels {shape[2]} widest level {shape[3]}")
    check_case(name, got)


# ------------------------------------------------------------------ two schedules
@pytest.mark.parametrize("tier", [1, 2, 3])
def test_level_solve_is_the_same_sums(alone, tier):
    """THIP_QP_LEVEL_SOLVE=1 runs the forward solve level by level instead of in
    passes of row segments: the same sums, so the same bits."""
    import os

    name = TIER_CASE[tier]
    before = os.environ.get("THIP_QP_LEVEL_SOLVE")
    lev, shape = solve_alone(name, level_solve=True)
    assert os.environ.get("THIP_QP_LEVEL_SOLVE") == before
    assert shape == alone(name)[1]
    assert same_bits(lev, alone(name)[0])


# ------------------------------------------------------------------ batch isolation
def _infeasible_twin(c):
    """c with the bounds of its fullest row moved out of reach of the box rows
    (every variable of the catalogue's tier cases is boxed into |x_j| <= 1): the same
    pattern, primal infeasible."""
    rows = c.A.tocsr()
    counts = np.diff(rows.indptr)
    r = int(np.argmax(counts))
    assert counts[r] >= 2
    reach = float(np.abs(rows[r].toarray()).sum())
    l, u = c.l.copy(), c.u.copy()
    l[r], u[r] = reach + 1.0, reach + 2.0
    return qp_cases.Case(c.name + "_infeasible", c.P, c.q, c.A, l, u, c.settings, c.tier, 3)


def _batch_content(name):
    c = CASES[name]
    inf = _infeasible_twin(c)
    s = qp_cases.settings_of(c)
    info = R._oracle().qp_solve_info(inf.P, inf.q, inf.A, inf.l, inf.u, s)[2]
    assert info["status"] == 3, info
    return c, inf, s


def test_batch_isolation_tier1(alone):
    """Batch 5 of one pattern: one QP's values in slots 0, 2 and 4, an infeasible QP
    in slot 1 and a max-iter QP in slot 3.  A launch has one max_iter: 450 lets the
    repeated QP finish (275 iterations) and the infeasible one find its certificate
    (400), and stops a QP that needs 525."""
    c, inf, s = _batch_content("mixed12")
    hard = qp_cases.Case("hard", c.P, c.q * 40.0, c.A, c.l, c.u, c.settings, 1, 7)
    s.max_iter = 450
    o = R._oracle()
    oi = o.qp_solve_info(inf.P, inf.q, inf.A, inf.l, inf.u, s)[2]
    oh = o.qp_solve_info(hard.P, hard.q, hard.A, hard.l, hard.u, s)[2]
    assert (oi["status"], oi["iter"]) == (3, 400) and (oh["status"], oh["iter"]) == (7, 450)
    assert o.qp_solve_info(c.P, c.q, c.A, c.l, c.u, s)[2] == R.reruns("mixed12").info  # 450 changes nothing for it
    qp = GpuQp(c, 5)
    try:
        assert qp.tier() == 1
        out = qp.solve([c, inf, c, hard, c], s)
    finally:
        qp.close()
    one = alone("mixed12")[0]
    for k in (0, 2, 4):
        assert same_bits(out[k], one), k
    assert (out[1][2]["status"], out[1][2]["iter"]) == (3, 400)
    assert np.isnan(out[1][0]).all() and np.isnan(out[1][1]).all()
    assert (out[3][2]["status"], out[3][2]["iter"], out[3][2]["polish_status"]) == (7, 450, 0)
    assert np.isfinite(out[3][0]).all() and np.isfinite(out[3][1]).all()


@pytest.mark.parametrize("tier", [1, 2, 3])
def test_batch_isolation_per_tier(alone, tier):
    name = TIER_CASE[tier]
    c, inf, s = _batch_content(name)
    qp = GpuQp(c, 3)
    try:
        assert qp.tier() == tier
        out = qp.solve([c, inf, c], s)
    finally:
        qp.close()
    one = alone(name)[0]
    assert same_bits(out[0], one) and same_bits(out[2], one)
    assert out[1][2]["status"] == 3 and np.isnan(out[1][0]).all() and np.isnan(out[1][1]).all()


# ------------------------------------------------------------------ solve_some
def test_solve_some_with_mask_and_rho():
    """count = 3 of batch 5, warm_mask = [1, 0, 1] and warm_rho: each QP equals the
    oracle's one-shot solve with or without the warm start."""
    name = "mixed12_unpolished"
    c = CASES[name]
    s = qp_cases.settings_of(c)
    rr = R.reruns(name)
    q2 = R.Sequence("mixed12").steps[2][2].q  # the same pattern with another q
    other = qp_cases.Case("other", c.P, q2, c.A, c.l, c.u, c.settings)
    cases = [c, other, c]
    wx = [rr.x, rr.x, 0.5 * rr.x]
    wy = [rr.y, rr.y, 0.5 * rr.y]
    mask = [1, 0, 1]
    rho = [rr.info["rho"], 0.3, 0.05]
    refs = []
    for k in range(3):
        runs = []
        for variant, seed in [("exact", None), ("fast", None)] + [("exact", j) for j in R.SEEDS]:
            kw = dict(warm_rho=rho[k])
            if mask[k]:
                kw.update(warm_x=wx[k], warm_y=wy[k])
            runs.append(R.solve_oracle(cases[k], variant, seed, **kw))
        assert len({tuple(r[2][f] for f in R.DISCRETE) for r in runs}) == 1, (k, "stability rule")
        sp = {"x": max(R.err_inf(r[0], runs[0][0]) for r in runs), "y": max(R.err_inf(r[1], runs[0][1]) for r in runs)}
        for f in ("rho", "prim_res", "dual_res"):
            sp[f] = max(abs(r[2][f] - runs[0][2][f]) for r in runs)
        refs.append((runs[0], sp))
    # the three differ from one another and from the cold solve: the mask and the rho are used
    assert len({(r[0][2]["iter"], r[0][2]["rho"]) for r in refs} | {(rr.info["iter"], rr.info["rho"])}) == 4
    qp = GpuQp(c, 5)
    try:
        out = qp.solve_some(cases, s, warm_x=wx, warm_y=wy, warm_mask=mask, warm_rho=rho)
    finally:
        qp.close()
    for k in range(3):
        check_solve(f"solve_some[{k}]", cases[k], out[k], refs[k][0], refs[k][1], None)


# ------------------------------------------------------------------ submit / collect, grouped launch
def test_submit_collect_equals_synchronous(alone):
    names = ["mixed12", "odd53"]
    qps = [GpuQp(CASES[k], 1) for k in names]
    try:
        for k, qp in zip(names, qps):
            qp.submit([CASES[k]], qp_cases.settings_of(CASES[k]))
        outs = [qp.collect()[0] for qp in qps]
    finally:
        for qp in qps:
            qp.close()
    for k, o in zip(names, outs):
        assert same_bits(o, alone(k)[0]), k


def test_grouped_launch_over_three_tiers(alone):
    """stage on a tier-1, a tier-2 and a tier-3 object, one launch_staged, collect
    each: every QP is its object's own thip_qp_solve, bit for bit."""
    names = [TIER_CASE[1], TIER_CASE[2], TIER_CASE[3]]
    qps = [GpuQp(CASES[k], 2) for k in names]
    try:
        assert [qp.tier() for qp in qps] == [1, 2, 3]
        for k, qp in zip(names, qps):
            qp.submit([CASES[k], CASES[k]], qp_cases.settings_of(CASES[k]), launch=False)
        GpuQp.launch_staged(qps)
        outs = [qp.collect() for qp in qps]
    finally:
        for qp in qps:
            qp.close()
    for k, o in zip(names, outs):
        assert same_bits(o[0], alone(k)[0]) and same_bits(o[1], alone(k)[0]), k


# ------------------------------------------------------------------ resident state machine
class DeviceBackend:
    def __init__(self, case):
        self.qp = GpuQp(case, 1)

    def setup(self, c, s):
        return self.qp.setup(c, s)

    def update_vec(self, q, l, u):
        return self.qp.update_vec(q, l, u)

    def update_mat(self, Px, Ax):
        return self.qp.update_mat(Px, Ax)

    def warm_start(self, x, y):
        return self.qp.warm_start(x, y)

    def solve(self):
        return self.qp.solve_resident()

    def solve_gone(self):
        return self.qp.solve_resident_rc()


@pytest.mark.parametrize("tier", [1, 2, 3])
def test_resident_sequence(tier):
    """Sequence (tests/qp_reference.py) against oracle.QpSession, the discrete and
    numeric rules at every solve.  After the non-convex update the oracle's
    session reports status -1 / error 5; the device lost the workspace with the
    same error and refuses the solve (THIP_E_STATE: the next call must be
    thip_qp_setup), then a fresh setup matches again."""
    name = TIER_CASE[tier]
    ref = R.sequence_ref(name)
    seq = ref.seq
    for k in ref.solves:
        assert len(ref.keys[k]) == 1, (k, "stability rule", ref.keys[k])
    assert ref.exact[1][2]["rho"] != qp_cases.settings_of(seq.case).rho  # step 3 follows a solve that changed rho
    dev = DeviceBackend(seq.case)
    try:
        assert dev.qp.tier() == tier
        got = seq.run(dev)
    finally:
        dev.qp.close()
    for k, (op, _, data) in enumerate(seq.steps):
        label = f"{name} step {k} {op}"
        if op == "solve":
            polished = ref.exact[k][2]["polish_status"] == 1
            check_solve(label, data, got[k], ref.exact[k], ref.spread[k], ref.star(k) if polished else None)
        elif op == "solve_gone":
            assert ref.exact[k][2]["status"] == -1 and ref.exact[k][2]["setup_error"] == 5
            assert got[k][0] == E_STATE, got[k]
        else:
            assert got[k] == ref.exact[k] == seq.expect_err.get(k, 0), (label, got[k], ref.exact[k])
