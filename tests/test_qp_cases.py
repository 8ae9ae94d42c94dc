"""The catalogue of tests/qp_cases.py proved on the CPU oracle, before the device
is measured against it (tests/test_gpu_qp_direct.py).

Stability rule -- a condition on the catalogue, not a tolerance: every case
returns the same (status, setup_error, iterations, polish status, rho
updates) from the exact build, the fast build and 8 seeds of a 1e-12 relative
jitter on every KKT solution.  A case that fails it is replaced, never
excused: the device tests have no "oracle is unstable" escape.

High-precision reference: for every solved and polished case the active set is
read from the oracle's y and the equality-constrained KKT system is solved by
iterative refinement with long-double residuals (x*, y*).  The oracle's
polished (x, y) must lie within cond_1(K_active) 2^-53 |(x*, y*)|_inf of it,
the forward-error bound of a backward-stable solve of the reduced KKT system
in double.  An unpolished y carries no clean active set, so the unpolished
solved cases are held to OSQP's own termination guarantee alone, recomputed in
long double from (x, y) -- as every status-1 case is.

Sessions: oracle.QpSession sequences equal fresh one-shot solves wherever OSQP
makes them the same computation.
"""
import numpy as np
import pytest

import qp_cases
import qp_reference as R
from qp_cases import CASES

POLISHED = [k for k in qp_cases.SOLVED if CASES[k].polish_status == 1]
VARIANTS = [k for k in CASES if k.startswith("mixed12_") and k not in ("mixed12_unpolished",)]


@pytest.fixture(scope="module", autouse=True)
def _built(oracle_mod):
    return oracle_mod


@pytest.mark.parametrize("name", list(CASES))
def test_status_and_stability_rule(name):
    c = CASES[name]
    rr = R.reruns(name)
    assert len(rr.keys) == 1, f"{name} breaks the stability rule: {sorted(rr.keys)}"
    assert (rr.info["status"], rr.info["setup_error"]) == (c.status, c.setup_error)
    if c.status in (3, 5):
        assert all(np.isnan(x).all() and np.isnan(y).all() for x, y, _ in rr.runs)
    if c.status == 7:
        assert rr.info["iter"] == c.settings["max_iter"]
    assert rr.info["polish_status"] == c.polish_status


def test_settings_variants_take_their_branch():
    """Every settings variant of the n = 12 case changes the run: another number
    of iterations or of rho updates than the defaults (a variant that solves the
    same way would test nothing)."""
    base = R.reruns("mixed12").info
    assert base["rho_updates"] >= 1 and base["rho"] != 0.1
    seen = {(base["iter"], base["rho_updates"])}
    for name in VARIANTS:
        i = R.reruns(name).info
        key = (i["iter"], i["rho_updates"])
        assert key not in seen, (name, key)
        seen.add(key)
    assert R.reruns("mixed12_no_adaptive_rho").info["rho_updates"] == 0
    # 30 is no multiple of check_termination = 25: rho adapts between two checks
    assert R.reruns("mixed12_rho_interval30").info["rho_updates"] >= 1
    assert R.reruns("mixed12_check0").info["iter"] == CASES["mixed12_check0"].settings["max_iter"]


def test_the_tier3_solve_adapts_rho():
    # the HBM solve vector also goes through a refactorisation in the loop
    assert R.reruns("tier3").info["rho_updates"] >= 1


@pytest.mark.parametrize("name", POLISHED)
def test_polished_solution_against_long_double_kkt(name):
    rr, st = R.reruns(name), R.kkt_star(name)
    assert st.residual <= 64 * np.finfo(np.longdouble).eps * max(1.0, st.scale) * max(1.0, st.cond)
    ex, ey = R.err_inf(rr.x, st.x), R.err_inf(rr.y, st.y)
    print(f"{name}: |x - x*| {ex:.2e} |y - y*| {ey:.2e} bound {st.forward:.2e} cond {st.cond:.2e}")
    assert ex <= st.forward and ey <= st.forward
    # the active set read from y is complementary: inactive rows hold strictly inside their bounds
    c = CASES[name]
    if c.m:
        Ax = c.A @ np.asarray(st.x, dtype=np.float64)
        tol = st.forward + 1e-12
        assert (Ax >= c.l - tol).all() and (Ax <= c.u + tol).all()


@pytest.mark.parametrize("name", qp_cases.SOLVED)
def test_termination_guarantee_in_long_double(name):
    rr = R.reruns(name)
    for x, y, _ in rr.runs:
        prim, ptol, dual, dtol = R.termination_gaps(CASES[name], x, y)
        assert prim <= ptol and dual <= dtol, (name, prim, ptol, dual, dtol)


def _same(a, b):
    (xa, ya, ia), (xb, yb, ib) = a, b
    return np.array_equal(xa, xb, equal_nan=True) and np.array_equal(ya, yb, equal_nan=True) and ia == ib


@pytest.mark.parametrize("variant", ["exact", "fast"])
@pytest.mark.parametrize("name", ["n1m1", "n5m0", "mixed12", "lp", "tier2", "primal_infeasible", "max_iter"])
def test_session_cold_setup_and_solve_is_the_one_shot_solve(oracle_mod, name, variant):
    c = CASES[name]
    s = qp_cases.settings_of(c)
    one = oracle_mod.qp_solve_info(c.P, c.q, c.A, c.l, c.u, s, variant=variant)
    ses = oracle_mod.QpSession(variant)
    assert ses.setup(c.P, c.q, c.A, c.l, c.u, s) == 0
    assert _same(ses.solve(), one)
    # a fresh setup drops every kept iterate
    assert ses.setup(c.P, c.q, c.A, c.l, c.u, s) == 0
    assert _same(ses.solve(), one)
    ses.close()


def test_session_setup_errors(oracle_mod):
    for name in ("non_convex", "l_above_u"):
        c = CASES[name]
        s = qp_cases.settings_of(c)
        ses = oracle_mod.QpSession()
        assert ses.setup(c.P, c.q, c.A, c.l, c.u, s) == c.setup_error
        _, _, info = ses.solve()
        assert (info["status"], info["setup_error"]) == (-1, c.setup_error)
        assert ses.update_vec(q=c.q) == -1 and ses.warm_start(x=np.zeros(c.n)) == -1


def test_warm_start_maps_as_osqp_model_does(oracle_mod):
    """qp_solve_info's warm x, y, rho are rho into the settings before osqp_setup,
    then osqp_warm_start: the same session calls give the same bits, and a warm
    start from the solution ends at the first check."""
    c = CASES["mixed12_unpolished"]
    x0, y0, i0 = R.reruns("mixed12_unpolished").runs[0]
    s = qp_cases.settings_of(c)
    warm = oracle_mod.qp_solve_info(c.P, c.q, c.A, c.l, c.u, s, warm_x=x0, warm_y=y0, warm_rho=i0["rho"])
    assert warm[2]["status"] == 1 and warm[2]["iter"] == 25 < i0["iter"]
    ses = oracle_mod.QpSession()
    assert ses.setup(c.P, c.q, c.A, c.l, c.u, qp_cases.settings_of(c, rho=i0["rho"])) == 0
    assert ses.warm_start(x0, y0) == 0
    assert _same(ses.solve(), warm)
    # rho alone: a cold start at another rho
    cold = oracle_mod.qp_solve_info(c.P, c.q, c.A, c.l, c.u, s, warm_rho=i0["rho"])
    assert (cold[2]["iter"], cold[2]["rho_updates"]) != (i0["iter"], i0["rho_updates"])
    assert ses.setup(c.P, c.q, c.A, c.l, c.u, qp_cases.settings_of(c, rho=i0["rho"])) == 0
    assert _same(ses.solve(), cold)


def test_session_rejected_update_leaves_the_solver_alone(oracle_mod):
    c = CASES["mixed12"]
    s = qp_cases.settings_of(c)
    q2 = c.q * 0.9
    a, b = oracle_mod.QpSession(), oracle_mod.QpSession()
    for ses in (a, b):
        assert ses.setup(c.P, c.q, c.A, c.l, c.u, s) == 0
        ses.solve()
    bad_u = c.u.copy()
    bad_u[6] = c.l[6] - 1.0 if c.l[6] > -1e29 else -1e31
    assert a.update_vec(l=c.l, u=bad_u) == 1
    assert a.update_vec(q=q2) == 0 and b.update_vec(q=q2) == 0
    assert _same(a.solve(), b.solve())
    # a non-convex P loses the solver object; a fresh setup brings it back
    Pbad = c.P.data.copy()
    Pbad[c.P.indptr[1:] - 1] = -1e6
    assert a.update_mat(Px=Pbad) == 5
    assert a.solve()[2]["status"] == -1 and a.solve()[2]["setup_error"] == 5
    assert a.setup(c.P, c.q, c.A, c.l, c.u, s) == 0
    assert _same(a.solve(), R.reruns("mixed12").runs[0])
