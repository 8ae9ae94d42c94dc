"""The CartPose error and its forward-difference Jacobian at the rotation logarithm's
edges on every device entry (MI355X).

kin_device.hpp's rot_error (Shoemake's four quaternion branches, Eigen's AngleAxis
conversion, tesseract's sign fix, the wrap into [-pi, pi] or [0, 2 pi]), transform_error,
apply_tolerances and transform_error_diff_tol's wrap switch are reached through four
device code paths, and the arm workloads of the other GPU tests only ever show them an
error rotation of a fraction of a radian in general position: the trace branch, w > 0.
Here the chains of tests/pose_cases.py put one case per problem of a batch (E = I and
angles down to 1e-200, every branch with both signs of w, exactly pi, revolute joints
beyond pi, a target 10 m away, band edges to the ulp, FD steps across the wrap at pi and
across the seam of the [0, 2 pi] form at 120 degrees), and every entry runs every batch
against tests/pose_reference.py (long double, its own logarithm) under tests/test_gpu.py's
bars: error 1e-12, Jacobian 1e-9, a term's value 6 max(w) 1e-12, all absolute.  The error
for E = I is exactly 0, the pi convention holds bit for bit, a component on a band's edge
gives exactly 0.  tests/test_pose_reference.py validates the table and the oracle on the CPU.

  thip_linearize                  linearize() of sqp_kernel.hip: error and Jacobian
  thip_eval_cart_pose / _all      cart_eval_one of term_eval.hip: error and Jacobian, and
                                  the two entries' bytes equal
  thip_terms_run                  term_values.hip's CartPose block: each batch as a cost
                                  (sum |err_i| w_i) and as a constraint (sum |err_i w_i|)
  thip_sqp_run                    the fused kernel's own value pass (A_COST, the merit's
                                  input): a few iterations from the wrap family's start, the
                                  solver's value of the term against the reference at the
                                  returned trajectory

Worst gaps, device against reference, 191 cases, MI355X (each test prints its own; the
oracle's, on the CPU, in tests/test_pose_reference.py):
  entry                                     error      jacobian   value
  thip_linearize                            2.2e-15    1.4e-10    -
  thip_eval_cart_pose = _all (same bytes)   2.2e-15    1.4e-10    -
  thip_terms_run, cost / constraint         -          -          6.3e-15 / 6.5e-15
  fused value pass (A_COST)                 -          -          2.7e-15
  oracle on the CPU                         2.0e-15    3.1e-10    -
No device code changed: the module found no bug.
"""
import ctypes as C

import numpy as np
import pytest

import pose_cases as pc
import pose_reference as pr
from trajopt_amd import abi
from trajopt_amd.runtime import BatchTrustRegionSQP, TermEvaluator, TermValues

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    dp = C.POINTER(C.c_double)
    lib.thip_eval_cart_pose_all.argtypes = [C.c_void_p, dp, dp, dp]
    lib.thip_eval_cart_pose_all.restype = C.c_int
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


_WL = {}


def workload(batch, is_cnt=False):
    key = (batch[0], is_cnt)
    if key not in _WL:
        _WL[key] = pc.make_workload(batch, is_cnt)
    return _WL[key]


# ------------------------------------------------------------------ thip_linearize
@pytest.mark.parametrize("batch", pc.BATCHES, ids=pc.BATCH_IDS)
def test_fused_linearize(batch):
    wl = workload(batch)
    s = BatchTrustRegionSQP(wl)
    try:
        err, jac = s.linearize(wl.init)
    finally:
        s.close()
    worst = pc.check(batch, err[:, 0], jac[:, 0], f"linearize/{batch[0]}")
    print(f"thip_linearize {batch[0]}: worst vs reference: error {worst[0]:.3e} jacobian {worst[1]:.3e}")


# ------------------------------------------------------------------ thip_eval_cart_pose / _all
@pytest.mark.parametrize("batch", pc.BATCHES, ids=pc.BATCH_IDS)
def test_eval_cart_pose(hip, batch):
    wl = workload(batch)
    B, D = wl.batch, wl.n_dof
    ev = TermEvaluator(wl)
    try:
        err, jac = ev.cart_pose(0, wl.init[:, 0])
        err_only, _ = ev.cart_pose(0, wl.init[:, 0], jac=False)
        x = np.ascontiguousarray(wl.init, dtype=np.float64)
        err_all, jac_all = np.zeros((B, 1, 6)), np.zeros((B, 1, 6, D))
        assert hip.thip_eval_cart_pose_all(ev.ev, _dp(x), _dp(err_all), _dp(jac_all)) == 0
    finally:
        ev.close()
    worst = pc.check(batch, err, jac, f"eval/{batch[0]}")
    print(f"thip_eval_cart_pose {batch[0]}: worst vs reference: error {worst[0]:.3e} jacobian {worst[1]:.3e}")
    assert err_all.tobytes() == err.tobytes() and jac_all.tobytes() == jac.tobytes(), "the two entries differ"
    assert err_only.tobytes() == err.tobytes()


# ------------------------------------------------------------------ thip_terms_run
def _value_gap(batch, is_cnt, got):
    """|value - reference| per problem (a value is a sum of |err_i|: it does not see the sign
    that a `*_pi_inexact` case leaves open)."""
    return np.abs(got.astype(pr.LD) - pc.ref_values(batch, is_cnt)).astype(np.float64)


@pytest.mark.parametrize("is_cnt", [False, True], ids=["cost", "constraint"])
@pytest.mark.parametrize("batch", pc.BATCHES, ids=pc.BATCH_IDS)
def test_term_values(batch, is_cnt):
    wl = workload(batch, is_cnt)
    tv = TermValues(wl)
    try:
        cart = [i for i, s in enumerate(tv.slots) if s.kind == abi.TERM_CART]
        assert len(cart) == 1 and bool(tv.slots[cart[0]].is_cnt) == is_cnt
        costs, viols = tv.run(wl.init)
        nc = tv.n_costs
    finally:
        tv.close()
    got = viols[:, cart[0] - nc] if is_cnt else costs[:, cart[0]]
    assert np.all(np.isfinite(got))
    gap = _value_gap(batch, is_cnt, got)
    print(f"thip_terms_run {batch[0]} {'constraint' if is_cnt else 'cost'}: worst vs reference {gap.max():.3e}")
    bad = [(c["name"], g) for c, g in zip(batch[4], gap) if g > pc.TOL_VALUE]
    assert not bad, bad


# ------------------------------------------------------------------ the fused kernel's value pass
@pytest.mark.parametrize("batch", [b for b in pc.BATCHES if b[0] in ("posebot-wide-ident", "posebot-none-ident-2")],
                         ids=lambda b: b[0])
def test_fused_value_pass(hip, batch):
    """A few SQP iterations from the batch's start (both hold the wrap family; the
    untoleranced one the joints beyond pi and the seam as well): the solver's own value of
    the CartPose cost (A_COST, evaluated by sqp_kernel.hip's value pass at the trajectory
    it returns; under THIP_DEBUG_STATIC_DISPATCH problem b keeps workspace b) against the
    reference at the downloaded trajectory, and the result's total_cost as their sum."""
    wl = pc.make_workload(batch)
    wl.desc.sqp.max_iter = 4
    assert hip.thip_debug_set_path(abi.DEBUG_STATIC_DISPATCH) == 0
    try:
        s = BatchTrustRegionSQP(wl, device=0)
    finally:
        hip.thip_debug_set_path(0)
    try:
        x, res = s.optimize()
        dws, _, doff, _ = s.debug_values()
    finally:
        s.close()
    tv = TermValues(wl)
    try:
        slots, nc = tv.slots, tv.n_costs
    finally:
        tv.close()
    cart = [i for i, sl in enumerate(slots) if sl.kind == abi.TERM_CART]
    assert len(cart) == 1 and cart[0] < nc and all(r.n_costs == nc for r in res)
    a_cost = dws[:, doff[abi.WS_A_COST]: doff[abi.WS_A_COST] + nc]
    assert np.isfinite(x).all() and np.abs(x - wl.init).max() > 1e-6, "the solve did not move"
    _, chain, band, offset, cases = batch
    want = []
    for b, c in enumerate(cases):
        E = pr.error_pose(pc.CHAINS[chain], x[b, 0], pc.TOOL, pc.OFFSETS[offset], pc.target_link(chain), c["target"])
        want.append(pr.value(pr.error(E, pc.BANDS[band]), pc.WEIGHTS, False))
    gap = np.abs(a_cost[:, cart[0]].astype(pr.LD) - np.array(want)).astype(np.float64)
    print(f"fused value pass {batch[0]}: worst vs reference {gap.max():.3e} (values up to {float(max(want)):.4g})")
    bad = [(c["name"], g) for c, g in zip(cases, gap) if g > pc.TOL_VALUE]
    assert not bad, bad
    for b, r in enumerate(res):
        assert abs(r.total_cost - a_cost[b].sum()) <= 1e-12 * max(1.0, abs(r.total_cost))
