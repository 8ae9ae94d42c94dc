"""thost_tsqp_solve_batch at the front door, without a GPU: the FFI layout of
tsqp_batch_stats, the refusals that come before any device call with their
messages, and a refused set's error reported for its problem."""
import ctypes as C

import numpy as np
import pytest

from trajopt_amd import abi, host, tsqp

D = 7


@pytest.fixture(scope="module")
def built():
    if not host.HOST_LIB.exists():
        import __graft_entry__

        __graft_entry__.build()
    tsqp._lib()
    return host.load_host()


def _call(L, specs, kins, batch, x, results, rounds=None, stats=None):
    err = C.create_string_buffer(4096)
    rc = L.thost_tsqp_solve_batch(specs, kins, batch, 0, x, results, rounds, stats, err, 4096)
    return rc, err.value.decode()


def test_batch_stats_layout(built):
    assert built.thost_tsqp_sizeof_batch_stats() == C.sizeof(tsqp.BatchStats) == 6 * 8
    # the structs the batch call shares with the single calls did not move
    assert built.thost_tsqp_sizeof_spec() == C.sizeof(tsqp.Spec)
    assert built.thost_tsqp_sizeof_result() == C.sizeof(tsqp.Result)
    assert abi.ABI_VERSION == 10


def test_step_prototype_and_op_bits(built):
    lib = abi.load_hip()
    assert lib.thip_qp_step.restype is C.c_int and len(lib.thip_qp_step.argtypes) == 13
    assert (abi.QP_OP_SETUP, abi.QP_OP_MAT_P, abi.QP_OP_VEC_Q, abi.QP_OP_MAT_A, abi.QP_OP_VEC_BOUNDS, abi.QP_OP_WARM,
            abi.QP_OP_SOLVE) == (1, 2, 4, 8, 16, 32, 64)
    assert "thip_qp_step" in abi.exported_symbols()
    # a null handle is refused before anything else
    assert lib.thip_qp_step(None, None, None, None, None, None, None, None, None, None, None, None, None) == abi.E_INVALID


def test_refusals_before_any_device_call(built):
    spec = tsqp.make_spec(np.zeros((2, D)), [])
    specs = (tsqp.Spec * 1)(spec)
    x = np.zeros(tsqp.MAX_NODES * tsqp.D_MAX)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    res = (tsqp.Result * 1)()
    for batch in (0, -3):
        rc, msg = _call(built, specs, None, batch, xp, res)
        assert rc != 0 and "batch must be at least 1" in msg, msg
    for args in ((None, None, 1, xp, res), (specs, None, 1, None, res), (specs, None, 1, xp, None)):
        rc, msg = _call(built, *args)
        assert rc != 0 and "null argument" in msg, msg
    with pytest.raises(host.HostError, match="batch must be at least 1"):
        tsqp.solve_batch([])
    with pytest.raises(ValueError):
        tsqp.solve_batch([spec], kins=[])


def test_refused_set_reports_its_problem(built):
    """use_numeric_differentiation = false is refused when the problem first updates the set, before any device call:
    the batch reports it under the problem's number."""
    spec = tsqp.make_spec(np.zeros((1, D)), [])
    kin = tsqp.make_kin_spec("right_arm", cart=[dict(source_frame="r_gripper_tool_frame", target_frame="base_footprint",
                                                     analytic_jacobian=True)])
    with pytest.raises(host.HostError) as e:
        tsqp.solve_batch([spec], [kin])
    assert "problem 0: " in str(e.value) and "use_numeric_differentiation = false" in str(e.value), str(e.value)
    # a spec that cannot be built is reported the same way
    bad = tsqp.make_spec(np.zeros((1, D)), [])
    bad.n_nodes = 0
    with pytest.raises(host.HostError) as e:
        tsqp.solve_batch([bad])
    assert "problem 0: " in str(e.value) and "spec out of range" in str(e.value), str(e.value)
