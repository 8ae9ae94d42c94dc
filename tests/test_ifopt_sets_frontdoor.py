"""The trajopt_ifopt kinematic sets (CartPosConstraint, the fixed-size
DiscreteCollisionConstraint over SingleTimestepCollisionEvaluator) and the
collision-set C-ABI (thip_csets_*) at the front door, without a GPU: FFI
layouts, the refusals with their messages, the RangeBoundHandling rows and
bounds, and thip_csets_create's validation, which returns before any device
call."""
import ctypes as C
import math

import numpy as np
import pytest

from trajopt_amd import abi, host, problems, tsqp

D = 7
TOOL, ROOT = "r_gripper_tool_frame", "base_footprint"


@pytest.fixture(scope="module")
def built():
    if not host.HOST_LIB.exists():
        import __graft_entry__

        __graft_entry__.build()
    return host.load_host()


def _spec(n_nodes=1, d=D):
    return tsqp.make_spec(np.zeros((n_nodes, d)), [])


def _no_x(spec):
    return np.zeros((0, spec.n_nodes, spec.n_dof))


# ------------------------------------------------------------------ layouts
def test_ffi_struct_sizes(built):
    lib = abi.load_hip()
    assert lib.thip_sizeof_csets_config() == C.sizeof(abi.CsetsConfig) == 40
    assert abi.CSETS_MAX_ROWS == 64
    cfg = abi.CsetsConfig()
    lib.thip_default_csets_config(C.byref(cfg))
    assert (cfg.margin, cfg.coeff, cfg.margin_buffer, cfg.max_num_cnt, cfg.first_step, cfg.last_step) == (0, 1, 0, 1, 0, 0)
    assert built.thost_tsqp_sizeof_kin_spec() == C.sizeof(tsqp.KinSpec)
    assert built.thost_tsqp_sizeof_cart_term() == C.sizeof(tsqp.CartTerm)
    assert built.thost_tsqp_sizeof_coll_term() == C.sizeof(tsqp.CollTerm) == 44 + 4
    # the joint front end's structs did not move
    assert built.thost_tsqp_sizeof_spec() == C.sizeof(tsqp.Spec)
    assert lib.thip_sizeof_desc() == C.sizeof(abi.ProblemDesc) and abi.ABI_VERSION == 10


# ------------------------------------------------------------------ CartPos refusals
CART_REFUSALS = [
    ("missing_source", dict(source_frame="r_gripper", target_frame=ROOT), "Source Link name 'r_gripper' provided does not exist."),
    ("missing_target", dict(source_frame=TOOL, target_frame="table"), "Target Link name 'table' provided does not exist."),
    ("two_static_frames", dict(source_frame="base_link", target_frame=ROOT),
     "CartPosInfo: Target and Source are both static links."),
    ("both_active", dict(source_frame=TOOL, target_frame="r_elbow_flex_link"), "kBothActive"),
]


@pytest.mark.parametrize("name, frames, needle", CART_REFUSALS, ids=[r[0] for r in CART_REFUSALS])
def test_cartpos_constructor_refusals(built, name, frames, needle):
    spec = _spec()
    with pytest.raises(host.HostError) as e:
        tsqp.eval_kin(spec, tsqp.make_kin_spec("right_arm", cart=[dict(node=0, **frames)]), _no_x(spec))
    assert needle in str(e.value), str(e.value)


def test_both_active_says_why(built):
    spec = _spec()
    with pytest.raises(host.HostError) as e:
        tsqp.eval_kin(spec, tsqp.make_kin_spec("right_arm", cart=[dict(source_frame=TOOL, target_frame="r_forearm_link")]),
                      _no_x(spec))
    msg = str(e.value)
    assert "both active" in msg and "not supported on the HIP path" in msg, msg


def test_analytic_jacobian_is_refused_and_names_the_flag(built):
    """use_numeric_differentiation = false: refused when the problem first updates
    the set, before any device call."""
    spec = _spec()
    kin = tsqp.make_kin_spec("right_arm", cart=[dict(source_frame=TOOL, target_frame=ROOT, analytic_jacobian=True)])
    with pytest.raises(host.HostError) as e:
        tsqp.eval_kin(spec, kin, np.zeros((1, 1, D)))
    assert "use_numeric_differentiation = false" in str(e.value), str(e.value)


def test_kin_spec_refusals(built):
    spec = _spec(n_nodes=2)
    ok = dict(source_frame=TOOL, target_frame=ROOT)
    for kin, needle in [
        (tsqp.make_kin_spec("right_arm", cart=[dict(node=2, **ok)]), "node out of range"),
        (tsqp.make_kin_spec("left_arm", cart=[dict(node=0, **ok)]), "Source Link name"),
        (tsqp.make_kin_spec("manipulator"), "2 joints"),
        (tsqp.make_kin_spec("right_arm", coll=[dict(first=1, last=0, margin=0.1)]), "nodes out of range"),
        (tsqp.make_kin_spec("right_arm", coll=[dict(first=0, margin=0.1, max_num_cnt=0)]),
         "max_num_cnt must be greater than zero!"),
        (tsqp.make_kin_spec("right_arm", coll=[dict(first=0, margin=0.1, max_num_cnt=65)]), "64 rows per node"),
        (tsqp.make_kin_spec("right_arm", cart=[dict(node=0, penalty=7, **ok)]), "unknown penalty type"),
    ]:
        with pytest.raises(host.HostError) as e:
            tsqp.eval_kin(spec, kin, _no_x(spec))
        assert needle in str(e.value), str(e.value)


# ------------------------------------------------------------------ RangeBoundHandling
def test_range_bounds_split_and_zero_coefficients_drop(built):
    """Mixed coefficient vector: component 2 has a zero coefficient (no row),
    component 1 a range bound (two inequality rows), component 4 a lower bound."""
    inf = math.inf
    spec = _spec(n_nodes=2)
    cart = dict(node=1, source_frame=TOOL, target_frame=ROOT, coeffs=[1, 5, 0, 2, 2, 2],
                lower=[0, -0.1, -9, 0, 0.25, 0], upper=[0, 0.2, 9, 0, inf, 0])
    coll = dict(first=0, last=1, margin=0.1, max_num_cnt=3)
    r = tsqp.eval_kin(spec, tsqp.make_kin_spec("right_arm", cart=[cart, dict(node=0, source_frame=TOOL, target_frame=ROOT)],
                                               coll=[coll]), _no_x(spec))
    assert r["launches"] == (0, 0)
    assert list(r["set_rows"]) == [6, 6, 3, 3]  # 5 components, one split; the default set; a set per node
    assert list(r["lower"][:6]) == [0, -0.1, -inf, 0, 0.25, 0]
    assert list(r["upper"][:6]) == [0, inf, 0.2, 0, inf, 0]
    # the default constructor: ones and BoundZero
    assert not r["lower"][6:12].any() and not r["upper"][6:12].any()
    # BoundSmallerZero on every collision row
    assert np.all(np.isneginf(r["lower"][12:])) and not r["upper"][12:].any()


def test_too_small_caps_are_an_error(built):
    spec = _spec()
    kin = tsqp.make_kin_spec("right_arm", cart=[dict(source_frame=TOOL, target_frame=ROOT)])
    with pytest.raises(host.HostError, match="cap_rows"):
        tsqp.eval_kin(spec, kin, _no_x(spec), cap_rows=5)


# ------------------------------------------------------------------ thip_csets_create
def _create(desc, cfg, batch=1):
    lib = abi.load_hip()
    cs = C.c_void_p()
    rc = lib.thip_csets_create(0, C.byref(desc), C.byref(cfg), batch, C.byref(cs))
    msg = lib.thip_csets_last_error(None).decode()
    if cs.value:  # a device is present and the arguments were accepted
        lib.thip_csets_destroy(cs)
    return rc, msg


def _desc(n_steps=3):
    return abi.ProblemDesc.from_buffer_copy(problems.make_workload("C", 1, n_steps=n_steps).desc)


I32 = 2 ** 31 - 1
CSETS_REFUSALS = [
    ("max_num_cnt_zero", abi.CsetsConfig(0.1, 1.0, 0.01, 0, 0, 2), "max_num_cnt 0 out of range [1, 64]"),
    ("max_num_cnt_65", abi.CsetsConfig(0.1, 1.0, 0.01, 65, 0, 2), "max_num_cnt 65 out of range"),
    ("max_num_cnt_min", abi.CsetsConfig(0.1, 1.0, 0.01, -I32 - 1, 0, 2), "out of range"),
    ("first_negative", abi.CsetsConfig(0.1, 1.0, 0.01, 3, -1, 2), "step range [-1, 2] outside [0, 2]"),
    ("last_past_the_end", abi.CsetsConfig(0.1, 1.0, 0.01, 3, 0, 3), "step range [0, 3] outside [0, 2]"),
    ("last_int_max", abi.CsetsConfig(0.1, 1.0, 0.01, 3, 0, I32), "outside [0, 2]"),
    ("first_int_min", abi.CsetsConfig(0.1, 1.0, 0.01, 3, -I32 - 1, I32), "outside [0, 2]"),
    ("inverted", abi.CsetsConfig(0.1, 1.0, 0.01, 3, 2, 1), "inverted step range [2, 1]"),
    ("margin_nan", abi.CsetsConfig(math.nan, 1.0, 0.01, 3, 0, 2), "margin is not finite"),
    ("margin_inf", abi.CsetsConfig(math.inf, 1.0, 0.01, 3, 0, 2), "margin is not finite"),
    ("coeff_nan", abi.CsetsConfig(0.1, math.nan, 0.01, 3, 0, 2), "coeff is not finite"),
    ("buffer_inf", abi.CsetsConfig(0.1, 1.0, -math.inf, 3, 0, 2), "margin_buffer is not finite"),
]


@pytest.mark.parametrize("name, cfg, needle", CSETS_REFUSALS, ids=[r[0] for r in CSETS_REFUSALS])
def test_csets_create_refuses_the_config(built, name, cfg, needle):
    rc, msg = _create(_desc(), cfg)
    assert rc == -1, (rc, msg)  # THIP_E_INVALID: no device call was made
    assert msg.startswith("thip_csets_create: ") and needle in msg, msg


def test_csets_create_refuses_the_descriptor(built):
    good = abi.CsetsConfig(0.1, 1.0, 0.01, 3, 0, 2)
    d = _desc()
    d.n_spheres = 0
    rc, msg = _create(d, good)
    assert rc == -1 and "no robot spheres" in msg and "sphere model" in msg, msg
    d = _desc()
    d.abi_version = 9
    assert _create(d, good) == (-1, "thip_csets_create: descriptor abi_version 9 != THIP_ABI_VERSION 10")
    d = _desc()
    d.sphere_link[3] = 40
    assert "bad sphere link of robot sphere 3" in _create(d, good)[1]
    d = _desc()
    d.sphere_radius[2] = math.nan
    assert "bad sphere radius of robot sphere 2" in _create(d, good)[1]
    d = _desc()
    d.n_steps = abi.ProblemDesc().n_steps  # 0
    assert "n_steps out of range" in _create(d, good)[1]
    d = _desc()
    d.n_prims = 1025
    assert "n_prims out of range" in _create(d, good)[1]
    d = _desc()
    problems.add_coll_pair(d, 2, 10, 0.1, 1.0)  # primitive 10 of 10
    assert "coll_pairs[0].other out of range" in _create(d, good)[1]
    d = _desc()
    problems.add_coll_pair(d, 2, -I32 - 1, 0.1, 1.0)
    assert "coll_pairs[0].other out of range" in _create(d, good)[1]
    d = _desc()
    problems.add_coll_pair(d, 2, 3, math.inf, 1.0)
    assert "margin / coeff must be finite" in _create(d, good)[1]
    # a self link pair listed twice, in the same or the other order: the selection's keys would repeat
    d = _desc()
    assert d.n_self_pairs >= 2
    d.self_pair[1][0], d.self_pair[1][1] = d.self_pair[0][0], d.self_pair[0][1]
    rc, msg = _create(d, good)
    assert rc == -1 and "self_pair[1] repeats self_pair[0]" in msg, (rc, msg)
    d = _desc()
    n = d.n_self_pairs
    d.self_pair[n][0], d.self_pair[n][1] = d.self_pair[0][1], d.self_pair[0][0]
    d.n_self_pairs = n + 1
    rc, msg = _create(d, good)
    assert rc == -1 and "self_pair[%d] repeats self_pair[0]" % n in msg, (rc, msg)
    # another term's entry is not read: the refusal is the one that comes after the override checks
    d = _desc()
    problems.add_coll_pair(d, 99, 99, math.nan, 1.0, term=2)
    d.self_pair[1][0], d.self_pair[1][1] = d.self_pair[0][0], d.self_pair[0][1]
    rc, msg = _create(d, good)
    assert rc == -1 and "repeats self_pair[0]" in msg, (rc, msg)
    assert _create(_desc(), good, batch=0)[1] == "thip_csets_create: null argument or batch <= 0"


def test_collision_sets_wrapper_reports_the_create_error(built):
    from trajopt_amd.runtime import CollisionSets, HipError

    d = _desc()
    with pytest.raises(HipError, match="inverted step range"):
        CollisionSets(d, 1, np.zeros((1, 10, 16)), abi.CsetsConfig(0.1, 1.0, 0.01, 3, 1, 0))
