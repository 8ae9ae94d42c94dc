"""The cart_vel term (trajopt::CartVelTermInfo) at the front door, without a GPU:
fromJson's checks, the lowered cvel table, the path such a problem takes, and the
C-ABI's refusals before any device call."""
import ctypes as C
import json

import pytest

from trajopt_amd import abi, host
from trajopt_amd.robots import PR2_TOOL_LINK

N, D = 8, 7


@pytest.fixture(scope="module")
def built():
    if not host.HOST_LIB.exists():
        import __graft_entry__

        __graft_entry__.build()
    return host.load_host()


def _term(link="r_gripper_tool_frame", first=1, last=4, disp=0.05, **extra):
    t = {"type": "cart_vel", "params": {"link": link, "first_step": first, "last_step": last,
                                        "max_displacement": disp}}
    t.update(extra)
    return t


def _doc(costs=(), cnts=(), **basic):
    bi = {"n_steps": N, "manip": "right_arm", "fixed_timesteps": [0]}
    bi.update(basic)
    return {
        "basic_info": bi,
        "costs": [{"type": "joint_vel", "params": {"coeffs": [1.0] * D, "targets": [0.0] * D}}] + list(costs),
        "constraints": list(cnts),
        "init_info": {"type": "stationary"},
    }


def _text(**kw):
    return json.dumps(_doc(**kw))


TWO_TERMS = dict(cnts=[_term()], costs=[_term(link="r_forearm_link", first=0, last=6, disp=0.125, name="slow_forearm")])


def test_lowering_fills_the_cvel_table(built):
    desc = host.lower_json(_text(**TWO_TERMS))[0]
    assert desc.abi_version == 10 == abi.ABI_VERSION
    assert desc.n_cvel == 2
    # costs hatch before constraints
    assert [desc.cvel_is_cnt[k] for k in range(2)] == [0, 1]
    assert [desc.cvel_link[k] for k in range(2)] == [7, PR2_TOOL_LINK]
    assert [desc.cvel_first_step[k] for k in range(2)] == [0, 1]
    assert [desc.cvel_last_step[k] for k in range(2)] == [6, 4]
    assert [desc.cvel_max_disp[k] for k in range(2)] == [0.125, 0.05]
    # nothing else moved: the JointVel cost is still the jv_* term
    assert desc.jv_enabled == 1 and desc.n_cart == 0 and desc.n_jdt == 0


def test_problem_is_not_lowerable_and_names_the_term(built):
    with pytest.raises(host.HostError) as e:
        host.eval_json_batch([_text(**TWO_TERMS)], None, None, route=host.EVAL_NAMES)
    msg = str(e.value)
    assert "do not take this problem" in msg and "cart_vel" in msg, msg
    # unloweredTerms(): the cost by its name, the constraints by the reference's "CartVel"
    assert "'slow_forearm'" in msg and "'CartVel'" in msg, msg


def _drop(doc_term, key):
    t = json.loads(json.dumps(doc_term))
    del t[key]
    return t


def _with_param(doc_term, key, value):
    t = json.loads(json.dumps(doc_term))
    t["params"][key] = value
    return t


REFUSALS = [
    ("missing_params", dict(cnts=[_drop(_term(), "params")]), "CartVelTermInfo: missing params"),
    ("unknown_member", dict(cnts=[_with_param(_term(), "coeffs", [1.0])]), "invalid field found: coeffs"),
    ("inactive_link", dict(cnts=[_term(link="torso_lift_link")]), "invalid link name: torso_lift_link"),
    ("unknown_link", dict(cnts=[_term(link="r_elbow")]), "invalid link name: r_elbow"),
    ("first_not_below_last", dict(cnts=[_term(first=4, last=4)]), "first_step 4, last_step 4"),
    ("first_above_last", dict(costs=[_term(first=5, last=2)]), "first_step 5, last_step 2"),
    # the decided deviation: the reference accepts last_step = n_steps - 1 and reads one row past the end
    ("last_step_reads_past_the_end", dict(cnts=[_term(first=1, last=N - 1)]),
     f"last_step {N - 1} reads waypoint {N}, past the last waypoint n_steps - 1 = {N - 1}"),
    ("use_time_cnt", dict(cnts=[_term(use_time=True)], use_time=True), "cart_vel does not support time"),
    ("use_time_cost", dict(costs=[_term(use_time=True, name="timed_vel")], use_time=True),
     "timed_vel does not support time"),
]


@pytest.mark.parametrize("name, kw, needle", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_with_the_offending_item_named(built, name, kw, needle):
    with pytest.raises(host.HostError) as e:
        host.lower_json(_text(**kw))
    assert needle in str(e.value), str(e.value)


def test_last_step_before_the_end_is_accepted(built):
    desc = host.lower_json(_text(cnts=[_term(first=0, last=N - 2)]))[0]
    assert desc.n_cvel == 1 and desc.cvel_last_step[0] == N - 2


def test_fused_kernel_and_term_values_refuse_without_a_device(built):
    lib = abi.load_hip()
    desc = host.lower_json(_text(**TWO_TERMS))[0]
    ctx = C.c_void_p()
    assert lib.thip_create(0, C.byref(desc), 1, C.byref(ctx)) == -1  # THIP_E_INVALID, not a HIP error
    msg = lib.thip_last_error(None).decode()
    assert "n_cvel" in msg and "generic path" in msg, msg
    tv = C.c_void_p()
    assert lib.thip_terms_create(0, C.byref(desc), 1, C.byref(tv)) == -1
    msg = lib.thip_terms_last_error(None).decode()
    assert "n_cvel" in msg and "generic path" in msg, msg
    nc, nv = C.c_int(), C.c_int()
    assert lib.thip_terms_slot_table(C.byref(desc), None, 0, C.byref(nc), C.byref(nv)) == -1


def test_descriptor_size_matches_the_mirror(built):
    assert abi.load_hip().thip_sizeof_desc() == C.sizeof(abi.ProblemDesc)
    assert abi.MAX_CVEL == 4 and len(abi.ProblemDesc().cvel_max_disp) == 4
