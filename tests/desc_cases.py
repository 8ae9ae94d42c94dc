"""Named descriptor mutations and slot-table problems shared by
tests/golden/make_golden_desc_lowering.py (which records what the library says
about each) and tests/test_desc_lowering.py (which compares a build against the
recording).

REFUSALS: name -> (config, n_steps or None for the config's default, mutate).
Every descriptor is refused by thip_create, thip_terms_create and
thip_terms_slot_table before any device call: one case per finding of the shared
validator (csrc/desc_lowering.hpp), the mutations of tests/test_abi.py and
tests/test_terms_abi.py among them.

SLOT_TABLES: name -> builder of a valid descriptor whose thip_terms_slot_table
output is recorded.
"""
import ctypes as C

from trajopt_amd import abi, problems

MAX_CONTACTS = 131072  # THIP_MAX_CONTACTS
PR2_FIRST_MOVED = 1    # the first link of the PR2 right arm that a joint moves


def _set(name, value):
    return lambda d: setattr(d, name, value)


def _item(name, k, value):
    return lambda d: getattr(d, name).__setitem__(k, value)


def _both(*fs):
    def mutate(d):
        for f in fs:
            f(d)

    return mutate


def _with_collision(evaluator):
    """Config C's collision model on a descriptor without one, on every step."""
    def mutate(d):
        c = problems.make_workload("C", 1).desc
        for name, _ in abi.ProblemDesc._fields_:
            if name.startswith("coll_") or name in ("n_spheres", "sphere_link", "sphere_center", "sphere_radius",
                                                    "n_prims"):
                setattr(d, name, getattr(c, name))
        d.coll_first_step, d.coll_last_step = 0, -1
        d.coll_continuous = evaluator

    return mutate


def _joint_acc(first, last):
    """A JointAccEqCost of the fused form on steps first..last as given."""
    def mutate(d):
        d.n_jdt = 1
        d.jdt_order[0] = 2
        d.jdt_first_step[0], d.jdt_last_step[0] = first, last
        for j in range(d.chain.n_dof):
            d.jdt_coeffs[0][j] = 1.0

    return mutate


def _non_fused_jdt(d):
    # a JointAccEqCost on an odd number of waypoints is not fused (thip_jdt_fused)
    d.n_steps = 7
    d.n_jdt = 1
    d.jdt_order[0] = 2
    d.jdt_first_step[0], d.jdt_last_step[0] = 0, 6


def _tree_parent(d):
    d.chain.is_tree = 1
    for k in range(1, d.chain.n_links):
        d.chain.parent[k] = k - 1
    d.chain.parent[2] = 2


def _coll_fixed(*steps):
    def mutate(d):
        d.coll_n_fixed = len(steps)
        for k, t in enumerate(steps):
            d.coll_fixed_steps[k] = t

    return mutate


def _coll_pair(term, link, other, margin=0.02, coeff=5.0):
    def mutate(d):
        e = d.coll_pairs[d.n_coll_pairs]
        e.term, e.link, e.other, e.margin, e.coeff = term, link, other, margin, coeff
        d.n_coll_pairs += 1

    return mutate


REFUSALS = {
    # tests/test_abi.py (config A at its 10 waypoints)
    "A10_n_steps_1": ("A", None, _set("n_steps", 1)),
    "A10_n_steps_65": ("A", None, _set("n_steps", 65)),
    "A10_osqp_max_iter_0": ("A", None, lambda d: setattr(d.osqp, "max_iter", 0)),
    "A10_coll_enabled_no_spheres": ("A", None, _set("coll_enabled", 1)),
    "A10_n_cart_65": ("A", None, _set("n_cart", 65)),
    "A10_n_jpos_9": ("A", None, _set("n_jpos", 9)),
    "A10_jpos_tol_inf": ("A", None, _both(_set("n_jpos", 1), lambda d: d.jpos_upper_tols[0].__setitem__(2, float("inf")))),
    "A10_jpos_coeff_nan": ("A", None, _both(_set("n_jpos", 1), lambda d: d.jpos_coeffs[0].__setitem__(0, float("nan")))),
    "A10_cart_inverted_band": ("A", None, _both(_item("cart_has_tol", 0, 1),
                                                lambda d: d.cart_lower_tol[0].__setitem__(3, 0.3))),
    "A10_n_jvx_5": ("A", None, _set("n_jvx", 5)),
    "A10_jvx_zero_tols": ("A", None, _set("n_jvx", 1)),
    "A10_coll_continuous_3": ("A", None, _with_collision(3)),
    "A10_jdt_last_is_n_steps": ("A", None, _joint_acc(0, 10)),
    "A10_jdt_first_negative": ("A", None, _joint_acc(-1, 9)),
    "A10_jdt_last_is_first_plus_1": ("A", None, _joint_acc(4, 5)),
    # tests/test_terms_abi.py (6 waypoints)
    "A_jdt_last_is_n_steps": ("A", 6, _joint_acc(0, 6)),
    "A_jdt_first_negative": ("A", 6, _joint_acc(-1, 5)),
    "A_jdt_last_is_first_plus_1": ("A", 6, _joint_acc(2, 3)),
    "A_abi_version": ("A", 6, _set("abi_version", abi.ABI_VERSION + 1)),
    "C_coll_extra": ("C", 6, _set("n_coll_extra", 1)),
    "A_use_time": ("A", 6, _set("use_time", 1)),
    "A_non_fused_jdt": ("A", 6, _non_fused_jdt),
    "A_n_steps_65": ("A", 6, _set("n_steps", abi.MAX_STEPS + 1)),
    "C_n_prims_17": ("C", 6, _set("n_prims", abi.MAX_PRIMS + 1)),
    "C_coll_contact_test_3": ("C", 6, _set("coll_contact_test", 3)),
    "A_cart_source_link_0": ("A", 6, _item("cart_source_link", 0, 0)),
    "A_trust_shrink_ratio": ("A", 6, lambda d: setattr(d.sqp, "trust_shrink_ratio", 1.5)),
    "A_max_time_negative": ("A", 6, lambda d: setattr(d.sqp, "max_time", -1.0)),
    "A_osqp_max_iter_0": ("A", 6, lambda d: setattr(d.osqp, "max_iter", 0)),
    "C_coll_buffer_negative": ("C", 6, _set("coll_buffer", -0.01)),
    "C_self_pair_same_link": ("C", 6, _both(_set("n_self_pairs", 1), lambda d: d.self_pair[0].__setitem__(0, 2),
                                            lambda d: d.self_pair[0].__setitem__(1, 2))),
    "C_n_fixed_65": ("C", 6, _set("n_fixed", abi.MAX_STEPS + 1)),
    # one for each remaining finding
    "A_n_dof_0": ("A", 6, lambda d: setattr(d.chain, "n_dof", 0)),
    "A_n_dof_17": ("A", 6, lambda d: setattr(d.chain, "n_dof", abi.MAX_DOF + 1)),
    "A_n_links_0": ("A", 6, lambda d: setattr(d.chain, "n_links", 0)),
    "A_n_links_33": ("A", 6, lambda d: setattr(d.chain, "n_links", abi.MAX_LINKS + 1)),
    "A_joint_type_4": ("A", 6, lambda d: d.chain.joint_type.__setitem__(2, 4)),
    "A_joint_dof_is_n_dof": ("A", 6, lambda d: d.chain.joint_dof.__setitem__(PR2_FIRST_MOVED, d.chain.n_dof)),
    "A_tree_parent_not_below": ("A", 6, _tree_parent),
    "A_n_fixed_negative": ("A", 6, _set("n_fixed", -1)),
    "A_fixed_step_is_n_steps": ("A", 6, _item("fixed_steps", 0, 6)),
    "A_fixed_step_negative": ("A", 6, _item("fixed_steps", 0, -1)),
    "A_fixed_step_twice": ("A", 6, _both(_set("n_fixed", 2), _item("fixed_steps", 1, 0))),
    "A_n_cart_129": ("A", 6, _set("n_cart", abi.MAX_CART + 1)),
    "A_n_cart_negative": ("A", 6, _set("n_cart", -1)),
    "A_cart_step_is_n_steps": ("A", 6, _item("cart_step", 0, 6)),
    "A_cart_step_negative": ("A", 6, _item("cart_step", 0, -1)),
    "A_cart_target_link_is_n_links": ("A", 6, lambda d: d.cart_target_link.__setitem__(0, d.chain.n_links)),
    "A_cart_target_link_negative": ("A", 6, _item("cart_target_link", 0, -1)),
    "A_n_jvx_negative": ("A", 6, _set("n_jvx", -1)),
    "A_n_jdt_9": ("A", 6, _set("n_jdt", abi.MAX_JDT + 1)),
    "A_n_jvt_1": ("A", 6, _set("n_jvt", 1)),
    "A_n_ttt_1": ("A", 6, _set("n_ttt", 1)),
    "A_n_fixed_dofs_1": ("A", 6, _set("n_fixed_dofs", 1)),
    "A_n_cvel_1": ("A", 6, _set("n_cvel", 1)),
    "A_n_coll_extra_without_collision": ("A", 6, _set("n_coll_extra", 1)),
    "A_n_jpos_negative": ("A", 6, _set("n_jpos", -1)),
    "C_n_spheres_33": ("C", 6, _set("n_spheres", abi.MAX_SPHERES + 1)),
    "C_sphere_link_0": ("C", 6, _item("sphere_link", 1, 0)),
    "C_sphere_link_is_n_links": ("C", 6, lambda d: d.sphere_link.__setitem__(0, d.chain.n_links)),
    "C_sphere_radius_negative": ("C", 6, _item("sphere_radius", 1, -0.01)),
    "C_sphere_radius_nan": ("C", 6, _item("sphere_radius", 0, float("nan"))),
    "C_n_prims_negative": ("C", 6, _set("n_prims", -1)),
    "C_coll_first_step_negative": ("C", 6, _set("coll_first_step", -1)),
    "C_coll_first_step_is_n_steps": ("C", 6, _set("coll_first_step", 6)),
    "C_coll_last_step_is_n_steps": ("C", 6, _set("coll_last_step", 6)),
    "C_coll_last_before_first": ("C", 6, _both(_set("coll_first_step", 3), _set("coll_last_step", 2))),
    "C_coll_continuous_negative": ("C", 6, _set("coll_continuous", -1)),
    "C_coll_lvs_0": ("C", 6, _set("coll_lvs", 0.0)),
    "C_coll_adjacent_fixed": ("C", 6, _coll_fixed(2, 3)),
    "C_coll_max_contacts_negative": ("C", 6, _set("coll_max_contacts", -1)),
    "C_coll_max_contacts_over": ("C", 6, _set("coll_max_contacts", MAX_CONTACTS + 1)),
    "C_n_self_pairs_65": ("C", 6, _set("n_self_pairs", abi.MAX_SELF_PAIRS + 1)),
    "C_n_coll_pairs_65": ("C", 6, _set("n_coll_pairs", abi.MAX_COLL_PAIRS + 1)),
    "C_coll_pair_term_1": ("C", 6, _coll_pair(1, 2, 0)),
    "C_coll_pair_link_is_n_links": ("C", 6, lambda d: _coll_pair(0, d.chain.n_links, 0)(d)),
    "C_coll_pair_other_is_n_prims": ("C", 6, lambda d: _coll_pair(0, 2, d.n_prims)(d)),
    "C_coll_pair_margin_inf": ("C", 6, _coll_pair(0, 2, 0, margin=float("inf"))),
    "A_coll_pair_without_collision": ("A", 6, _coll_pair(0, 2, 0)),
    "A_trust_shrink_ratio_0": ("A", 6, lambda d: setattr(d.sqp, "trust_shrink_ratio", 0.0)),
    "A_min_trust_box_size_0": ("A", 6, lambda d: setattr(d.sqp, "min_trust_box_size", 0.0)),
    "A_trust_box_size_0": ("A", 6, lambda d: setattr(d.sqp, "trust_box_size", 0.0)),
    "A_max_time_nan": ("A", 6, lambda d: setattr(d.sqp, "max_time", float("nan"))),
    "A_check_termination_negative": ("A", 6, lambda d: setattr(d.osqp, "check_termination", -1)),
    "A_osqp_scaling_negative": ("A", 6, lambda d: setattr(d.osqp, "scaling", -1)),
}

# Refusals that are not recorded, since the build the recording was made on got them wrong:
# name -> (config, n_steps, mutate, the reason every entry point gives after its own prefix).
#  * coll_n_fixed outside [0, THIP_MAX_STEPS]: thip_create did not test it and read
#    coll_fixed_steps past its end;
#  * a negative first step of a JointVel term: JointVelTermInfo::hatch clamps it from above
#    only, and the kernels index the trajectory with the clamped steps.
UNRECORDED_REFUSALS = {
    "C_coll_n_fixed_65": ("C", 6, _set("coll_n_fixed", 65), "collision: coll_n_fixed out of range"),
    "C_coll_n_fixed_1000": ("C", 6, _set("coll_n_fixed", 1000), "collision: coll_n_fixed out of range"),
    "C_coll_n_fixed_negative": ("C", 6, _set("coll_n_fixed", -1), "collision: coll_n_fixed out of range"),
    "A_jv_first_step_negative": ("A", 6, _set("jv_first_step", -1), "jv_first_step must be >= 0"),
    "unit_jvx_first_step_negative": ("joint_vel_ineq", None, _item("jvx_first_step", 1, -1),
                                     "jvx term 1: jvx_first_step must be >= 0"),
}


def _desc(config, n_steps, mutate):
    if config in ("joint_pos_eq", "joint_pos_ineq", "joint_vel_ineq"):
        d = problems.make_reference_unit(config).desc
    else:
        d = problems.make_workload(config, 1, n_steps=n_steps).desc
    mutate(d)
    return d


def refusal_desc(name):
    return _desc(*REFUSALS[name])


def unrecorded_refusal(name):
    """The descriptor and the three messages it must get."""
    config, n_steps, mutate, reason = UNRECORDED_REFUSALS[name]
    return _desc(config, n_steps, mutate), {f: f"{f}: {reason}" for f in
                                            ("thip_create", "thip_terms_create", "thip_terms_slot_table")}


def _config(config, *mutations, **kw):
    def build():
        d = problems.make_workload(config, 1, n_steps=6, **kw).desc
        for m in mutations:
            m(d)
        return d

    return build


def _unit(name):
    return lambda: problems.make_reference_unit(name).desc


def _jpos_tols(k, lower, upper):
    def mutate(d):
        for j in range(d.chain.n_dof):
            d.jpos_lower_tols[k][j], d.jpos_upper_tols[k][j] = lower, upper

    return mutate


def _joint_acc_2dof():
    return problems.with_joint_acc(problems.make_workload("B", 1, n_steps=6, robot="right_arm_2dof")).desc


SLOT_TABLES = {
    "A": _config("A"),
    "B": _config("B"),
    "C": _config("C"),
    "J": _config("J"),  # a JointPos cost and a JointPos constraint with zero tolerances
    "E": _config("E"),
    "HA": _config("HA"),
    "C_coll_is_cnt": _config("C", _set("coll_is_cnt", 1)),
    "C_discrete_fixed_0_3": _config("C", _set("coll_continuous", 2), _coll_fixed(0, 3)),
    "C_discrete_cnt_fixed_0_3": _config("C", _set("coll_continuous", 2), _set("coll_is_cnt", 1), _coll_fixed(0, 3)),
    "C_steps_1_4": _config("C", _set("coll_first_step", 1), _set("coll_last_step", 4)),
    # (config A's only CartPose is a constraint already; B's second made one shows the
    # two passes: costs in descriptor order, then constraints)
    "A_cart_cost": _config("A", _item("cart_is_cnt", 0, 0)),
    "B_cart_1_cnt": _config("B", _item("cart_is_cnt", 1, 1)),
    "B_cart_zero_coeffs": _config("B", lambda d: d.cart_rot_coeffs[2].__setitem__(1, 0.0),
                                  lambda d: d.cart_pos_coeffs[2].__setitem__(0, 0.0)),
    "J_cnt_with_tols": _config("J", _jpos_tols(1, -0.1, 0.2)),
    "J_cost_with_tols": _config("J", _jpos_tols(0, -0.01, 0.01)),
    "J_reversed_steps": _config("J", _item("jpos_first_step", 0, 9), _item("jpos_last_step", 0, -3)),
    "unit_joint_pos_eq": _unit("joint_pos_eq"),
    "unit_joint_pos_ineq": _unit("joint_pos_ineq"),
    "unit_joint_vel_ineq": _unit("joint_vel_ineq"),  # a jvx cost and a jvx constraint
    "joint_acc_2dof": _joint_acc_2dof,
    "no_joint_vel": _config("B", _set("jv_enabled", 0)),
}


def refusals_of(lib, d):
    """The three messages a refused descriptor gets, each the whole string."""
    ctx, t = C.c_void_p(), C.c_void_p()
    nc, nv = C.c_int(), C.c_int()
    assert lib.thip_create(0, C.byref(d), 3, C.byref(ctx)) == -1 and not ctx
    create = lib.thip_last_error(None).decode()
    assert lib.thip_terms_create(0, C.byref(d), 3, C.byref(t)) == -1 and not t
    terms_create = lib.thip_terms_last_error(None).decode()
    assert lib.thip_terms_slot_table(C.byref(d), None, 0, C.byref(nc), C.byref(nv)) == -1
    slot_table = lib.thip_terms_last_error(None).decode()
    return {"thip_create": create, "thip_terms_create": terms_create, "thip_terms_slot_table": slot_table}


def slot_table_of(lib, d):
    nc, nv = C.c_int(), C.c_int()
    cap = 4 * abi.MAX_CART
    tab = (abi.TermSlot * cap)()
    assert lib.thip_terms_slot_table(C.byref(d), tab, cap, C.byref(nc), C.byref(nv)) == 0, \
        lib.thip_terms_last_error(None).decode()
    n = nc.value + nv.value
    assert n <= cap
    return {"n_costs": nc.value, "n_cnts": nv.value,
            "slots": [[s.kind, s.index, s.unit, s.is_cnt] for s in tab[:n]]}
