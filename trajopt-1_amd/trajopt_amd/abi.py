"""ctypes mirror of include/trajopt_hip.h and the loader of the HIP library.

The HIP library (libtrajopt_hip.so, built in-tree by __graft_entry__.build())
is the only compute path. `load_hip()` raises if it is missing: there is no
CPU fallback anywhere in the product.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

ABI_VERSION = 10  # THIP_ABI_VERSION
CONTACT_ALL, CONTACT_FIRST, CONTACT_CLOSEST = 0, 1, 2  # THIP_CONTACT_* (collision contact_test_type)
MAX_DOF = 16
MAX_LINKS = 32
MAX_STEPS = 64
MAX_CART = 128
MAX_SPHERES = 32
MAX_PRIMS = 16
MAX_JPOS = 8
MAX_JVX = 4
MAX_JDT = 8
MAX_JVT = 4
MAX_TTT = 2
MAX_CVEL = 4
MAX_COLL_EXTRA = 3
MAX_SELF_PAIRS = 64
MAX_SELF_SPHERE_PAIRS = 512
MAX_COLL_PAIRS = 64
EVAL_MAX_STEPS = 4096  # THIP_EVAL_MAX_STEPS: the generic path's horizon
EVAL_MAX_PRIMS = 1024  # THIP_EVAL_MAX_PRIMS
TRACE_W = 16  # THIP_TRACE_W
CHECK_CHUNK = 8  # THIP_CHECK_CHUNK: sub-states per chunk of the trajectory checker's kernel
CHECK_LVS_DISCRETE, CHECK_LVS_CONTINUOUS, CHECK_DISCRETE = 0, 1, 2  # thip_check_config.type (the coll_continuous encoding)
DEBUG_NO_SEGMENT, DEBUG_FORCE_WIDE, DEBUG_NO_BRANCH, DEBUG_STATIC_DISPATCH, DEBUG_GEN_BUILD = 1, 2, 4, 8, 16  # thip_debug_set_path flags
DEBUG_MAIN_BUILD = 32
DEBUG_SEG_REBUILD = 64  # the segment's packs rebuilt at every call (bitwise the same results)
DEBUG_SEG_RETURN = 128  # the segment returns at every termination check, third infeasibility tests unused (same bits)
DEBUG_SETUP_REF = 256  # the QP set-up's serial Ruiz column-norm loops, as before round 9 (same bits)
DEBUG_FP_REF = 512  # the sparsity fingerprint from thread 0's serial walk, as before round 12 (same bits)

JOINT_FIXED, JOINT_REVOLUTE, JOINT_CONTINUOUS, JOINT_PRISMATIC = 0, 1, 2, 3
PRIM_SPHERE, PRIM_BOX, PRIM_CAPSULE = 0, 1, 2

OPT_STATUS = {
    0: "OPT_CONVERGED",
    1: "OPT_SCO_ITERATION_LIMIT",
    2: "OPT_PENALTY_ITERATION_LIMIT",
    3: "OPT_TIME_LIMIT",
    4: "OPT_FAILED",
    5: "INVALID",
}

_D12 = C.c_double * 12
_D3 = C.c_double * 3


class Chain(C.Structure):
    _fields_ = [
        ("n_links", C.c_int),
        ("n_dof", C.c_int),
        ("is_tree", C.c_int),
        ("base_pose", C.c_double * 12),
        ("joint_type", C.c_int * MAX_LINKS),
        ("joint_dof", C.c_int * MAX_LINKS),
        ("parent", C.c_int * MAX_LINKS),
        ("joint_origin", _D12 * MAX_LINKS),
        ("joint_axis", _D3 * MAX_LINKS),
        ("lower", C.c_double * MAX_DOF),
        ("upper", C.c_double * MAX_DOF),
    ]


class SqpParams(C.Structure):
    _fields_ = [
        ("improve_ratio_threshold", C.c_double),
        ("min_trust_box_size", C.c_double),
        ("min_approx_improve", C.c_double),
        ("min_approx_improve_frac", C.c_double),
        ("max_iter", C.c_int),
        ("trust_shrink_ratio", C.c_double),
        ("trust_expand_ratio", C.c_double),
        ("cnt_tolerance", C.c_double),
        ("max_merit_coeff_increases", C.c_double),
        ("max_qp_solver_failures", C.c_int),
        ("merit_coeff_increase_ratio", C.c_double),
        ("initial_merit_error_coeff", C.c_double),
        ("inflate_constraints_individually", C.c_int),
        ("trust_box_size", C.c_double),
        ("max_time", C.c_double),
    ]


class OsqpSettings(C.Structure):
    _fields_ = [
        ("rho", C.c_double),
        ("sigma", C.c_double),
        ("alpha", C.c_double),
        ("scaling", C.c_int),
        ("adaptive_rho", C.c_int),
        ("adaptive_rho_interval", C.c_int),
        ("adaptive_rho_tolerance", C.c_double),
        ("max_iter", C.c_int),
        ("eps_abs", C.c_double),
        ("eps_rel", C.c_double),
        ("eps_prim_inf", C.c_double),
        ("eps_dual_inf", C.c_double),
        ("check_termination", C.c_int),
        ("warm_starting", C.c_int),
        ("polishing", C.c_int),
        ("delta", C.c_double),
        ("polish_refine_iter", C.c_int),
    ]


class CollTerm(C.Structure):
    """thip_coll_term: a collision term beyond the descriptor's first."""
    _fields_ = [
        ("is_cnt", C.c_int),
        ("first_step", C.c_int),
        ("last_step", C.c_int),
        ("n_fixed", C.c_int),
        ("fixed_steps", C.c_int * MAX_STEPS),
        ("margin", C.c_double),
        ("coeff", C.c_double),
        ("buffer", C.c_double),
        ("lvs", C.c_double),
        ("continuous", C.c_int),
        ("contact_test", C.c_int),
    ]


class CollPair(C.Structure):
    """thip_coll_pair: one link pair's margin and coefficient in a collision term."""
    _fields_ = [
        ("term", C.c_int),
        ("link", C.c_int),
        ("other", C.c_int),
        ("pad_", C.c_int),
        ("margin", C.c_double),
        ("coeff", C.c_double),
    ]


class ProblemDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int),
        ("n_steps", C.c_int),
        ("chain", Chain),
        ("n_fixed", C.c_int),
        ("fixed_steps", C.c_int * MAX_STEPS),
        ("jv_enabled", C.c_int),
        ("jv_first_step", C.c_int),
        ("jv_last_step", C.c_int),
        ("jv_coeffs", C.c_double * MAX_DOF),
        ("jv_targets", C.c_double * MAX_DOF),
        ("jv_upper_tols", C.c_double * MAX_DOF),
        ("jv_lower_tols", C.c_double * MAX_DOF),
        ("n_cart", C.c_int),
        ("cart_step", C.c_int * MAX_CART),
        ("cart_is_cnt", C.c_int * MAX_CART),
        ("cart_source_link", C.c_int * MAX_CART),
        ("cart_source_offset", _D12 * MAX_CART),
        ("cart_pos_coeffs", _D3 * MAX_CART),
        ("cart_rot_coeffs", _D3 * MAX_CART),
        ("cart_has_tol", C.c_int * MAX_CART),
        ("cart_lower_tol", (C.c_double * 6) * MAX_CART),
        ("cart_upper_tol", (C.c_double * 6) * MAX_CART),
        ("cart_target_link", C.c_int * MAX_CART),
        ("n_jpos", C.c_int),
        ("jpos_is_cnt", C.c_int * MAX_JPOS),
        ("jpos_first_step", C.c_int * MAX_JPOS),
        ("jpos_last_step", C.c_int * MAX_JPOS),
        ("jpos_coeffs", (C.c_double * MAX_DOF) * MAX_JPOS),
        ("jpos_targets", (C.c_double * MAX_DOF) * MAX_JPOS),
        ("jpos_upper_tols", (C.c_double * MAX_DOF) * MAX_JPOS),
        ("jpos_lower_tols", (C.c_double * MAX_DOF) * MAX_JPOS),
        ("n_jvx", C.c_int),
        ("jvx_is_cnt", C.c_int * MAX_JVX),
        ("jvx_first_step", C.c_int * MAX_JVX),
        ("jvx_last_step", C.c_int * MAX_JVX),
        ("jvx_coeffs", (C.c_double * MAX_DOF) * MAX_JVX),
        ("jvx_targets", (C.c_double * MAX_DOF) * MAX_JVX),
        ("jvx_upper_tols", (C.c_double * MAX_DOF) * MAX_JVX),
        ("jvx_lower_tols", (C.c_double * MAX_DOF) * MAX_JVX),
        ("n_jdt", C.c_int),
        ("jdt_order", C.c_int * MAX_JDT),
        ("jdt_is_cnt", C.c_int * MAX_JDT),
        ("jdt_first_step", C.c_int * MAX_JDT),
        ("jdt_last_step", C.c_int * MAX_JDT),
        ("jdt_coeffs", (C.c_double * MAX_DOF) * MAX_JDT),
        ("jdt_targets", (C.c_double * MAX_DOF) * MAX_JDT),
        ("jdt_upper_tols", (C.c_double * MAX_DOF) * MAX_JDT),
        ("jdt_lower_tols", (C.c_double * MAX_DOF) * MAX_JDT),
        ("use_time", C.c_int),
        ("dt_lower", C.c_double),
        ("dt_upper", C.c_double),
        ("init_dt", C.c_double),
        ("n_fixed_dofs", C.c_int),
        ("fixed_dofs", C.c_int * MAX_DOF),
        ("n_jvt", C.c_int),
        ("jvt_is_cnt", C.c_int * MAX_JVT),
        ("jvt_first_step", C.c_int * MAX_JVT),
        ("jvt_last_step", C.c_int * MAX_JVT),
        ("jvt_coeffs", (C.c_double * MAX_DOF) * MAX_JVT),
        ("jvt_targets", (C.c_double * MAX_DOF) * MAX_JVT),
        ("jvt_upper_tols", (C.c_double * MAX_DOF) * MAX_JVT),
        ("jvt_lower_tols", (C.c_double * MAX_DOF) * MAX_JVT),
        ("n_ttt", C.c_int),
        ("ttt_is_cnt", C.c_int * MAX_TTT),
        ("ttt_coeff", C.c_double * MAX_TTT),
        ("ttt_limit", C.c_double * MAX_TTT),
        ("coll_enabled", C.c_int),
        ("coll_is_cnt", C.c_int),
        ("coll_first_step", C.c_int),
        ("coll_last_step", C.c_int),
        ("coll_n_fixed", C.c_int),
        ("coll_fixed_steps", C.c_int * MAX_STEPS),
        ("coll_margin", C.c_double),
        ("coll_coeff", C.c_double),
        ("coll_buffer", C.c_double),
        ("coll_lvs", C.c_double),
        ("coll_continuous", C.c_int),
        ("coll_contact_test", C.c_int),
        ("n_spheres", C.c_int),
        ("sphere_link", C.c_int * MAX_SPHERES),
        ("sphere_center", _D3 * MAX_SPHERES),
        ("sphere_radius", C.c_double * MAX_SPHERES),
        ("n_prims", C.c_int),
        ("n_self_pairs", C.c_int),
        ("self_pair", (C.c_int * 2) * MAX_SELF_PAIRS),
        ("coll_max_contacts", C.c_int),
        ("n_coll_extra", C.c_int),
        ("coll_extra", CollTerm * MAX_COLL_EXTRA),
        ("n_coll_pairs", C.c_int),
        ("coll_pairs", CollPair * MAX_COLL_PAIRS),
        ("sqp", SqpParams),
        ("osqp", OsqpSettings),
        # CartVel terms (ABI 10): after the solver parameters, so no earlier field moved
        ("n_cvel", C.c_int),
        ("cvel_is_cnt", C.c_int * MAX_CVEL),
        ("cvel_link", C.c_int * MAX_CVEL),
        ("cvel_first_step", C.c_int * MAX_CVEL),
        ("cvel_last_step", C.c_int * MAX_CVEL),
        ("cvel_max_disp", C.c_double * MAX_CVEL),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.abi_version = ABI_VERSION


class Result(C.Structure):
    _fields_ = [
        ("status", C.c_int),
        ("n_sqp_iters", C.c_int),
        ("n_qp_solves", C.c_int),
        ("n_func_evals", C.c_int),
        ("n_admm_iters", C.c_longlong),
        ("n_merit_increases", C.c_int),
        ("total_cost", C.c_double),
        ("max_cnt_viol", C.c_double),
        ("final_trust_box", C.c_double),
        ("n_costs", C.c_int),
        ("n_cnts", C.c_int),
        ("flags", C.c_int),
        ("n_contact_rows", C.c_longlong),
        ("n_hinge_admm", C.c_longlong),
        ("n_substates", C.c_longlong),
    ]


class CheckConfig(C.Structure):
    """thip_check_config: what a trajectory check tests."""
    _fields_ = [
        ("type", C.c_int),
        ("lvs", C.c_double),
        ("margin", C.c_double),
        ("first_step", C.c_int),
        ("last_step", C.c_int),
    ]


class CheckResult(C.Structure):
    """thip_check_result: one problem's verdict and clearance."""
    _fields_ = [
        ("found", C.c_int),
        ("n_contacts", C.c_int),
        ("first_unit", C.c_int),
        ("n_candidates", C.c_longlong),
        ("min_distance", C.c_double),
        ("min_t", C.c_int),
        ("min_link", C.c_int),
        ("min_other", C.c_int),
        ("min_sphere", C.c_int),
        ("min_substate", C.c_int),
        ("min_cc_time", C.c_double),
    ]


CSETS_MAX_ROWS = 64  # THIP_CSETS_MAX_ROWS: rows per node of a collision set


class CsetsConfig(C.Structure):
    """thip_csets_config: the collision sets of thip_csets_* (TrajOptCollisionConfig's
    margin / coeff / buffer, rows per node, the nodes that carry a set)."""
    _fields_ = [
        ("margin", C.c_double),
        ("coeff", C.c_double),
        ("margin_buffer", C.c_double),
        ("max_num_cnt", C.c_int),
        ("first_step", C.c_int),
        ("last_step", C.c_int),
    ]


CCSETS_MAX_SUBSTATES = 4096  # THIP_CCSETS_MAX_SUBSTATES: states of one segment of a continuous collision set
# thip_ccsets_config.evaluator_type (THIP_EVALUATOR_*: tesseract's CollisionEvaluatorType values)
EVALUATOR_LVS_DISCRETE, EVALUATOR_CONTINUOUS, EVALUATOR_LVS_CONTINUOUS = 2, 3, 4


class CcsetsConfig(C.Structure):
    """thip_ccsets_config: the continuous collision sets of thip_ccsets_* (margin / coeff /
    buffer, rows per segment, the segments (t, t + 1) of first_step <= t < last_step, the
    evaluator type and its longest valid segment length)."""
    _fields_ = [
        ("margin", C.c_double),
        ("coeff", C.c_double),
        ("margin_buffer", C.c_double),
        ("max_num_cnt", C.c_int),
        ("first_step", C.c_int),
        ("last_step", C.c_int),
        ("evaluator_type", C.c_int),
        ("longest_valid_segment_length", C.c_double),
    ]


TERM_JOINT_VEL, TERM_JVX, TERM_JPOS, TERM_JDT, TERM_CART, TERM_COLL = range(6)  # thip_term_slot.kind (THIP_TERM_*)
TERM_KIND_NAMES = ("joint_vel", "jvx", "jpos", "jdt", "cart", "coll")
# workspace arrays of layout.hpp's DArr / IArr that thip_debug_layout + thip_debug_workspace expose to tests
WS_A_COST, WS_A_VIOL, WS_I_PCNT = 6, 7, 10


class TermSlot(C.Structure):
    """thip_term_slot: what one cost / constraint slot of thip_terms_run holds."""
    _fields_ = [
        ("kind", C.c_int),
        ("index", C.c_int),
        ("unit", C.c_int),
        ("is_cnt", C.c_int),
    ]


# thip_qp_step's per-QP operation bits (THIP_QP_OP_*), run in this order
QP_OP_SETUP, QP_OP_MAT_P, QP_OP_VEC_Q, QP_OP_MAT_A, QP_OP_VEC_BOUNDS, QP_OP_WARM, QP_OP_SOLVE = 1, 2, 4, 8, 16, 32, 64
E_INVALID, E_HIP, E_NOMEM, E_STATE = -1, -2, -3, -4  # THIP_E_*


class QpInfo(C.Structure):
    """thip_qp_info (include/trajopt_hip.h): one generic QP's solve report."""

    _fields_ = [
        ("status", C.c_int),
        ("setup_error", C.c_int),
        ("polish_status", C.c_int),
        ("iter", C.c_int),
        ("rho", C.c_double),
        ("prim_res", C.c_double),
        ("dual_res", C.c_double),
    ]


def default_check_config() -> CheckConfig:
    """thip_default_check_config: one cast per step pair (CONTINUOUS), margin 0, every step."""
    return CheckConfig(CHECK_LVS_CONTINUOUS, float("inf"), 0.0, 0, -1)


def default_sqp_params() -> SqpParams:
    """sco::BasicTrustRegionSQPParameters defaults (optimizers.hpp:92-135)."""
    p = SqpParams()
    p.improve_ratio_threshold = 0.25
    p.min_trust_box_size = 1e-4
    p.min_approx_improve = 1e-4
    p.min_approx_improve_frac = -1.7976931348623157e308
    p.max_iter = 50
    p.trust_shrink_ratio = 0.1
    p.trust_expand_ratio = 1.5
    p.cnt_tolerance = 1e-4
    p.max_merit_coeff_increases = 5
    p.max_qp_solver_failures = 3
    p.merit_coeff_increase_ratio = 10
    p.initial_merit_error_coeff = 10
    p.inflate_constraints_individually = 1
    p.trust_box_size = 1e-1
    p.max_time = 1.7976931348623157e308
    return p


def default_osqp_settings() -> OsqpSettings:
    """OSQP 1.0 defaults + OSQPModelConfig::setDefaultOSQPSettings overrides
    (trajopt_sco/src/osqp_interface.cpp:78-90)."""
    s = OsqpSettings()
    s.rho = 0.1
    s.sigma = 1e-6
    s.alpha = 1.6
    s.scaling = 10
    s.adaptive_rho = 1
    s.adaptive_rho_interval = 0
    s.adaptive_rho_tolerance = 5.0
    s.max_iter = 8192
    s.eps_abs = 1e-4
    s.eps_rel = 1e-6
    s.eps_prim_inf = 1e-4
    s.eps_dual_inf = 1e-4
    s.check_termination = 25
    s.warm_starting = 1
    s.polishing = 1
    s.delta = 1e-6
    s.polish_refine_iter = 3
    return s


PKG_DIR = Path(__file__).resolve().parent.parent          # trajopt-1_amd/
LIB_DIR = PKG_DIR / "lib"
HIP_LIB = LIB_DIR / "libtrajopt_hip.so"

_hip = None


def _declare(lib):
    P = C.POINTER
    vp = C.c_void_p
    dp = P(C.c_double)
    lib.thip_create.argtypes = [C.c_int, P(ProblemDesc), C.c_int, P(vp)]
    lib.thip_create.restype = C.c_int
    lib.thip_set_stream.argtypes = [vp, vp]
    lib.thip_set_stream.restype = C.c_int
    lib.thip_upload.argtypes = [vp, dp, dp, dp]
    lib.thip_upload.restype = C.c_int
    lib.thip_upload_joint_targets.argtypes = [vp, dp]
    lib.thip_upload_joint_targets.restype = C.c_int
    lib.thip_upload_device.argtypes = [vp, vp, vp, vp]
    lib.thip_upload_device.restype = C.c_int
    lib.thip_sqp_run.argtypes = [vp]
    lib.thip_sqp_run.restype = C.c_int
    lib.thip_synchronize.argtypes = [vp]
    lib.thip_synchronize.restype = C.c_int
    lib.thip_linearize.argtypes = [vp, dp, dp, dp]
    lib.thip_linearize.restype = C.c_int
    lib.thip_fwd_kin.argtypes = [vp, dp, dp]
    lib.thip_fwd_kin.restype = C.c_int
    lib.thip_download.argtypes = [vp, dp, P(Result)]
    lib.thip_download.restype = C.c_int
    lib.thip_device_x.argtypes = [vp]
    lib.thip_device_x.restype = vp
    lib.thip_last_kernel_ms.argtypes = [vp]
    lib.thip_last_kernel_ms.restype = C.c_double
    lib.thip_destroy.argtypes = [vp]
    lib.thip_destroy.restype = None
    lib.thip_last_error.argtypes = [vp]
    lib.thip_last_error.restype = C.c_char_p
    lib.thip_build_info.argtypes = []
    lib.thip_build_info.restype = C.c_char_p
    lib.thip_default_sqp_params.argtypes = [P(SqpParams)]
    lib.thip_default_sqp_params.restype = None
    lib.thip_default_osqp_settings.argtypes = [P(OsqpSettings)]
    lib.thip_default_osqp_settings.restype = None
    lib.thip_debug_trace.argtypes = [vp, C.c_int]
    lib.thip_debug_trace.restype = C.c_int
    lib.thip_debug_get_trace.argtypes = [vp, dp, P(C.c_int)]
    lib.thip_debug_get_trace.restype = C.c_int
    lib.thip_collision_rows.argtypes = [vp, dp, dp, C.c_int, P(C.c_int)]
    lib.thip_collision_rows.restype = C.c_int
    lib.thip_debug_profile.argtypes = [vp, C.c_int]
    lib.thip_debug_profile.restype = C.c_int
    lib.thip_debug_get_profile.argtypes = [vp, P(C.c_longlong)]
    lib.thip_debug_get_profile.restype = C.c_int
    lib.thip_debug_set_path.argtypes = [C.c_int]
    lib.thip_debug_set_path.restype = C.c_int
    lib.thip_jdt_fused.argtypes = [C.POINTER(ProblemDesc)]
    lib.thip_jdt_fused.restype = C.c_int
    lib.thip_debug_solve_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    lib.thip_debug_solve_layout.restype = C.c_int
    lib.thip_eval_create.argtypes = [C.c_int, P(ProblemDesc), C.c_int, P(vp)]
    lib.thip_eval_create.restype = C.c_int
    lib.thip_eval_upload.argtypes = [vp, dp, dp]
    lib.thip_eval_upload.restype = C.c_int
    lib.thip_eval_cart_pose.argtypes = [vp, C.c_int, dp, dp, dp]
    lib.thip_eval_cart_pose.restype = C.c_int
    lib.thip_eval_cart_vel_pairs.argtypes = [vp]
    lib.thip_eval_cart_vel_pairs.restype = C.c_int
    lib.thip_eval_cart_vel_all.argtypes = [vp, dp, dp, dp]
    lib.thip_eval_cart_vel_all.restype = C.c_int
    lib.thip_eval_collision.argtypes = [vp, C.c_int, dp, dp, C.c_int, P(C.c_int)]
    lib.thip_eval_collision.restype = C.c_int
    lib.thip_eval_destroy.argtypes = [vp]
    lib.thip_eval_destroy.restype = None
    lib.thip_eval_last_error.argtypes = [vp]
    lib.thip_eval_last_error.restype = C.c_char_p
    lib.thip_default_check_config.argtypes = [P(CheckConfig)]
    lib.thip_default_check_config.restype = None
    lib.thip_sizeof_check_config.argtypes = []
    lib.thip_sizeof_check_config.restype = C.c_int
    lib.thip_sizeof_check_result.argtypes = []
    lib.thip_sizeof_check_result.restype = C.c_int
    lib.thip_check_create.argtypes = [C.c_int, P(ProblemDesc), P(CheckConfig), C.c_int, P(vp)]
    lib.thip_check_create.restype = C.c_int
    lib.thip_check_upload.argtypes = [vp, dp]
    lib.thip_check_upload.restype = C.c_int
    lib.thip_check_upload_device.argtypes = [vp, vp]
    lib.thip_check_upload_device.restype = C.c_int
    lib.thip_check_units.argtypes = [vp]
    lib.thip_check_units.restype = C.c_int
    lib.thip_check_run.argtypes = [vp, dp, P(CheckResult), dp]
    lib.thip_check_run.restype = C.c_int
    lib.thip_check_run_device.argtypes = [vp, vp, P(CheckResult), dp]
    lib.thip_check_run_device.restype = C.c_int
    lib.thip_check_last_ms.argtypes = [vp]
    lib.thip_check_last_ms.restype = C.c_double
    lib.thip_check_destroy.argtypes = [vp]
    lib.thip_check_destroy.restype = None
    lib.thip_check_last_error.argtypes = [vp]
    lib.thip_check_last_error.restype = C.c_char_p
    lib.thip_sizeof_term_slot.argtypes = []
    lib.thip_sizeof_term_slot.restype = C.c_int
    lib.thip_terms_create.argtypes = [C.c_int, P(ProblemDesc), C.c_int, P(vp)]
    lib.thip_terms_create.restype = C.c_int
    lib.thip_terms_slot_table.argtypes = [P(ProblemDesc), P(TermSlot), C.c_int, P(C.c_int), P(C.c_int)]
    lib.thip_terms_slot_table.restype = C.c_int
    lib.thip_terms_counts.argtypes = [vp, P(C.c_int), P(C.c_int)]
    lib.thip_terms_counts.restype = C.c_int
    lib.thip_terms_slots.argtypes = [vp, P(TermSlot)]
    lib.thip_terms_slots.restype = C.c_int
    lib.thip_terms_upload.argtypes = [vp, dp, dp]
    lib.thip_terms_upload.restype = C.c_int
    lib.thip_terms_upload_device.argtypes = [vp, vp, vp]
    lib.thip_terms_upload_device.restype = C.c_int
    lib.thip_terms_upload_joint_targets.argtypes = [vp, dp]
    lib.thip_terms_upload_joint_targets.restype = C.c_int
    lib.thip_terms_upload_joint_targets_device.argtypes = [vp, vp]
    lib.thip_terms_upload_joint_targets_device.restype = C.c_int
    lib.thip_terms_run.argtypes = [vp, dp, dp, dp]
    lib.thip_terms_run.restype = C.c_int
    lib.thip_terms_run_device.argtypes = [vp, vp, dp, dp]
    lib.thip_terms_run_device.restype = C.c_int
    lib.thip_terms_last_ms.argtypes = [vp]
    lib.thip_terms_last_ms.restype = C.c_double
    lib.thip_terms_destroy.argtypes = [vp]
    lib.thip_terms_destroy.restype = None
    lib.thip_terms_last_error.argtypes = [vp]
    lib.thip_terms_last_error.restype = C.c_char_p
    ip = P(C.c_int)
    lib.thip_default_csets_config.argtypes = [P(CsetsConfig)]
    lib.thip_default_csets_config.restype = None
    lib.thip_sizeof_csets_config.argtypes = []
    lib.thip_sizeof_csets_config.restype = C.c_int
    lib.thip_csets_create.argtypes = [C.c_int, P(ProblemDesc), P(CsetsConfig), C.c_int, P(vp)]
    lib.thip_csets_create.restype = C.c_int
    lib.thip_csets_upload.argtypes = [vp, dp]
    lib.thip_csets_upload.restype = C.c_int
    lib.thip_csets_upload_device.argtypes = [vp, vp]
    lib.thip_csets_upload_device.restype = C.c_int
    lib.thip_csets_nodes.argtypes = [vp]
    lib.thip_csets_nodes.restype = C.c_int
    lib.thip_csets_run.argtypes = [vp, dp, dp, dp, dp, ip, ip]
    lib.thip_csets_run.restype = C.c_int
    lib.thip_csets_run_device.argtypes = [vp, vp, dp, dp, dp, ip, ip]
    lib.thip_csets_run_device.restype = C.c_int
    lib.thip_csets_last_ms.argtypes = [vp]
    lib.thip_csets_last_ms.restype = C.c_double
    lib.thip_csets_destroy.argtypes = [vp]
    lib.thip_csets_destroy.restype = None
    lib.thip_csets_last_error.argtypes = [vp]
    lib.thip_csets_last_error.restype = C.c_char_p
    lib.thip_default_ccsets_config.argtypes = [P(CcsetsConfig)]
    lib.thip_default_ccsets_config.restype = None
    lib.thip_sizeof_ccsets_config.argtypes = []
    lib.thip_sizeof_ccsets_config.restype = C.c_int
    lib.thip_ccsets_create.argtypes = [C.c_int, P(ProblemDesc), P(CcsetsConfig), ip, C.c_int, P(vp)]
    lib.thip_ccsets_create.restype = C.c_int
    lib.thip_ccsets_upload.argtypes = [vp, dp]
    lib.thip_ccsets_upload.restype = C.c_int
    lib.thip_ccsets_upload_device.argtypes = [vp, vp]
    lib.thip_ccsets_upload_device.restype = C.c_int
    lib.thip_ccsets_segments.argtypes = [vp]
    lib.thip_ccsets_segments.restype = C.c_int
    lib.thip_ccsets_run.argtypes = [vp, dp, dp, dp, dp, ip, ip]
    lib.thip_ccsets_run.restype = C.c_int
    lib.thip_ccsets_run_device.argtypes = [vp, vp, dp, dp, dp, ip, ip]
    lib.thip_ccsets_run_device.restype = C.c_int
    lib.thip_ccsets_last_ms.argtypes = [vp]
    lib.thip_ccsets_last_ms.restype = C.c_double
    lib.thip_ccsets_destroy.argtypes = [vp]
    lib.thip_ccsets_destroy.restype = None
    lib.thip_ccsets_last_error.argtypes = [vp]
    lib.thip_ccsets_last_error.restype = C.c_char_p
    lib.thip_debug_layout.argtypes = [vp, P(C.c_longlong), P(C.c_longlong), P(C.c_longlong)]
    lib.thip_debug_layout.restype = C.c_int
    lib.thip_debug_workspace.argtypes = [vp, dp, P(C.c_int)]
    lib.thip_debug_workspace.restype = C.c_int
    # generic QP (thip_qp_*)
    sp, qi, ll = P(OsqpSettings), P(QpInfo), P(C.c_longlong)
    lib.thip_sizeof_qp_info.argtypes = []
    lib.thip_sizeof_qp_info.restype = C.c_int
    lib.thip_qp_create.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip, ip, C.c_int, P(vp)]
    lib.thip_qp_create.restype = C.c_int
    lib.thip_qp_solve.argtypes = [vp, dp, dp, dp, dp, dp, sp, dp, dp, dp, dp, dp, qi]
    lib.thip_qp_solve.restype = C.c_int
    lib.thip_qp_solve_some.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, sp, dp, dp, ip, dp, dp, dp, qi]
    lib.thip_qp_solve_some.restype = C.c_int
    lib.thip_qp_submit.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, sp, dp, dp, ip, dp]
    lib.thip_qp_submit.restype = C.c_int
    lib.thip_qp_collect.argtypes = [vp, dp, dp, qi]
    lib.thip_qp_collect.restype = C.c_int
    lib.thip_qp_stage.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, sp, dp, dp, ip, dp]
    lib.thip_qp_stage.restype = C.c_int
    lib.thip_qp_launch_staged.argtypes = [P(vp), C.c_int]
    lib.thip_qp_launch_staged.restype = C.c_int
    lib.thip_qp_destroy.argtypes = [vp]
    lib.thip_qp_destroy.restype = None
    lib.thip_qp_last_error.argtypes = [vp]
    lib.thip_qp_last_error.restype = C.c_char_p
    lib.thip_qp_factor_nnz.argtypes = [vp]
    lib.thip_qp_factor_nnz.restype = C.c_longlong
    lib.thip_qp_shape.argtypes = [vp, ll]
    lib.thip_qp_shape.restype = C.c_int
    lib.thip_qp_debug_profile.argtypes = [ll, C.c_int]
    lib.thip_qp_debug_profile.restype = C.c_int
    lib.thip_qp_setup.argtypes = [vp, dp, dp, dp, dp, dp, sp, qi]
    lib.thip_qp_setup.restype = C.c_int
    lib.thip_qp_update_vec.argtypes = [vp, dp, dp, dp, qi]
    lib.thip_qp_update_vec.restype = C.c_int
    lib.thip_qp_update_mat.argtypes = [vp, dp, dp, qi]
    lib.thip_qp_update_mat.restype = C.c_int
    lib.thip_qp_warm_start.argtypes = [vp, dp, dp]
    lib.thip_qp_warm_start.restype = C.c_int
    lib.thip_qp_solve_resident.argtypes = [vp, dp, dp, qi]
    lib.thip_qp_solve_resident.restype = C.c_int
    # ops [batch] of QP_OP_* bits; P, q, A, l, u; settings; warm x, y; out x, y, info
    lib.thip_qp_step.argtypes = [vp, ip, dp, dp, dp, dp, dp, sp, dp, dp, dp, dp, qi]
    lib.thip_qp_step.restype = C.c_int
    lib.thip_sizeof_desc.argtypes = []
    lib.thip_sizeof_desc.restype = C.c_int
    lib.thip_sizeof_result.argtypes = []
    lib.thip_sizeof_result.restype = C.c_int
    return lib


def load_hip():
    """Load the in-tree HIP library. Raises if it has not been built: the
    product has no fallback path."""
    global _hip
    if _hip is None:
        # torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's):
        # load it first so the process has one HIP runtime that torch (device
        # memory, streams, torch.distributed) and this library share.  If ours
        # loaded first, torch would see no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not HIP_LIB.exists():
            raise RuntimeError(
                f"{HIP_LIB} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)"
            )
        _hip = _declare(C.CDLL(str(HIP_LIB)))
        if _hip.thip_sizeof_desc() != C.sizeof(ProblemDesc) or _hip.thip_sizeof_result() != C.sizeof(Result):
            raise RuntimeError("thip_problem_desc / thip_result layout mismatch between Python and the HIP library")
        if (_hip.thip_sizeof_check_config() != C.sizeof(CheckConfig)
                or _hip.thip_sizeof_check_result() != C.sizeof(CheckResult)):
            raise RuntimeError("thip_check_config / thip_check_result layout mismatch between Python and the HIP library")
        if _hip.thip_sizeof_term_slot() != C.sizeof(TermSlot):
            raise RuntimeError("thip_term_slot layout mismatch between Python and the HIP library")
        if _hip.thip_sizeof_csets_config() != C.sizeof(CsetsConfig):
            raise RuntimeError("thip_csets_config layout mismatch between Python and the HIP library")
        if _hip.thip_sizeof_ccsets_config() != C.sizeof(CcsetsConfig):
            raise RuntimeError("thip_ccsets_config layout mismatch between Python and the HIP library")
        if _hip.thip_sizeof_qp_info() != C.sizeof(QpInfo):
            raise RuntimeError("thip_qp_info layout mismatch between Python and the HIP library")
    return _hip


def exported_symbols():
    """Function names declared in include/trajopt_hip.h."""
    import re

    hdr = (PKG_DIR.parent / "include" / "trajopt_hip.h").read_text()
    return sorted(set(re.findall(r"\b(thip_[a-z_]+)\s*\(", hdr)))
