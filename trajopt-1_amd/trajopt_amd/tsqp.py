"""ctypes binding of the trajopt_sqp front end (include/trajopt_host.h, tsqp_*).

trajopt's second SQP front end (trajopt_optimizers/trajopt_sqp: TrustRegionSQPSolver
over a TrajOptQPProblem of trajopt_ifopt constraint sets)
keeps one QP sparsity pattern for the whole solve and updates it in place; here
the QP lives in thip_qp's resident GPU workspace (trajopt_sqp::GpuQPSolver).
`Spec` mirrors tsqp_spec: a joint trajectory of n_nodes nodes with joint
position / velocity / acceleration / jerk terms, as constraints or as squared /
absolute / hinge costs.  `solve` runs the C++ product path on a HIP device.
`solve_batch` runs many problems in lock step on one device
(trajopt_sqp::BatchTrustRegionSQPSolver: one thip_qp_step launch per round and QP
pattern), every problem's result bit for bit the one of its solve alone.
`KinSpec` mirrors tsqp_kin_spec: CartPosConstraint sets and fixed-size
DiscreteCollisionConstraint sets on the built-in environment of a group, their
values and jacobians from the device; `solve_kin` solves with them, `eval_kin`
returns every set's values, jacobian, coefficients and bounds without a solve.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi, host

MAX_NODES = 64
MAX_TERMS = 16
JOINT_POS, JOINT_VEL, JOINT_ACC, JOINT_JERK = 0, 1, 2, 3
CONSTRAINT, SQUARED, ABSOLUTE, HINGE = 0, 1, 2, 3
STATUS = {0: "SQP_RUNNING", 1: "SQP_CONVERGED", 2: "SQP_ITERATION_LIMIT", 3: "SQP_PENALTY_ITERATION_LIMIT",
          4: "SQP_TIME_LIMIT", 5: "SQP_FAILED", 6: "SQP_STOPPED_BY_CALLBACK"}
D_MAX = abi.MAX_DOF


class Term(C.Structure):
    _fields_ = [("kind", C.c_int), ("penalty", C.c_int), ("first", C.c_int), ("last", C.c_int),
                ("n_coeffs", C.c_int), ("coeffs", C.c_double * D_MAX), ("lower", C.c_double * D_MAX),
                ("upper", C.c_double * D_MAX)]


class Spec(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("n_dof", C.c_int), ("init", C.c_double * (MAX_NODES * D_MAX)),
                ("var_lower", C.c_double * D_MAX), ("var_upper", C.c_double * D_MAX), ("n_terms", C.c_int),
                ("terms", Term * MAX_TERMS),
                ("improve_ratio_threshold", C.c_double), ("min_trust_box_size", C.c_double),
                ("min_approx_improve", C.c_double), ("min_approx_improve_frac", C.c_double),
                ("max_iterations", C.c_int), ("trust_shrink_ratio", C.c_double), ("trust_expand_ratio", C.c_double),
                ("cnt_tolerance", C.c_double), ("max_merit_coeff_increases", C.c_double),
                ("max_qp_solver_failures", C.c_int), ("merit_coeff_increase_ratio", C.c_double),
                ("max_time", C.c_double), ("initial_merit_error_coeff", C.c_double),
                ("inflate_constraints_individually", C.c_int), ("initial_trust_box_size", C.c_double),
                ("osqp", abi.OsqpSettings)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int), ("overall_iteration", C.c_int), ("penalty_iteration", C.c_int),
                ("qp_setups", C.c_int), ("qp_updates", C.c_int), ("qp_solves", C.c_int),
                ("admm_iters", C.c_longlong), ("best_exact_merit", C.c_double)]


KIN_MAX_CART, KIN_MAX_COLL, KIN_MAX_PRIMS, KIN_NAME_LEN = 16, 4, 32, 64
IDENTITY12 = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


class CartTerm(C.Structure):
    _fields_ = [("node", C.c_int), ("penalty", C.c_int), ("analytic_jacobian", C.c_int), ("pad_", C.c_int),
                ("source_frame", C.c_char * KIN_NAME_LEN),
                ("target_frame", C.c_char * KIN_NAME_LEN), ("source_offset", C.c_double * 12),
                ("target_offset", C.c_double * 12), ("coeffs", C.c_double * 6), ("lower", C.c_double * 6),
                ("upper", C.c_double * 6)]


class CollTerm(C.Structure):
    _fields_ = [("first", C.c_int), ("last", C.c_int), ("penalty", C.c_int), ("max_num_cnt", C.c_int),
                ("fixed_sparsity", C.c_int), ("margin", C.c_double), ("coeff", C.c_double), ("buffer", C.c_double)]


class CcollTerm(C.Structure):
    """tsqp_ccoll_term: one ContinuousCollisionConstraint per segment of first..last."""
    _fields_ = [("first", C.c_int), ("last", C.c_int), ("penalty", C.c_int), ("max_num_cnt", C.c_int),
                ("fixed_sparsity", C.c_int), ("evaluator_type", C.c_int), ("fixed_first", C.c_int),
                ("fixed_last", C.c_int), ("margin", C.c_double), ("coeff", C.c_double), ("buffer", C.c_double),
                ("lvs_length", C.c_double)]


class KinSpec(C.Structure):
    _fields_ = [("manip", C.c_char * KIN_NAME_LEN), ("n_prims", C.c_int),
                ("prims", (C.c_double * 16) * KIN_MAX_PRIMS), ("n_cart", C.c_int), ("cart", CartTerm * KIN_MAX_CART),
                ("n_coll", C.c_int), ("coll", CollTerm * KIN_MAX_COLL),
                ("n_ccoll", C.c_int), ("ccoll", CcollTerm * KIN_MAX_COLL)]


class BatchStats(C.Structure):
    """tsqp_batch_stats: rendezvous rounds, thip_qp_step launches, thip_qp objects created (one symbolic analysis
    each), the largest of them, and the launches of the problems' CartPos / collision evaluators."""
    _fields_ = [("rounds", C.c_longlong), ("step_launches", C.c_longlong), ("groups", C.c_longlong),
                ("max_group", C.c_longlong), ("set_launches", C.c_longlong * 2)]


def _lib():
    L = host.load_host()
    if not hasattr(L, "_tsqp_ready"):
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        L.thost_tsqp_solve_batch.argtypes = [C.POINTER(Spec), C.POINTER(KinSpec), C.c_int, C.c_int, dp,
                                             C.POINTER(Result), ip, C.POINTER(BatchStats), C.c_char_p, C.c_int]
        L.thost_tsqp_solve_batch.restype = C.c_int
        L.thost_tsqp_sizeof_batch_stats.restype = C.c_int
        if L.thost_tsqp_sizeof_batch_stats() != C.sizeof(BatchStats):
            raise RuntimeError("tsqp_batch_stats layout mismatch between Python and the host library")
        L.thost_tsqp_solve_kin.argtypes = [C.POINTER(Spec), C.POINTER(KinSpec), C.c_int, dp, C.POINTER(Result),
                                           C.c_char_p, C.c_int]
        L.thost_tsqp_solve_kin.restype = C.c_int
        L.thost_tsqp_eval_kin.argtypes = [C.POINTER(Spec), C.POINTER(KinSpec), C.c_int, dp, C.c_int, ip, ip, C.c_int,
                                          dp, dp, dp, dp, dp, C.c_int, dp, dp, C.POINTER(C.c_longlong), C.c_char_p,
                                          C.c_int]
        L.thost_tsqp_eval_kin.restype = C.c_int
        for fn, st in (("thost_tsqp_sizeof_kin_spec", KinSpec), ("thost_tsqp_sizeof_cart_term", CartTerm),
                       ("thost_tsqp_sizeof_coll_term", CollTerm), ("thost_tsqp_sizeof_ccoll_term", CcollTerm)):
            getattr(L, fn).restype = C.c_int
            if getattr(L, fn)() != C.sizeof(st):
                raise RuntimeError(f"{st.__name__} layout mismatch between Python and the host library")
        L.thost_tsqp_defaults.argtypes = [C.POINTER(Spec)]
        L.thost_tsqp_defaults.restype = None
        L.thost_tsqp_solve.argtypes = [C.POINTER(Spec), C.c_int, C.POINTER(C.c_double), C.POINTER(Result),
                                       C.c_char_p, C.c_int]
        L.thost_tsqp_solve.restype = C.c_int
        L.thost_tsqp_sizeof_spec.restype = C.c_int
        L.thost_tsqp_sizeof_result.restype = C.c_int
        if L.thost_tsqp_sizeof_spec() != C.sizeof(Spec) or L.thost_tsqp_sizeof_result() != C.sizeof(Result):
            raise RuntimeError("tsqp_spec / tsqp_result layout mismatch between Python and the host library")
        L._tsqp_ready = True
    return L


def make_spec(init, terms, var_lower=None, var_upper=None, **params):
    """init [n_nodes, n_dof]; terms: dicts with kind, penalty, first, last (default
    first), coeffs (list), lower, upper (per-dof lists); params: SQPParameters /
    `osqp` (dict of thip_osqp_settings fields) overrides.  SQPParameters and OSQP
    settings default to the reference's (types.h, OSQPEigenSolver::setDefaultOSQPSettings)."""
    init = np.asarray(init, dtype=np.float64)
    n, d = init.shape
    if n > MAX_NODES or d > D_MAX or len(terms) > MAX_TERMS:
        raise ValueError("spec exceeds TSQP_MAX_NODES / THIP_MAX_DOF / TSQP_MAX_TERMS")
    s = Spec()
    _lib().thost_tsqp_defaults(C.byref(s))
    s.n_nodes, s.n_dof = n, d
    for i, v in enumerate(init.reshape(-1)):
        s.init[i] = float(v)
    for k in range(d):
        s.var_lower[k] = -np.inf if var_lower is None else float(var_lower[k])
        s.var_upper[k] = np.inf if var_upper is None else float(var_upper[k])
    s.n_terms = len(terms)
    for i, t in enumerate(terms):
        T = s.terms[i]
        T.kind, T.penalty = int(t["kind"]), int(t.get("penalty", CONSTRAINT))
        T.first = int(t.get("first", 0))
        T.last = int(t.get("last", T.first))
        co = list(t.get("coeffs", []))
        T.n_coeffs = len(co)
        for k, v in enumerate(co):
            T.coeffs[k] = float(v)
        lo = list(t.get("lower", [0.0] * d))
        up = list(t.get("upper", lo))
        for k in range(d):
            T.lower[k] = float(lo[k])
            T.upper[k] = float(up[k])
    osqp = params.pop("osqp", {})
    for k, v in params.items():
        if not hasattr(s, k):
            raise KeyError(k)
        setattr(s, k, v)
    for k, v in osqp.items():
        if not hasattr(s.osqp, k):
            raise KeyError(k)
        setattr(s.osqp, k, v)
    return s


def solve(spec: Spec, device: int = 0):
    """-> (x [n_nodes, n_dof], Result) through trajopt_sqp::TrustRegionSQPSolver with
    trajopt_sqp::GpuQPSolver on HIP device `device`."""
    L = _lib()
    x = np.zeros((spec.n_nodes, spec.n_dof))
    res = Result()
    err = C.create_string_buffer(4096)
    rc = L.thost_tsqp_solve(C.byref(spec), device, x.ctypes.data_as(C.POINTER(C.c_double)), C.byref(res), err, 4096)
    if rc != 0:
        raise host.HostError(err.value.decode())
    return x, res


def solve_batch(specs, kins=None, device: int = 0):
    """-> (list of x [n_nodes, n_dof], list of Result, qp_rounds [batch], BatchStats): the problems of `specs` (with
    the kinematic sets of `kins`, one per spec, when given) in lock step on HIP device `device`
    (thost_tsqp_solve_batch).  Problem b's x and Result are those of solve(specs[b]) / solve_kin(specs[b], kins[b])
    alone, bit for bit; qp_rounds[b] counts the rounds it took part in.  Raises HostError naming every problem that
    failed."""
    L = _lib()
    B = len(specs)
    if kins is not None and len(kins) != B:
        raise ValueError("solve_batch: one KinSpec per Spec")
    sa = (Spec * max(B, 1))(*specs)
    ka = None if kins is None else (KinSpec * max(B, 1))(*kins)
    stride = MAX_NODES * D_MAX
    x = np.zeros((max(B, 1), stride))
    res = (Result * max(B, 1))()
    rounds = np.zeros(max(B, 1), dtype=np.int32)
    stats = BatchStats()
    err = C.create_string_buffer(16384)
    rc = L.thost_tsqp_solve_batch(sa, ka, B, device, x.ctypes.data_as(C.POINTER(C.c_double)), res,
                                  rounds.ctypes.data_as(C.POINTER(C.c_int)), C.byref(stats), err, 16384)
    if rc != 0:
        raise host.HostError(err.value.decode())
    xs = [x[b, :specs[b].n_nodes * specs[b].n_dof].reshape(specs[b].n_nodes, specs[b].n_dof).copy() for b in range(B)]
    return xs, [res[b] for b in range(B)], rounds[:B].copy(), stats


def make_kin_spec(manip, cart=(), coll=(), prims=None, ccoll=()):
    """manip: a group of the built-in environments ("right_arm", "left_arm",
    "both_arms", spherebot's "manipulator").  cart: dicts with node, source_frame,
    target_frame, source_offset / target_offset (12 values, default identity),
    coeffs (6, default ones), lower / upper (6, default zeros: BoundZero), penalty,
    analytic_jacobian (use_numeric_differentiation = false: refused).
    coll: dicts with first, last (default first), margin, coeff, buffer,
    max_num_cnt, fixed_sparsity, penalty.  prims [n, 16]: scene primitives added
    to the environment's own.  ccoll: dicts as coll's over the segments of first..last
    (last > first), plus evaluator_type (tesseract's CollisionEvaluatorType value,
    default 4 LVS_CONTINUOUS), lvs_length (default 0.005), fixed_first, fixed_last."""
    if len(cart) > KIN_MAX_CART or len(coll) > KIN_MAX_COLL or len(ccoll) > KIN_MAX_COLL:
        raise ValueError("kinematic spec exceeds TSQP_KIN_MAX_CART / TSQP_KIN_MAX_COLL")
    k = KinSpec()
    k.manip = manip.encode()
    prims = np.zeros((0, 16)) if prims is None else np.asarray(prims, dtype=np.float64).reshape(-1, 16)
    if len(prims) > KIN_MAX_PRIMS:
        raise ValueError("kinematic spec exceeds TSQP_KIN_MAX_PRIMS")
    k.n_prims = len(prims)
    for p, rec in enumerate(prims):
        for i in range(16):
            k.prims[p][i] = float(rec[i])
    k.n_cart = len(cart)
    for i, t in enumerate(cart):
        T = k.cart[i]
        T.node, T.penalty = int(t.get("node", 0)), int(t.get("penalty", CONSTRAINT))
        T.analytic_jacobian = int(bool(t.get("analytic_jacobian", False)))
        T.source_frame, T.target_frame = t["source_frame"].encode(), t["target_frame"].encode()
        so = np.asarray(t.get("source_offset", IDENTITY12), dtype=np.float64).reshape(12)
        to = np.asarray(t.get("target_offset", IDENTITY12), dtype=np.float64).reshape(12)
        co, lo = list(t.get("coeffs", [1.0] * 6)), list(t.get("lower", [0.0] * 6))
        up = list(t.get("upper", lo))
        if len(co) != 6 or len(lo) != 6 or len(up) != 6:
            raise ValueError("a CartPos term takes 6 coefficients and 6 bounds")
        for j in range(12):
            T.source_offset[j], T.target_offset[j] = float(so[j]), float(to[j])
        for j in range(6):
            T.coeffs[j], T.lower[j], T.upper[j] = float(co[j]), float(lo[j]), float(up[j])
    k.n_coll = len(coll)
    for i, t in enumerate(coll):
        T = k.coll[i]
        T.first = int(t.get("first", 0))
        T.last = int(t.get("last", T.first))
        T.penalty = int(t.get("penalty", CONSTRAINT))
        T.max_num_cnt, T.fixed_sparsity = int(t.get("max_num_cnt", 3)), int(bool(t.get("fixed_sparsity", True)))
        T.margin, T.coeff, T.buffer = float(t["margin"]), float(t.get("coeff", 1.0)), float(t.get("buffer", 0.01))
    k.n_ccoll = len(ccoll)
    for i, t in enumerate(ccoll):
        T = k.ccoll[i]
        T.first = int(t.get("first", 0))
        T.last = int(t.get("last", T.first + 1))
        T.penalty = int(t.get("penalty", CONSTRAINT))
        T.max_num_cnt, T.fixed_sparsity = int(t.get("max_num_cnt", 3)), int(bool(t.get("fixed_sparsity", True)))
        T.evaluator_type = int(t.get("evaluator_type", 4))
        T.fixed_first, T.fixed_last = int(bool(t.get("fixed_first", False))), int(bool(t.get("fixed_last", False)))
        T.margin, T.coeff, T.buffer = float(t["margin"]), float(t.get("coeff", 1.0)), float(t.get("buffer", 0.01))
        T.lvs_length = float(t.get("lvs_length", 0.005))
    return k


def solve_kin(spec: Spec, kin: KinSpec, device: int = 0):
    """solve() with the kinematic sets of `kin` added (thost_tsqp_solve_kin)."""
    L = _lib()
    x = np.zeros((spec.n_nodes, spec.n_dof))
    res = Result()
    err = C.create_string_buffer(4096)
    if L.thost_tsqp_solve_kin(C.byref(spec), C.byref(kin), device, x.ctypes.data_as(C.POINTER(C.c_double)),
                              C.byref(res), err, 4096) != 0:
        raise host.HostError(err.value.decode())
    return x, res


def eval_kin(spec: Spec, kin: KinSpec, xs, probe_q=None, device: int = 0, cap_sets=256, cap_rows=2048):
    """Every set of (spec, kin) at each variable vector of xs [n_x, n_nodes, n_dof],
    without a solve (thost_tsqp_eval_kin) -> dict: set_rows [n_sets]; values,
    coeffs [n_x, rows]; jac [n_x, rows, n_nodes * n_dof]; lower, upper [rows];
    launches (CartPos evaluator, collision evaluators); probe [rows] with every
    CartPos set's calcValues(probe_q) in its rows (NaN elsewhere) when probe_q is given."""
    L = _lib()
    dp = C.POINTER(C.c_double)
    xs = np.ascontiguousarray(xs, dtype=np.float64).reshape(-1, spec.n_nodes, spec.n_dof)
    n_x, nv = len(xs), spec.n_nodes * spec.n_dof
    n_sets = C.c_int(0)
    set_rows = np.zeros(cap_sets, dtype=np.int32)
    values, coeffs = np.zeros((n_x, cap_rows)), np.zeros((n_x, cap_rows))
    jac = np.zeros((n_x, cap_rows, nv))
    lower, upper = np.zeros(cap_rows), np.zeros(cap_rows)
    probe = np.full(cap_rows, np.nan)
    pq = None if probe_q is None else np.ascontiguousarray(probe_q, dtype=np.float64)
    launches = (C.c_longlong * 2)()
    err = C.create_string_buffer(4096)
    d = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    rc = L.thost_tsqp_eval_kin(C.byref(spec), C.byref(kin), device, d(xs), n_x, C.byref(n_sets),
                               set_rows.ctypes.data_as(C.POINTER(C.c_int)), cap_sets, d(values), d(jac), d(coeffs),
                               d(lower), d(upper), cap_rows, None if pq is None else d(pq), d(probe), launches, err,
                               4096)
    if rc != 0:
        raise host.HostError(err.value.decode())
    rows = int(set_rows[:n_sets.value].sum())
    return {"set_rows": set_rows[:n_sets.value].copy(), "values": values[:, :rows], "coeffs": coeffs[:, :rows],
            "jac": jac[:, :rows], "lower": lower[:rows], "upper": upper[:rows], "probe": probe[:rows],
            "launches": (int(launches[0]), int(launches[1]))}
