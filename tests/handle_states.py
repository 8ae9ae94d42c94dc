"""What every C-ABI handle answers when it is called out of order or with a
missing argument, and that one good upload and run then succeed.

record(lib) walks the seven handles (batch 2: config C at n_steps = 6 for
thip_ctx, thip_eval, thip_terms and thip_check, the spherebot cases of the
collision-set tests, the smallest case of qp_cases) and returns, per handle and
call, [return code, the whole last_error text].  Every refusal returns before a
launch.  tests/golden/make_golden_handle_states.py writes the recording of the
reference build; tests/test_gpu_handle_states.py compares the build under test
with it, so the two cannot drift apart.
"""
import ctypes as C

import numpy as np

import qp_cases
from test_gpu_ifopt_ccsets import spherebot_desc as ccsets_desc
from test_gpu_ifopt_sets import sphere_rec, spherebot_desc as csets_desc
from trajopt_amd import abi, problems

BATCH = 2


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


class _Log:
    """Calls a function of the library and keeps [rc, last_error(handle)] under a name."""

    def __init__(self, lib, last_error):
        self.lib, self.last_error, self.h, self.out = lib, last_error, C.c_void_p(), {}

    def __call__(self, name, fn, *args):
        assert name not in self.out, name
        rc = getattr(self.lib, fn)(self.h, *args)
        self.out[name] = [rc, self.last_error(self.h).decode()]
        return rc


def _device(n):
    import torch

    return torch.zeros(max(n, 1), dtype=torch.float64, device="cuda")


def _config_c():
    wl = problems.make_workload("C", BATCH, n_steps=6)
    assert wl.desc.n_cart > 0 and wl.desc.n_prims > 0 and wl.desc.coll_enabled
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    return wl, f(wl.init), f(wl.targets), f(wl.scene)


def ctx_states(lib):
    wl, x, tgt, scene = _config_c()
    log = _Log(lib, lib.thip_last_error)
    assert lib.thip_create(0, C.byref(wl.desc), BATCH, C.byref(log.h)) == 0, lib.thip_last_error(None)
    d_x, d_tgt, d_scene = _device(x.size), _device(tgt.size), _device(scene.size)
    try:
        err, jac = np.zeros(BATCH * wl.desc.n_cart * 6), np.zeros(BATCH * wl.desc.n_cart * 6 * wl.n_dof)
        rec, cnt = np.zeros(BATCH * 4 * (8 + 2 * wl.n_dof + 1)), np.zeros(BATCH, dtype=np.int32)
        log("run_before_upload", "thip_sqp_run")
        log("download_before_run", "thip_download", _dp(np.zeros_like(x)), None)
        log("linearize_before_upload", "thip_linearize", _dp(x), _dp(err), _dp(jac))
        log("collision_rows_before_upload", "thip_collision_rows", _dp(x), _dp(rec), 4, _ip(cnt))
        log("linearize_null_x", "thip_linearize", None, _dp(err), _dp(jac))
        log("linearize_null_results", "thip_linearize", _dp(x), None, None)
        log("upload_null_scene", "thip_upload", _dp(x), _dp(tgt), None)
        log("upload_device_null_scene", "thip_upload_device", d_x.data_ptr(), d_tgt.data_ptr(), None)
        log("upload_null_cart_targets", "thip_upload", _dp(x), None, _dp(scene))
        log("upload_device_null_cart_targets", "thip_upload_device", d_x.data_ptr(), None, d_scene.data_ptr())
        log("upload_null_x", "thip_upload", None, _dp(tgt), _dp(scene))
        log("upload_device_null_x", "thip_upload_device", None, d_tgt.data_ptr(), d_scene.data_ptr())
        log("good_upload", "thip_upload", _dp(x), _dp(tgt), _dp(scene))
        log("good_run", "thip_sqp_run")
        log("good_synchronize", "thip_synchronize")
        log.out["last_ms_ok"] = bool(lib.thip_last_kernel_ms(log.h) >= 0)
    finally:
        lib.thip_destroy(log.h)
    return log.out


def eval_states(lib):
    wl, x, tgt, scene = _config_c()
    d = wl.desc
    log = _Log(lib, lib.thip_eval_last_error)
    assert lib.thip_eval_create(0, C.byref(d), BATCH, C.byref(log.h)) == 0, lib.thip_eval_last_error(None)
    try:
        q = np.ascontiguousarray(x[:, 0])
        err, jac = np.zeros(BATCH * d.n_cart * 6), np.zeros(BATCH * d.n_cart * 6 * wl.n_dof)
        cap = 64
        rec, cnt = np.zeros(BATCH * cap * (8 + 2 * wl.n_dof + 1)), np.zeros(BATCH, dtype=np.int32)
        log("cart_pose_before_upload", "thip_eval_cart_pose", 0, _dp(q), _dp(err), _dp(jac))
        log("cart_pose_all_before_upload", "thip_eval_cart_pose_all", _dp(x), _dp(err), _dp(jac))
        log("collision_before_upload", "thip_eval_collision", 0, _dp(x), _dp(rec), cap, _ip(cnt))
        log("cart_pose_null_x", "thip_eval_cart_pose", 0, None, _dp(err), _dp(jac))
        log("cart_pose_all_null_x", "thip_eval_cart_pose_all", None, _dp(err), _dp(jac))
        log("cart_vel_all_null_x", "thip_eval_cart_vel_all", None, _dp(err), _dp(jac))
        log("collision_null_x", "thip_eval_collision", 0, None, _dp(rec), cap, _ip(cnt))
        log("cart_pose_null_results", "thip_eval_cart_pose", 0, _dp(q), None, None)
        log("cart_pose_all_null_results", "thip_eval_cart_pose_all", _dp(x), None, None)
        log("cart_vel_all_null_results", "thip_eval_cart_vel_all", _dp(x), None, None)
        log("collision_null_results", "thip_eval_collision", 0, _dp(x), None, cap, None)
        log("upload_null_scene", "thip_eval_upload", _dp(tgt), None)
        log("upload_null_cart_targets", "thip_eval_upload", None, _dp(scene))
        log("cart_pose_term_below_range", "thip_eval_cart_pose", -1, _dp(q), _dp(err), _dp(jac))
        log("cart_pose_term_out_of_range", "thip_eval_cart_pose", d.n_cart, _dp(q), _dp(err), _dp(jac))
        log("collision_term_below_range", "thip_eval_collision", -1, _dp(x), _dp(rec), cap, _ip(cnt))
        log("collision_term_out_of_range", "thip_eval_collision", 1 + d.n_coll_extra, _dp(x), _dp(rec), cap, _ip(cnt))
        log("good_upload", "thip_eval_upload", _dp(tgt), _dp(scene))
        log("good_cart_pose", "thip_eval_cart_pose", 0, _dp(q), _dp(err), _dp(jac))
        log("good_cart_pose_all", "thip_eval_cart_pose_all", _dp(x), _dp(err), _dp(jac))
        log("good_collision", "thip_eval_collision", 0, _dp(x), _dp(rec), cap, _ip(cnt))
    finally:
        lib.thip_eval_destroy(log.h)
    return log.out


def terms_states(lib):
    wl, x, tgt, scene = _config_c()
    log = _Log(lib, lib.thip_terms_last_error)
    assert lib.thip_terms_create(0, C.byref(wl.desc), BATCH, C.byref(log.h)) == 0, lib.thip_terms_last_error(None)
    d_x, d_tgt, d_scene = _device(x.size), _device(tgt.size), _device(scene.size)
    try:
        nc, nv = C.c_int(), C.c_int()
        assert lib.thip_terms_counts(log.h, C.byref(nc), C.byref(nv)) == 0 and nc.value > 0
        costs, viols = np.zeros(BATCH * max(nc.value, 1)), np.zeros(BATCH * max(nv.value, 1))
        log("run_before_upload", "thip_terms_run", _dp(x), _dp(costs), _dp(viols))
        log("run_device_before_upload", "thip_terms_run_device", d_x.data_ptr(), _dp(costs), _dp(viols))
        log("run_null_x", "thip_terms_run", None, _dp(costs), _dp(viols))
        log("run_device_null_x", "thip_terms_run_device", None, _dp(costs), _dp(viols))
        log("run_null_results", "thip_terms_run", _dp(x), None, None)
        log("run_device_null_results", "thip_terms_run_device", d_x.data_ptr(), None, None)
        log("upload_null_scene", "thip_terms_upload", _dp(tgt), None)
        log("upload_device_null_scene", "thip_terms_upload_device", d_tgt.data_ptr(), None)
        log("upload_null_cart_targets", "thip_terms_upload", None, _dp(scene))
        log("upload_device_null_cart_targets", "thip_terms_upload_device", None, d_scene.data_ptr())
        log("upload_joint_targets_null", "thip_terms_upload_joint_targets", None)
        log("upload_joint_targets_device_null", "thip_terms_upload_joint_targets_device", None)
        log("good_upload", "thip_terms_upload", _dp(tgt), _dp(scene))
        log("good_run", "thip_terms_run", _dp(x), _dp(costs), _dp(viols))
        log.out["last_ms_ok"] = bool(lib.thip_terms_last_ms(log.h) >= 0)
    finally:
        lib.thip_terms_destroy(log.h)
    return log.out


def check_states(lib):
    wl, x, _, scene = _config_c()
    cfg = abi.CheckConfig(abi.CHECK_LVS_CONTINUOUS, 0.05, 0.0, 0, -1)
    log = _Log(lib, lib.thip_check_last_error)
    assert lib.thip_check_create(0, C.byref(wl.desc), C.byref(cfg), BATCH, C.byref(log.h)) == 0, \
        lib.thip_check_last_error(None)
    d_x = _device(x.size)
    try:
        res = (abi.CheckResult * BATCH)()
        log("run_before_upload", "thip_check_run", _dp(x), res, None)
        log("run_device_before_upload", "thip_check_run_device", d_x.data_ptr(), res, None)
        log("run_null_x", "thip_check_run", None, res, None)
        log("run_device_null_x", "thip_check_run_device", None, res, None)
        log("run_null_results", "thip_check_run", _dp(x), None, None)
        log("run_device_null_results", "thip_check_run_device", d_x.data_ptr(), None, None)
        log("upload_null_scene", "thip_check_upload", None)
        log("upload_device_null_scene", "thip_check_upload_device", None)
        log("good_upload", "thip_check_upload", _dp(scene))
        log("good_run", "thip_check_run", _dp(x), res, None)
        log.out["last_ms_ok"] = bool(lib.thip_check_last_ms(log.h) >= 0)
    finally:
        lib.thip_check_destroy(log.h)
    return log.out


def _sets_states(lib, api, create, n_steps, jac_width):
    """thip_csets / thip_ccsets on the spherebot: one sphere primitive at the origin."""
    scene = np.ascontiguousarray(np.stack([sphere_rec((0.0, 0.0, 0.0), 0.5)[None]] * BATCH))
    x = np.ascontiguousarray(np.tile(np.array([-1.0, 0.0]), (BATCH, n_steps, 1)))
    x[:, 0, 0] = -1.9 if n_steps > 1 else -1.0  # the continuous sets' segment has a length
    log = _Log(lib, getattr(lib, api + "_last_error"))
    assert create(log.h) == 0, getattr(lib, api + "_last_error")(None)
    d_x = _device(x.size)
    try:
        items = BATCH * (n_steps if api == "thip_csets" else n_steps - 1)
        values, jac, coeffs = np.zeros(items), np.zeros(items * jac_width), np.zeros(items)
        counts, keys = np.zeros(items, dtype=np.int32), np.zeros(items * 4, dtype=np.int32)
        outs = (_dp(values), _dp(jac), _dp(coeffs), _ip(counts), _ip(keys))
        log("run_before_upload", api + "_run", _dp(x), *outs)
        log("run_device_before_upload", api + "_run_device", d_x.data_ptr(), *outs)
        log("run_null_x", api + "_run", None, *outs)
        log("run_device_null_x", api + "_run_device", None, *outs)
        log("run_null_results", api + "_run", _dp(x), None, None, None, None, None)
        log("run_device_null_results", api + "_run_device", d_x.data_ptr(), None, None, None, None, None)
        log("upload_null_scene", api + "_upload", None)
        log("upload_device_null_scene", api + "_upload_device", None)
        log("good_upload", api + "_upload", _dp(scene))
        log("good_run", api + "_run", _dp(x), *outs)
        log.out["last_ms_ok"] = bool(getattr(lib, api + "_last_ms")(log.h) >= 0)
    finally:
        getattr(lib, api + "_destroy")(log.h)
    return log.out


def csets_states(lib):
    d, cfg = csets_desc(), abi.CsetsConfig(0.1, 1.0, 0.01, 1, 0, 0)
    return _sets_states(lib, "thip_csets",
                        lambda h: lib.thip_csets_create(0, C.byref(d), C.byref(cfg), BATCH, C.byref(h)), 1, 2)


def ccsets_states(lib):
    d = ccsets_desc()
    cfg = abi.CcsetsConfig(0.1, 1.0, 0.01, 1, 0, 1, abi.EVALUATOR_LVS_CONTINUOUS, 0.5)
    return _sets_states(lib, "thip_ccsets",
                        lambda h: lib.thip_ccsets_create(0, C.byref(d), C.byref(cfg), None, BATCH, C.byref(h)), 2, 4)


def qp_states(lib):
    case = qp_cases.CASES["n1m1"]
    assert (case.n, case.m) == min((c.n, c.m) for c in qp_cases.CASES.values())
    pat = [np.ascontiguousarray(v, dtype=np.int32) for v in (case.P.indptr, case.P.indices, case.A.indptr, case.A.indices)]
    log = _Log(lib, lib.thip_qp_last_error)
    assert lib.thip_qp_create(0, case.n, case.m, *[_ip(v) for v in pat], BATCH, C.byref(log.h)) == 0, \
        lib.thip_qp_last_error(None)
    try:
        rep = lambda v: np.ascontiguousarray(np.tile(np.asarray(v, dtype=np.float64), BATCH))  # noqa: E731
        Pv, q, Av, lo, up = rep(case.P.data), rep(case.q), rep(case.A.data), rep(case.l), rep(case.u)
        st = qp_cases.settings_of(case)
        x, y, info = np.zeros(BATCH * case.n), np.zeros(BATCH * case.m), (abi.QpInfo * BATCH)()
        ins = (_dp(Pv), _dp(q), _dp(Av), _dp(lo), _dp(up), C.byref(st), None, None, None)
        log("collect_before_submit", "thip_qp_collect", _dp(x), _dp(y), info)
        log("solve_resident_before_setup", "thip_qp_solve_resident", _dp(x), _dp(y), info)
        log("update_vec_before_setup", "thip_qp_update_vec", _dp(q), None, None, info)
        log("update_mat_before_setup", "thip_qp_update_mat", _dp(Pv), None, info)
        log("warm_start_before_setup", "thip_qp_warm_start", _dp(x), None)
        log("solve_null_q", "thip_qp_solve", _dp(Pv), None, _dp(Av), _dp(lo), _dp(up), C.byref(st), None, None, None,
            _dp(x), _dp(y), info)
        log("solve_null_results", "thip_qp_solve", *ins, None, None, None)
        log("solve_some_count_out_of_range", "thip_qp_solve_some", BATCH + 1, _dp(Pv), _dp(q), _dp(Av), _dp(lo), _dp(up),
            C.byref(st), None, None, None, None, _dp(x), _dp(y), info)
        log("good_solve", "thip_qp_solve", *ins, _dp(x), _dp(y), info)
        log.out["solved"] = [int(i.status) for i in info]
    finally:
        lib.thip_qp_destroy(log.h)
    return log.out


HANDLES = {
    "thip_ctx": ctx_states,
    "thip_eval": eval_states,
    "thip_terms": terms_states,
    "thip_check": check_states,
    "thip_csets": csets_states,
    "thip_ccsets": ccsets_states,
    "thip_qp": qp_states,
}
