"""BatchTrustRegionSQP over the C-ABI (the batched tier of SURVEY.md §8b).

Lowers a Workload (one shared thip_problem_desc + per-problem arrays) onto one
HIP device and runs sco::BasicTrustRegionSQP::optimize for every problem in
one fused launch.  No CPU fallback: every method raises if the HIP library or
the device call fails.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class HipError(RuntimeError):
    pass


class BatchTrustRegionSQP:
    def __init__(self, workload, device: int = 0, stream=None):
        self.lib = abi.load_hip()
        self.wl = workload
        self.batch = workload.batch
        self.ctx = C.c_void_p()
        self._device = device
        rc = self.lib.thip_create(device, C.byref(workload.desc), self.batch, C.byref(self.ctx))
        if rc != 0:
            raise HipError(f"thip_create: {self.lib.thip_last_error(None).decode()}")
        if stream is not None:
            self._check(self.lib.thip_set_stream(self.ctx, C.c_void_p(stream)), "thip_set_stream")
        self.uploaded = False

    def _check(self, rc, what):
        if rc != 0:
            raise HipError(f"{what}: {self.lib.thip_last_error(self.ctx).decode()}")

    def upload(self):
        wl = self.wl
        self._init = np.ascontiguousarray(wl.init, dtype=np.float64)
        self._tgt = np.ascontiguousarray(wl.targets, dtype=np.float64) if wl.targets.size else None
        self._scene = np.ascontiguousarray(wl.scene, dtype=np.float64) if wl.scene.size else None
        self._check(
            self.lib.thip_upload(self.ctx, _dp(self._init), _dp(self._tgt) if self._tgt is not None else None,
                                 _dp(self._scene) if self._scene is not None else None),
            "thip_upload",
        )
        jt = getattr(wl, "jpos_targets", None)
        if jt is not None:
            self._jpt = np.ascontiguousarray(jt, dtype=np.float64)
            self._check(self.lib.thip_upload_joint_targets(self.ctx, _dp(self._jpt)), "thip_upload_joint_targets")
        self.uploaded = True

    def run(self):
        if not self.uploaded:
            self.upload()
        self._check(self.lib.thip_sqp_run(self.ctx), "thip_sqp_run")

    def sync(self):
        self._check(self.lib.thip_synchronize(self.ctx), "thip_synchronize")

    def kernel_ms(self) -> float:
        return float(self.lib.thip_last_kernel_ms(self.ctx))

    def download(self):
        x = np.zeros((self.batch, self.wl.n_steps, self.wl.n_dof))
        res = (abi.Result * self.batch)()
        self._check(self.lib.thip_download(self.ctx, _dp(x), res), "thip_download")
        return x, list(res)

    def optimize(self):
        self.run()
        return self.download()

    def linearize(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        D = self.wl.n_dof
        n_cart = self.wl.desc.n_cart
        err = np.zeros((self.batch, n_cart, 6))
        jac = np.zeros((self.batch, n_cart, 6, D))
        if not self.uploaded:
            self.upload()
        self._check(self.lib.thip_linearize(self.ctx, _dp(x), _dp(err), _dp(jac)), "thip_linearize")
        return err, jac

    def fwd_kin(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        n_links = self.wl.desc.chain.n_links
        poses = np.zeros((self.batch, self.wl.n_steps, n_links, 12))
        self._check(self.lib.thip_fwd_kin(self.ctx, _dp(x), _dp(poses)), "thip_fwd_kin")
        return poses

    def collision_rows(self, x, cap=4096):
        """Linearised collision rows at trajectories x [B, N, D] (list of
        [n, 8 + 2 D + 1] arrays, one per problem; see thip_collision_rows)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if not self.uploaded:
            self.upload()
        W = 8 + 2 * self.wl.n_dof + 1
        rec = np.zeros((self.batch, cap, W))
        cnt = (C.c_int * self.batch)()
        self._check(self.lib.thip_collision_rows(self.ctx, _dp(x), _dp(rec), cap, cnt), "thip_collision_rows")
        out = []
        for b in range(self.batch):
            if cnt[b] < 0:
                raise HipError(f"problem {b}: contact overflow")
            out.append(rec[b, : min(cnt[b], cap)])
        return out

    def check(self, config=None, unit_min=False):
        """checkTrajectory on the last solve's trajectories where they lie on the
        device (thip_device_x): list of abi.CheckResult, one per problem (and the
        per-unit clearance [B, n_units] with unit_min)."""
        self.sync()
        chk = TrajectoryChecker(self.wl.desc, self.batch, self.wl.scene, config, device=self._device)
        try:
            return chk.run_device(self.lib.thip_device_x(self.ctx), unit_min=unit_min)
        finally:
            chk.close()

    def term_values(self):
        """The value of every cost and the violation of every constraint at the last
        solve's trajectories where they lie on the device (thip_device_x): costs
        [B, n_costs], viols [B, n_cnts] (OptResults::cost_vals / cnt_viols in slot
        order; TermValues.slots names the slots).  Explicit: no other method
        evaluates terms."""
        self.sync()
        tv = TermValues(self.wl, device=self._device)
        try:
            return tv.run_device(self.lib.thip_device_x(self.ctx))
        finally:
            tv.close()

    def debug_values(self):
        """Diagnostic: the solver's own A_COST / A_VIOL [B, n_costs] / [B, n_cnts] and the
        contact counts I_PCNT [B, N] read from the workspace (thip_debug_layout +
        thip_debug_workspace).  They belong to the returned trajectories only under
        abi.DEBUG_STATIC_DISPATCH, where every problem keeps its workspace."""
        doff = (C.c_longlong * 256)()
        ioff = (C.c_longlong * 256)()
        dims = (C.c_longlong * 12)()
        self._check(self.lib.thip_debug_layout(self.ctx, doff, ioff, dims), "thip_debug_layout")
        dstride, istride = int(dims[8]), int(dims[9])
        dws = np.zeros((self.batch, dstride))
        iws = np.zeros((self.batch, istride), dtype=np.int32)
        self._check(self.lib.thip_debug_workspace(self.ctx, _dp(dws), iws.ctypes.data_as(C.POINTER(C.c_int))),
                    "thip_debug_workspace")
        return dws, iws, list(doff), list(ioff)

    def enable_trace(self, capacity=512):
        self._trace_cap = capacity
        self._check(self.lib.thip_debug_trace(self.ctx, capacity), "thip_debug_trace")

    def get_trace(self):
        rec = np.zeros((self.batch, self._trace_cap, abi.TRACE_W))
        cnt = (C.c_int * self.batch)()
        self._check(self.lib.thip_debug_get_trace(self.ctx, _dp(rec), cnt), "thip_debug_get_trace")
        return [rec[b, : cnt[b]] for b in range(self.batch)]

    PROFILE_SLOTS = ["admm_step", "residuals", "termination", "factor", "polish", "linearize", "evaluate",
                     "build_and_scale", "solve_rhs_diag", "fwd_chain", "bwd_chain", "aux_backsub", "qp_solve",
                     "sqp_total", "sqp_wall_ticks", "seg_B_rhs_linv", "fwd_wave0_own",
                     "seg_hinge_gather", "seg_hinge_E", "coll_count_pass", "coll_rank_pass", "coll_rows", "coll_fk_substates",
                     "gen_rhs_mr", "gen_rhs_cols", "gen_rhs_linv", "gen_dvalue_middle",
                     "n_primal_inf_full", "n_dual_inf_full", "n_factor", "gen_pre", "gen_updates",
                     "factor_blocks", "factor_twisted", "bwd_wave0_own", "gen_dvalue", "gen_middle_wait", "seg_setup", "seg_writeback",
                     "n_seg_entries", "sqp_fingerprint", "sqp_model_values", "sqp_decide"]

    def layout(self):
        """The solve layout this context chose (thip_debug_solve_layout): branches, dofs
        per block, wide, segment possible, generic-step build, threads, waypoints per solve
        block (2 with JointAccEqCost terms), solve blocks per branch."""
        out = (C.c_int * 8)()
        self._check(self.lib.thip_debug_solve_layout(self.ctx, out, 8), "thip_debug_solve_layout")
        return dict(zip(("nbr", "block_dofs", "wide", "seg_ok", "gen", "threads", "grp", "blocks"), list(out)))

    def enable_profile(self, on=True):
        self._check(self.lib.thip_debug_profile(self.ctx, 1 if on else 0), "thip_debug_profile")

    def get_profile(self):
        out = np.zeros((self.batch, len(self.PROFILE_SLOTS)), dtype=np.int64)  # csrc/layout.hpp kProfSlots
        self._check(self.lib.thip_debug_get_profile(self.ctx, out.ctypes.data_as(C.POINTER(C.c_longlong))),
                    "thip_debug_get_profile")
        return out

    def close(self):
        if self.ctx:
            self.lib.thip_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TermEvaluator:
    """thip_eval_*: the CartPose and collision terms of a workload's problems
    evaluated on the device (what the host SQP loop calls for problems the
    fused kernel does not lower)."""

    def __init__(self, workload, device: int = 0):
        self.lib = abi.load_hip()
        self.wl = workload
        self.ev = C.c_void_p()
        rc = self.lib.thip_eval_create(device, C.byref(workload.desc), workload.batch, C.byref(self.ev))
        if rc != 0:
            raise HipError(f"thip_eval_create: {self.lib.thip_eval_last_error(None).decode()}")
        self._tgt = np.ascontiguousarray(workload.targets, dtype=np.float64) if workload.targets.size else None
        self._scene = np.ascontiguousarray(workload.scene, dtype=np.float64) if workload.scene.size else None
        self._check(self.lib.thip_eval_upload(self.ev, None if self._tgt is None else _dp(self._tgt),
                                              None if self._scene is None else _dp(self._scene)), "thip_eval_upload")

    def _check(self, rc, what):
        if rc != 0:
            raise HipError(f"{what}: {self.lib.thip_eval_last_error(self.ev).decode()}")

    def cart_pose(self, term, q, jac=True):
        """q [B, D] -> err [B, 6], jac [B, 6, D] (or None)."""
        B, D = self.wl.batch, self.wl.n_dof
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(B, D)
        err = np.zeros((B, 6))
        J = np.zeros((B, 6, D)) if jac else None
        self._check(self.lib.thip_eval_cart_pose(self.ev, term, _dp(q), _dp(err), None if J is None else _dp(J)),
                    "thip_eval_cart_pose")
        return err, J

    def cart_vel(self, x, jac=True):
        """x [B, N, D] -> err [B, P, 6], jac [B, P, 6, 2 D] (or None): every step
        pair of every CartVel term, in term order and then ascending step
        (thip_eval_cart_vel_all)."""
        B, D = self.wl.batch, self.wl.n_dof
        P = self.lib.thip_eval_cart_vel_pairs(self.ev)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(B, self.wl.desc.n_steps, D)
        err = np.zeros((B, P, 6))
        J = np.zeros((B, P, 6, 2 * D)) if jac else None
        self._check(self.lib.thip_eval_cart_vel_all(self.ev, _dp(x), _dp(err), None if J is None else _dp(J)),
                    "thip_eval_cart_vel_all")
        return err, J

    def collision(self, term, x, cap=4096):
        """x [B, N, D] -> list of record arrays [n_b, 8 + 2 D + 1]."""
        B, D = self.wl.batch, self.wl.n_dof
        W = 8 + 2 * D + 1
        x = np.ascontiguousarray(x, dtype=np.float64)
        cnt = (C.c_int * B)()
        out = np.zeros((B, cap, W))
        self._check(self.lib.thip_eval_collision(self.ev, term, _dp(x), _dp(out), cap, cnt), "thip_eval_collision")
        if max(cnt) > cap:
            return self.collision(term, x, cap=max(cnt))
        return [out[b, : cnt[b]].copy() for b in range(B)]

    def close(self):
        if self.ev:
            self.lib.thip_eval_destroy(self.ev)
            self.ev = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TermValues:
    """thip_terms_*: the value of every cost and the violation of every constraint
    of every problem of a workload at any trajectories (OptResults::cost_vals /
    cnt_viols of the reference), in the fused kernel's slot order.  Takes the
    descriptors thip_create takes (contact test ALL, FIRST or CLOSEST); anything
    else raises."""

    def __init__(self, workload, device: int = 0):
        self.lib = abi.load_hip()
        self.wl = workload
        self.batch = workload.batch
        self.t = C.c_void_p()
        rc = self.lib.thip_terms_create(device, C.byref(workload.desc), self.batch, C.byref(self.t))
        if rc != 0:
            raise HipError(f"thip_terms_create: {self.lib.thip_terms_last_error(None).decode()}")
        nc, nv = C.c_int(), C.c_int()
        self._check(self.lib.thip_terms_counts(self.t, C.byref(nc), C.byref(nv)), "thip_terms_counts")
        self.n_costs, self.n_cnts = nc.value, nv.value
        tab = (abi.TermSlot * max(self.n_costs + self.n_cnts, 1))()
        self._check(self.lib.thip_terms_slots(self.t, tab), "thip_terms_slots")
        self.slots = list(tab)[: self.n_costs + self.n_cnts]
        self._tgt = np.ascontiguousarray(workload.targets, dtype=np.float64) if workload.targets.size else None
        self._scene = np.ascontiguousarray(workload.scene, dtype=np.float64) if workload.scene.size else None
        self._check(self.lib.thip_terms_upload(self.t, None if self._tgt is None else _dp(self._tgt),
                                               None if self._scene is None else _dp(self._scene)), "thip_terms_upload")
        jt = getattr(workload, "jpos_targets", None)
        if jt is not None:
            self._jpt = np.ascontiguousarray(jt, dtype=np.float64)
            self._check(self.lib.thip_terms_upload_joint_targets(self.t, _dp(self._jpt)),
                        "thip_terms_upload_joint_targets")

    def _check(self, rc, what):
        if rc != 0:
            raise HipError(f"{what}: {self.lib.thip_terms_last_error(self.t).decode()}")

    def slot_names(self):
        """One readable name per slot, costs first: e.g. 'cost:cart[3]', 'cnt:coll[2]@t=2'."""
        return [("cnt:" if s.is_cnt else "cost:") + f"{abi.TERM_KIND_NAMES[s.kind]}[{s.index}]"
                + (f"@t={s.unit}" if s.unit >= 0 else "") for s in self.slots]

    def _out(self):
        return np.zeros((self.batch, self.n_costs)), np.zeros((self.batch, self.n_cnts))

    def run(self, x):
        """x [B, N, D] (host) -> costs [B, n_costs], viols [B, n_cnts]."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.size != self.batch * self.wl.n_steps * self.wl.n_dof:
            raise HipError(f"TermValues.run: x has {x.size} values, not [batch][n_steps][n_dof]")
        costs, viols = self._out()
        self._check(self.lib.thip_terms_run(self.t, _dp(x), _dp(costs), _dp(viols)), "thip_terms_run")
        return costs, viols

    def run_device(self, d_x):
        """As run() on trajectories already on the device (an address, e.g. thip_device_x)."""
        costs, viols = self._out()
        self._check(self.lib.thip_terms_run_device(self.t, C.c_void_p(d_x), _dp(costs), _dp(viols)),
                    "thip_terms_run_device")
        return costs, viols

    def kernel_ms(self) -> float:
        return float(self.lib.thip_terms_last_ms(self.t))

    def close(self):
        if self.t:
            self.lib.thip_terms_destroy(self.t)
            self.t = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrajectoryChecker:
    """thip_check_*: tesseract's checkTrajectory for a batch -- per problem, is the
    joint trajectory within `margin` of its scene or of itself, how many such
    contacts, and the smallest signed distance with where it occurs.  Reads the
    chain, robot spheres, self-collision pairs, n_prims and n_steps of `desc`
    (a collision term is not needed); scene [B, n_prims, 16]."""

    def __init__(self, desc, batch, scene, config=None, device: int = 0):
        self.lib = abi.load_hip()
        self.batch = batch
        self.n_steps, self.n_dof = desc.n_steps, desc.chain.n_dof
        self.config = abi.default_check_config() if config is None else config
        self.chk = C.c_void_p()
        rc = self.lib.thip_check_create(device, C.byref(desc), C.byref(self.config), batch, C.byref(self.chk))
        if rc != 0:
            raise HipError(f"thip_check_create: {self.lib.thip_check_last_error(None).decode()}")
        self.n_units = self.lib.thip_check_units(self.chk)
        self._scene = np.ascontiguousarray(scene, dtype=np.float64) if desc.n_prims > 0 else None
        if self._scene is not None and self._scene.size != batch * desc.n_prims * 16:
            self.close()
            raise HipError(f"TrajectoryChecker: scene has {self._scene.size} values, not [batch][n_prims][16]")
        self._check(self.lib.thip_check_upload(self.chk, None if self._scene is None else _dp(self._scene)),
                    "thip_check_upload")

    def _check(self, rc, what):
        if rc != 0:
            raise HipError(f"{what}: {self.lib.thip_check_last_error(self.chk).decode()}")

    def _out(self, unit_min):
        res = (abi.CheckResult * self.batch)()
        um = np.zeros((self.batch, self.n_units)) if unit_min else None
        return res, um

    def run(self, x, unit_min=False):
        """x [B, N, D] (host) -> list of abi.CheckResult (, unit_min [B, n_units])."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.size != self.batch * self.n_steps * self.n_dof:
            raise HipError(f"TrajectoryChecker.run: x has {x.size} values, not [batch][n_steps][n_dof]")
        res, um = self._out(unit_min)
        self._check(self.lib.thip_check_run(self.chk, _dp(x), res, None if um is None else _dp(um)), "thip_check_run")
        return (list(res), um) if unit_min else list(res)

    def run_device(self, d_x, unit_min=False):
        """As run() on trajectories already on the device (an address, e.g. thip_device_x)."""
        res, um = self._out(unit_min)
        self._check(self.lib.thip_check_run_device(self.chk, C.c_void_p(d_x), res, None if um is None else _dp(um)),
                    "thip_check_run_device")
        return (list(res), um) if unit_min else list(res)

    def kernel_ms(self) -> float:
        return float(self.lib.thip_check_last_ms(self.chk))

    def close(self):
        if self.chk:
            self.lib.thip_check_destroy(self.chk)
            self.chk = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _CollisionSetsBase:
    """What CollisionSets and ContinuousCollisionSets share.  A subclass sets _api (the
    thip_<_api>_* symbols' prefix) and _count (the symbol that counts its nodes or
    segments) and has _jac_shape(); its __init__ calls _create() with the arguments of
    thip_<_api>_create between config and batch."""

    _api = _count = ""
    cs = None

    def _fn(self, name):
        return getattr(self.lib, f"thip_{self._api}_{name}")

    def _create(self, desc, batch, scene, config, device, *extra):
        """Creates the object, uploads the scene; returns the count of nodes or segments."""
        self.lib = abi.load_hip()
        self.batch = batch
        self.n_steps, self.n_dof = desc.n_steps, desc.chain.n_dof
        self.config = config
        self.cs = C.c_void_p()
        rc = self._fn("create")(device, C.byref(desc), C.byref(config), *extra, batch, C.byref(self.cs))
        if rc != 0:
            raise HipError(f"thip_{self._api}_create: {self._fn('last_error')(None).decode()}")
        self._items = self._fn(self._count)(self.cs)
        self.rows = config.max_num_cnt
        self._scene = np.ascontiguousarray(scene, dtype=np.float64) if desc.n_prims > 0 else None
        if self._scene is not None and self._scene.size != batch * desc.n_prims * 16:
            self.close()
            raise HipError(f"{type(self).__name__}: scene has {self._scene.size} values, not [batch][n_prims][16]")
        self._check(self._fn("upload")(self.cs, None if self._scene is None else _dp(self._scene)),
                    f"thip_{self._api}_upload")
        return self._items

    def _check(self, rc, what):
        if rc != 0:
            raise HipError(f"{what}: {self._fn('last_error')(self.cs).decode()}")

    def _out(self):
        rows = (self.batch, self._items, self.rows)
        return (np.zeros(rows), np.zeros(rows + self._jac_shape()), np.zeros(rows),
                np.zeros(rows[:2], dtype=np.int32), np.zeros(rows + (4,), dtype=np.int32))

    @staticmethod
    def _ip(a):
        return a.ctypes.data_as(C.POINTER(C.c_int))

    def _run(self, name, x):
        v, J, cf, cnt, keys = self._out()
        self._check(self._fn(name)(self.cs, x, _dp(v), _dp(J), _dp(cf), self._ip(cnt), self._ip(keys)),
                    f"thip_{self._api}_{name}")
        return v, J, cf, cnt, keys

    def run(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.size != self.batch * self.n_steps * self.n_dof:
            raise HipError(f"{type(self).__name__}.run: x has {x.size} values, not [batch][n_steps][n_dof]")
        return self._run("run", _dp(x))

    def run_device(self, d_x):
        """As run() on trajectories already on the device (an address)."""
        return self._run("run_device", C.c_void_p(d_x))

    def kernel_ms(self) -> float:
        return float(self._fn("last_ms")(self.cs))

    def close(self):
        if self.cs:
            self._fn("destroy")(self.cs)
            self.cs = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CollisionSets(_CollisionSetsBase):
    """thip_csets_*: the rows of trajopt_ifopt's fixed-size DiscreteCollisionConstraint
    (SingleTimestepCollisionEvaluator) at every node of [first_step, last_step]
    of every problem, one launch per x.  Reads the chain, robot spheres,
    self-collision pairs, n_prims, n_steps and collision term 0's coll_pairs of
    `desc`; config: abi.CsetsConfig; scene [B, n_prims, 16]."""

    _api, _count = "csets", "nodes"

    def __init__(self, desc, batch, scene, config, device: int = 0):
        self.n_nodes = self._create(desc, batch, scene, config, device)

    def _jac_shape(self):
        return (self.n_dof,)

    def run(self, x):
        """x [B, N, D] (host) -> values [B, n, R], jac [B, n, R, D], coeffs [B, n, R],
        counts [B, n], keys [B, n, R, 4] (link, other, sphere, other_sphere)."""
        return super().run(x)


class ContinuousCollisionSets(_CollisionSetsBase):
    """thip_ccsets_*: the rows of trajopt_ifopt's fixed-size ContinuousCollisionConstraint
    (LVSContinuousCollisionEvaluator / LVSDiscreteCollisionEvaluator) on every segment
    (t, t + 1), first_step <= t < last_step, of every problem, one launch per x.  Reads
    what CollisionSets reads of `desc`; config: abi.CcsetsConfig; scene [B, n_prims, 16];
    seg_fixed: per segment bit 0 = vars0 fixed, bit 1 = vars1 fixed (None: no end fixed)."""

    _api, _count = "ccsets", "segments"

    def __init__(self, desc, batch, scene, config, seg_fixed=None, device: int = 0):
        fixed = None
        if seg_fixed is not None:
            fixed = np.ascontiguousarray(seg_fixed, dtype=np.int32)
            n = config.last_step - config.first_step
            if fixed.size != max(n, 0) and n > 0:
                raise HipError(f"ContinuousCollisionSets: seg_fixed has {fixed.size} entries, not {n}")
        self.n_segments = self._create(desc, batch, scene, config, device, None if fixed is None else self._ip(fixed))

    def _jac_shape(self):
        return (2, self.n_dof)

    def run(self, x):
        """x [B, N, D] (host) -> values [B, n, R], jac [B, n, R, 2, D] (end 0 = node t, end 1 =
        node t + 1), coeffs [B, n, R], counts [B, n], keys [B, n, R, 4].  Raises when a segment
        needs more than abi.CCSETS_MAX_SUBSTATES states."""
        return super().run(x)
