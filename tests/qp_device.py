"""A thin handle on the C-ABI's generic QP object (thip_qp_*, csrc/qp_csc.hip)
for the direct tests and tools/qp_direct_gaps.py: numpy in, numpy and plain
dicts out, nothing hidden -- every return code of the library is asserted or
handed back."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from trajopt_amd import abi

INFO_FIELDS = ("status", "setup_error", "polish_status", "iter", "rho", "prim_res", "dual_res")
E_STATE = -4  # THIP_E_STATE


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


def _stack(vs, width):
    """[count][width] doubles (at least one element, so the pointer is never NULL)."""
    out = np.zeros(max(len(vs) * width, 1))
    for k, v in enumerate(vs):
        out[k * width:(k + 1) * width] = v
    return out


def info_dict(i):
    return {k: getattr(i, k) for k in INFO_FIELDS}


class GpuQp:
    """One thip_qp: the pattern of `case`, `batch` QPs.  level_solve creates it
    with THIP_QP_LEVEL_SOLVE=1 in the environment (the level-by-level forward
    solve) and restores the environment after the create."""

    def __init__(self, case, batch=1, level_solve=False, device=0):
        self.L = abi.load_hip()
        self.n, self.m, self.batch = case.n, case.m, batch
        self.nnz_p, self.nnz_a = case.P.nnz, case.A.nnz
        pat = [np.ascontiguousarray(v, dtype=np.int32) for v in
               (case.P.indptr, case.P.indices, case.A.indptr, case.A.indices)]
        pat = [v if v.size else np.zeros(1, dtype=np.int32) for v in pat]
        self.h = C.c_void_p()
        old = os.environ.get("THIP_QP_LEVEL_SOLVE")
        if level_solve:
            os.environ["THIP_QP_LEVEL_SOLVE"] = "1"
        else:
            os.environ.pop("THIP_QP_LEVEL_SOLVE", None)
        try:
            rc = self.L.thip_qp_create(device, self.n, self.m, _ip(pat[0]), _ip(pat[1]), _ip(pat[2]), _ip(pat[3]),
                                       batch, C.byref(self.h))
        finally:
            if old is None:
                os.environ.pop("THIP_QP_LEVEL_SOLVE", None)
            else:
                os.environ["THIP_QP_LEVEL_SOLVE"] = old
        if rc != 0:
            raise RuntimeError(f"thip_qp_create: {rc} {self.L.thip_qp_last_error(None)}")
        self._keep = None

    def close(self):
        if self.h:
            self.L.thip_qp_destroy(self.h)
            self.h = C.c_void_p()

    def error(self):
        e = self.L.thip_qp_last_error(self.h)
        return e.decode() if e else ""

    def shape(self):
        out = (C.c_longlong * 6)()
        assert self.L.thip_qp_shape(self.h, out) == 0
        return list(out)

    def tier(self):
        """1 the factor in LDS, 2 the solve vector in LDS, 3 the solve vector in HBM
        (None: the shape words fit none of them)."""
        N, _, _, _, lds_pat, lds = self.shape()
        if lds_pat == 1:
            return 1
        if lds_pat == 0 and lds > 0 and N <= 8192:
            return 2
        if lds == 0 and N > 8192:
            return 3
        return None

    # ------------------------------------------------------------ one-shot
    def _inputs(self, cases, warm_x, warm_y, warm_mask, warm_rho):
        cnt = len(cases)
        assert 1 <= cnt <= self.batch
        for c in cases:
            assert (c.n, c.m, c.P.nnz, c.A.nnz) == (self.n, self.m, self.nnz_p, self.nnz_a)
        a = dict(Pv=_stack([c.P.data for c in cases], self.nnz_p), q=_stack([c.q for c in cases], self.n),
                 Av=_stack([c.A.data for c in cases], self.nnz_a), l=_stack([c.l for c in cases], self.m),
                 u=_stack([c.u for c in cases], self.m))
        a["wx"] = None if warm_x is None else _stack(warm_x, self.n)
        a["wy"] = None if warm_y is None else _stack(warm_y, self.m)
        a["mask"] = None if warm_mask is None else np.ascontiguousarray(warm_mask, dtype=np.int32)
        a["rho"] = None if warm_rho is None else np.ascontiguousarray(warm_rho, dtype=np.float64)
        assert a["mask"] is None or a["mask"].size == cnt
        assert a["rho"] is None or a["rho"].size == cnt
        return cnt, a

    def _outputs(self, cnt):
        return np.full(max(cnt * self.n, 1), -7.0), np.full(max(cnt * self.m, 1), -7.0), (abi.QpInfo * cnt)()

    def _results(self, cnt, x, y, info):
        return [(x[k * self.n:(k + 1) * self.n].copy(), y[k * self.m:(k + 1) * self.m].copy(), info_dict(info[k]))
                for k in range(cnt)]

    def solve(self, cases, settings, warm_x=None, warm_y=None, warm_rho=None):
        """thip_qp_solve: len(cases) must be the batch."""
        cnt, a = self._inputs(cases, warm_x, warm_y, None, warm_rho)
        assert cnt == self.batch
        x, y, info = self._outputs(cnt)
        rc = self.L.thip_qp_solve(self.h, _dp(a["Pv"]), _dp(a["q"]), _dp(a["Av"]), _dp(a["l"]), _dp(a["u"]),
                                  C.byref(settings), _dp(a["wx"]), _dp(a["wy"]), _dp(a["rho"]), _dp(x), _dp(y), info)
        assert rc == 0, (rc, self.error())
        return self._results(cnt, x, y, info)

    def solve_some(self, cases, settings, warm_x=None, warm_y=None, warm_mask=None, warm_rho=None):
        cnt, a = self._inputs(cases, warm_x, warm_y, warm_mask, warm_rho)
        x, y, info = self._outputs(cnt)
        rc = self.L.thip_qp_solve_some(self.h, cnt, _dp(a["Pv"]), _dp(a["q"]), _dp(a["Av"]), _dp(a["l"]),
                                       _dp(a["u"]), C.byref(settings), _dp(a["wx"]), _dp(a["wy"]), _ip(a["mask"]),
                                       _dp(a["rho"]), _dp(x), _dp(y), info)
        assert rc == 0, (rc, self.error())
        return self._results(cnt, x, y, info)

    def submit(self, cases, settings, launch=True, **kw):
        """thip_qp_submit (or thip_qp_stage with launch=False); the inputs stay alive until collect()."""
        cnt, a = self._inputs(cases, kw.get("warm_x"), kw.get("warm_y"), kw.get("warm_mask"), kw.get("warm_rho"))
        self._keep = (cnt, a, settings)
        f = self.L.thip_qp_submit if launch else self.L.thip_qp_stage
        rc = f(self.h, cnt, _dp(a["Pv"]), _dp(a["q"]), _dp(a["Av"]), _dp(a["l"]), _dp(a["u"]), C.byref(settings),
               _dp(a["wx"]), _dp(a["wy"]), _ip(a["mask"]), _dp(a["rho"]))
        assert rc == 0, (rc, self.error())

    def collect(self):
        cnt = self._keep[0]
        x, y, info = self._outputs(cnt)
        rc = self.L.thip_qp_collect(self.h, _dp(x), _dp(y), info)
        assert rc == 0, (rc, self.error())
        self._keep = None
        return self._results(cnt, x, y, info)

    @staticmethod
    def launch_staged(qps):
        arr = (C.c_void_p * len(qps))(*[q.h for q in qps])
        rc = qps[0].L.thip_qp_launch_staged(arr, len(qps))
        assert rc == 0, (rc, qps[0].error())

    # ------------------------------------------------------------ resident (batch 1)
    def _err(self, rc, info):
        assert rc == 0, (rc, self.error())
        return info.setup_error if info.status == -1 else 0

    def setup(self, case, settings):
        assert self.batch == 1
        _, a = self._inputs([case], None, None, None, None)
        info = abi.QpInfo()
        rc = self.L.thip_qp_setup(self.h, _dp(a["Pv"]), _dp(a["q"]), _dp(a["Av"]), _dp(a["l"]), _dp(a["u"]),
                                  C.byref(settings), C.byref(info))
        return self._err(rc, info)

    def update_vec(self, q=None, l=None, u=None):
        q, l, u = (None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (q, l, u))
        assert (q is None or q.size == self.n) and (l is None or l.size == self.m) and (u is None or u.size == self.m)
        info = abi.QpInfo()
        return self._err(self.L.thip_qp_update_vec(self.h, _dp(q), _dp(l), _dp(u), C.byref(info)), info)

    def update_mat(self, Px=None, Ax=None):
        Px, Ax = (None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (Px, Ax))
        assert (Px is None or Px.size == self.nnz_p) and (Ax is None or Ax.size == self.nnz_a)
        info = abi.QpInfo()
        return self._err(self.L.thip_qp_update_mat(self.h, _dp(Px), _dp(Ax), C.byref(info)), info)

    def warm_start(self, x=None, y=None):
        x, y = (None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (x, y))
        assert (x is None or x.size == self.n) and (y is None or y.size == self.m)
        rc = self.L.thip_qp_warm_start(self.h, _dp(x), _dp(y))
        assert rc == 0, (rc, self.error())
        return 0

    def solve_resident_rc(self):
        """(return code, results or None): THIP_E_STATE when there is no workspace."""
        x, y, info = self._outputs(1)
        rc = self.L.thip_qp_solve_resident(self.h, _dp(x), _dp(y), info)
        return rc, (self._results(1, x, y, info)[0] if rc == 0 else None)

    def solve_resident(self):
        rc, res = self.solve_resident_rc()
        assert rc == 0, (rc, self.error())
        return res
