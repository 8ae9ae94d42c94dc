"""GPU tests of thip_qp_step (include/trajopt_hip.h): the masked, fused step on
the resident QP workspaces.  Its contract is bitwise: for every QP of the batch
the workspace, x, y and info after a step are what the separate resident calls
give on a batch-1 object, issued in the order update_mat(P), update_vec(q),
update_mat(A), update_vec(l, u), warm_start, solve_resident.  Every test keeps
such a twin per QP and compares bytes; a workspace is compared through its next
warm-started solve, which continues from everything a workspace keeps.

The small QP is the 12-variable, 20-row one of
test_gpu_tsqp.py::test_resident_setup_equals_one_shot, and the perturbed data
come from the same generator."""
import ctypes as C

import numpy as np
import pytest

from trajopt_amd import abi

pytestmark = pytest.mark.gpu

SETUP, MAT_P, VEC_Q, MAT_A, VEC_BOUNDS, WARM, SOLVE = (abi.QP_OP_SETUP, abi.QP_OP_MAT_P, abi.QP_OP_VEC_Q,
                                                       abi.QP_OP_MAT_A, abi.QP_OP_VEC_BOUNDS, abi.QP_OP_WARM,
                                                       abi.QP_OP_SOLVE)
UPDATES = MAT_P | VEC_Q | MAT_A | VEC_BOUNDS
SENTINEL = -12345.678

dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731


@pytest.fixture(scope="module")
def L():
    lib = abi.load_hip()
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


def _csc(Mx):
    p, i, x = [0], [], []
    for j in range(Mx.shape[1]):
        nz = np.nonzero(Mx[:, j])[0]
        i += list(nz)
        x += list(Mx[nz, j])
        p.append(len(i))
    return np.array(p, dtype=np.int32), np.array(i, dtype=np.int32), np.array(x, dtype=np.float64)


class Pattern:
    """A sparsity pattern with its base data and a generator of perturbed data."""

    def __init__(self, Pu, A, q, lo, up, rng):
        self.n, self.m = A.shape[1], A.shape[0]
        self.Pp, self.Pi, self.Px = _csc(Pu)
        self.Ap, self.Ai, self.Ax = _csc(A)
        self.q, self.lo, self.up, self.rng = q, lo, up, rng

    def data(self):
        """(P values, q, A values, l, u), perturbed: P stays positive definite
        (its smallest eigenvalue is above 1, the change below 0.3 in norm)."""
        r = self.rng
        return (self.Px * (1 + 0.01 * r.normal(size=self.Px.shape)), self.q + 0.1 * r.normal(size=self.n),
                self.Ax * (1 + 0.05 * r.normal(size=self.Ax.shape)), self.lo - 0.1 * r.random(self.m),
                self.up + 0.1 * r.random(self.m))

    def warm(self):
        return 0.1 * self.rng.normal(size=self.n), 0.1 * self.rng.normal(size=self.m)

    def create(self, L, batch):
        h = C.c_void_p()
        assert L.thip_qp_create(0, self.n, self.m, ip(self.Pp), ip(self.Pi), ip(self.Ap), ip(self.Ai), batch,
                                C.byref(h)) == 0, L.thip_qp_last_error(None)
        return h


def small_pattern():
    rng = np.random.default_rng(7)
    n, m0 = 12, 8
    M = rng.normal(size=(n, n))
    Pu = np.triu(M @ M.T + np.eye(n))
    A = np.vstack([rng.normal(size=(m0, n)) * (rng.random((m0, n)) < 0.5), np.eye(n)])
    q = rng.normal(size=n)
    lo = np.concatenate([rng.uniform(-1, 0, m0), np.full(n, -2.0)])
    up = np.concatenate([rng.uniform(0, 1, m0), np.full(n, 2.0)])
    return Pattern(Pu, A, q, lo, up, rng)


def settings(L):
    s = abi.OsqpSettings()
    L.thip_default_osqp_settings(C.byref(s))
    return s


class Twin:
    """One QP on a batch-1 object, driven by the separate resident calls in the contract's order."""

    def __init__(self, L, pat, s):
        self.L, self.pat, self.s = L, pat, s
        self.h = pat.create(L, 1)
        self.info = abi.QpInfo()
        self.x, self.y = np.zeros(pat.n), np.zeros(pat.m)

    def run(self, ops, d=None, w=None):
        L, h, info = self.L, self.h, C.byref(self.info)
        if ops & SETUP:
            assert L.thip_qp_setup(h, dp(d[0]), dp(d[1]), dp(d[2]), dp(d[3]), dp(d[4]), C.byref(self.s), info) == 0
        if ops & MAT_P:
            assert L.thip_qp_update_mat(h, dp(d[0]), None, info) == 0
        if ops & VEC_Q:
            assert L.thip_qp_update_vec(h, dp(d[1]), None, None, info) == 0
        if ops & MAT_A:
            assert L.thip_qp_update_mat(h, None, dp(d[2]), info) == 0
        if ops & VEC_BOUNDS:
            assert L.thip_qp_update_vec(h, None, dp(d[3]), dp(d[4]), info) == 0
        if ops & WARM:
            assert L.thip_qp_warm_start(h, dp(w[0]), dp(w[1])) == 0
        if ops & SOLVE:
            assert L.thip_qp_solve_resident(h, dp(self.x), dp(self.y), info) == 0
        return self

    def close(self):
        self.L.thip_qp_destroy(self.h)


class Batch:
    """A batch object driven by thip_qp_step; rows of x, y, info start as sentinels."""

    def __init__(self, L, pat, s, batch):
        self.L, self.pat, self.s, self.B = L, pat, s, batch
        self.h = pat.create(L, batch)
        self.x = np.full((batch, pat.n), SENTINEL)
        self.y = np.full((batch, pat.m), SENTINEL)
        self.info = (abi.QpInfo * batch)()
        self.reset_rows()

    def reset_rows(self):
        self.x[:], self.y[:] = SENTINEL, SENTINEL
        C.memset(self.info, 0x5A, C.sizeof(self.info))

    def step(self, ops, data=None, warm=None):
        """ops [B]; data / warm: per-QP tuples (None where a QP has none)."""
        pat, B = self.pat, self.B
        sizes = (len(pat.Px), pat.n, len(pat.Ax), pat.m, pat.m)
        arrs = [np.zeros((B, k)) for k in sizes]
        wx, wy = np.zeros((B, pat.n)), np.zeros((B, pat.m))
        for b in range(B):
            if data is not None and data[b] is not None:
                for a, v in zip(arrs, data[b]):
                    a[b] = v
            if warm is not None and warm[b] is not None:
                wx[b], wy[b] = warm[b]
        o = np.array(ops, dtype=np.int32)
        if data is None:  # no QP uses them: NULL
            arrs = [None] * 5
        if warm is None:
            wx = wy = None
        return self.L.thip_qp_step(self.h, ip(o), dp(arrs[0]), dp(arrs[1]), dp(arrs[2]), dp(arrs[3]), dp(arrs[4]),
                                   C.byref(self.s), dp(wx), dp(wy), dp(self.x), dp(self.y), self.info)

    def untouched(self, b):
        return (np.all(self.x[b] == SENTINEL) and np.all(self.y[b] == SENTINEL)
                and bytes(self.info[b]) == b"\x5a" * C.sizeof(abi.QpInfo))

    def error(self):
        return self.L.thip_qp_last_error(self.h).decode()

    def close(self):
        self.L.thip_qp_destroy(self.h)


def same(batch, b, twin, solved=True):
    """Row b of the batch against its twin, bit for bit: every info field, and x, y after a solve."""
    fields = [f for f, _ in abi.QpInfo._fields_]
    got = {f: getattr(batch.info[b], f) for f in fields}
    want = {f: getattr(twin.info, f) for f in fields}
    assert bytes(batch.info[b]) == bytes(twin.info), (b, got, want)
    if solved:
        assert batch.x[b].tobytes() == twin.x.tobytes(), (b, np.abs(batch.x[b] - twin.x).max())
        assert batch.y[b].tobytes() == twin.y.tobytes(), (b, np.abs(batch.y[b] - twin.y).max())
        assert twin.info.status == 1 and twin.info.iter > 0  # a real solve was compared


def test_batch1_equals_separate_calls(L):
    pat, s = small_pattern(), settings(L)
    bt, tw = Batch(L, pat, s, 1), Twin(L, pat, s)
    d0, w0 = pat.data(), pat.warm()
    assert bt.step([SETUP | WARM | SOLVE], [d0], [w0]) == 0, bt.error()
    same(bt, 0, tw.run(SETUP | WARM | SOLVE, d0, w0))
    d1, w1 = pat.data(), pat.warm()
    assert bt.step([UPDATES | WARM | SOLVE], [d1], [w1]) == 0, bt.error()
    same(bt, 0, tw.run(UPDATES | WARM | SOLVE, d1, w1))
    # and what the workspace keeps: the next solve continues from it
    assert bt.step([SOLVE]) == 0
    same(bt, 0, tw.run(SOLVE))
    bt.close(), tw.close()


def _three(L):
    pat, s = small_pattern(), settings(L)
    bt, tws = Batch(L, pat, s, 3), [Twin(L, pat, s) for _ in range(3)]
    d = [pat.data() for _ in range(3)]
    assert bt.step([SETUP | SOLVE] * 3, d) == 0, bt.error()
    for b in range(3):
        same(bt, b, tws[b].run(SETUP | SOLVE, d[b]))
    return pat, bt, tws


def test_masked_step(L):
    pat, bt, tws = _three(L)
    d = [pat.data(), pat.data(), None]
    bt.reset_rows()
    assert bt.step([UPDATES | SOLVE, VEC_BOUNDS | SOLVE, 0], d) == 0, bt.error()
    same(bt, 0, tws[0].run(UPDATES | SOLVE, d[0]))
    same(bt, 1, tws[1].run(VEC_BOUNDS | SOLVE, d[1]))
    assert bt.untouched(2)
    # QP 2's workspace never saw the step
    bt.reset_rows()
    assert bt.step([0, 0, SOLVE]) == 0
    same(bt, 2, tws[2].run(SOLVE))
    assert bt.untouched(0) and bt.untouched(1)
    bt.close(), [t.close() for t in tws]


def test_bounds_refused_for_one_qp(L):
    pat, bt, tws = _three(L)
    d = [list(pat.data()) for _ in range(3)]
    d[1][3] = d[1][3].copy()
    d[1][3][5] = d[1][4][5] + 0.25  # l > u in one row of QP 1 only
    bt.reset_rows()
    assert bt.step([VEC_BOUNDS | SOLVE] * 3, d) == 0, bt.error()
    assert (bt.info[1].status, bt.info[1].setup_error) == (-1, 1)
    tws[1].run(VEC_BOUNDS, d[1])
    assert (tws[1].info.status, tws[1].info.setup_error) == (-1, 1)
    assert np.all(bt.x[1] == SENTINEL)  # its ops of the step were dropped
    for b in (0, 2):
        same(bt, b, tws[b].run(VEC_BOUNDS | SOLVE, d[b]))
    # QP 1 kept its data and stays live
    assert bt.step([0, SOLVE, 0]) == 0, bt.error()
    same(bt, 1, tws[1].run(SOLVE))
    bt.close(), [t.close() for t in tws]


def test_setup_beside_solve_and_state_errors(L):
    pat, s = small_pattern(), settings(L)
    bt, tws = Batch(L, pat, s, 2), [Twin(L, pat, s) for _ in range(2)]
    d0, d1 = pat.data(), pat.data()
    # never set up, selected without SETUP: refused whole, nothing changes
    assert bt.step([SETUP | SOLVE, SOLVE], [d0, None]) == abi.E_STATE
    assert "QP 1" in bt.error()
    assert bt.untouched(0) and bt.untouched(1)
    assert bt.step([SOLVE, 0]) == abi.E_STATE and "QP 0" in bt.error()  # QP 0 was not set up by the refused call
    assert bt.step([SETUP | SOLVE, 0], [d0, None]) == 0, bt.error()
    same(bt, 0, tws[0].run(SETUP | SOLVE, d0))
    assert bt.untouched(1)
    # QP 1 is set up while QP 0 solves on
    assert bt.step([SOLVE, SETUP | SOLVE], [None, d1]) == 0, bt.error()
    same(bt, 0, tws[0].run(SOLVE))
    same(bt, 1, tws[1].run(SETUP | SOLVE, d1))
    # SETUP excludes the updates; other settings than the live QPs' are refused
    assert bt.step([SETUP | VEC_Q, 0], [d0, None]) == abi.E_INVALID
    other = settings(L)
    other.alpha = 1.5
    keep, bt.s = bt.s, other
    assert bt.step([SETUP, 0], [d0, None]) == abi.E_INVALID and "settings" in bt.error()
    bt.s = keep
    # a refactorisation that fails kills QP 0 alone: P = -P is not quasi-definite
    bad = (-d0[0],) + tuple(d0[1:])
    assert bt.step([MAT_P | SOLVE, 0], [bad, None]) == 0, bt.error()
    tws[0].run(MAT_P, bad)
    assert bt.info[0].status == -1 and bt.info[0].setup_error in (4, 5)
    same(bt, 0, tws[0], solved=False)
    bt.reset_rows()
    assert bt.step([SOLVE, 0]) == abi.E_STATE and "QP 0" in bt.error()
    assert bt.untouched(0)
    assert bt.step([0, SOLVE]) == 0, bt.error()
    same(bt, 1, tws[1].run(SOLVE))
    bt.close(), [t.close() for t in tws]


# Nodes of the trajectory pattern below: the smallest count whose factor, staged
# in LDS, takes more than 64 KB of dynamic LDS (thip_qp_shape out[5]), so that a
# launch needs hipFuncAttributeMaxDynamicSharedMemorySize raised for the kernel
# it launches.  The test asserts that it does.  (The bytes grow by 1168 a node:
# 46,216 at 40 nodes, 64,904 at 56.)
LARGE_NODES = 58


def trajectory_pattern(T, D=7):
    """A joint trajectory's QP: squared velocity and acceleration costs over T nodes
    of D joints (P block pentadiagonal), the box rows and one velocity row per joint
    and segment."""
    rng = np.random.default_rng(31)
    n = T * D
    V = np.zeros(((T - 1) * D, n))
    for t in range(T - 1):
        for k in range(D):
            V[t * D + k, t * D + k], V[t * D + k, (t + 1) * D + k] = -1.0, 1.0
    Acc = np.zeros(((T - 2) * D, n))
    for t in range(T - 2):
        for k in range(D):
            r = t * D + k
            Acc[r, r], Acc[r, r + D], Acc[r, r + 2 * D] = 1.0, -2.0, 1.0
    Pu = np.triu(V.T @ V + 0.5 * Acc.T @ Acc + 2.0 * np.eye(n))
    A = np.vstack([np.eye(n), V])
    q = rng.normal(size=n)
    lo = np.concatenate([np.full(n, -1.0), np.full((T - 1) * D, -0.3)])
    up = -lo
    return Pattern(Pu, A, q, lo, up, rng)


def test_large_pattern_over_64k_lds(L):
    pat, s = trajectory_pattern(LARGE_NODES), settings(L)
    bt, tw = Batch(L, pat, s, 2), Twin(L, pat, s)
    shape = (C.c_longlong * 6)()
    assert L.thip_qp_shape(bt.h, shape) == 0
    assert shape[4] == 1 and shape[5] > 65536, list(shape)
    d0, w0, d1 = pat.data(), pat.warm(), pat.data()
    assert bt.step([0, SETUP | WARM | SOLVE], [None, d0], [None, w0]) == 0, bt.error()
    same(bt, 1, tw.run(SETUP | WARM | SOLVE, d0, w0))
    assert bt.step([0, UPDATES | SOLVE], [None, d1]) == 0, bt.error()
    same(bt, 1, tw.run(UPDATES | SOLVE, d1))
    assert bt.untouched(0)
    bt.close(), tw.close()
