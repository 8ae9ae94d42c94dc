"""The reference side of the direct QP tests: what tests/test_qp_cases.py proves
on the CPU and tests/test_gpu_qp_direct.py holds the device to.

  * reruns(case): the oracle's ten solves of a case -- the exact build, the
    fast build (FMA contraction, another rounding of the same algorithm) and 8
    seeds of a relative 1e-12 jitter on every KKT solution entry (the amplitude
    tests/test_gpu_tsqp.py uses, 200 x the parity gate's 5e-15) -- and their
    spread around the exact build's answer.
  * kkt_star(case, y): the active set read from a dual vector, and the
    equality-constrained KKT system of that active set solved by iterative
    refinement with long-double residuals: x*, y*, and a 1-norm condition
    estimate of the reduced KKT matrix.
  * termination_gaps(case, x, y): OSQP's termination guarantee recomputed in
    long double from (x, y) alone.

Everything is cached per case name: a reference is computed once and shared.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import qp_cases

LD = np.longdouble
JITTER = 1e-12
SEEDS = tuple(range(1, 9))
DISCRETE = ("status", "setup_error", "iter", "polish_status", "rho_updates")
EPS = 2.0 ** -53


def _oracle():
    from oracle import oracle

    return oracle


def solve_oracle(case, variant="exact", seed=None, **kw):
    o = _oracle()
    s = qp_cases.settings_of(case)
    if seed is not None:
        o.set_jitter(kkt_rel=JITTER, seed=seed, variant=variant)
    try:
        return o.qp_solve_info(case.P, case.q, case.A, case.l, case.u, s, variant=variant, **kw)
    finally:
        if seed is not None:
            o.set_jitter(variant=variant)


class Reruns:
    """runs[0] is the exact build's (x, y, info); spread[k] = max over the ten of
    |value - exact value| for k in x, y, rho, prim_res, dual_res."""

    def __init__(self, case):
        self.runs = [solve_oracle(case), solve_oracle(case, "fast")] + [solve_oracle(case, seed=k) for k in SEEDS]
        self.x, self.y, self.info = self.runs[0]
        self.keys = {tuple(i[k] for k in DISCRETE) for _, _, i in self.runs}
        self.spread = {}
        if np.isfinite(self.x).all():
            self.spread["x"] = max(float(np.abs(r[0] - self.x).max()) for r in self.runs)
            self.spread["y"] = max(float(np.abs(r[1] - self.y).max(initial=0.0)) for r in self.runs)
        for k in ("rho", "prim_res", "dual_res"):
            self.spread[k] = max(abs(r[2][k] - self.info[k]) for r in self.runs)


@functools.lru_cache(maxsize=None)
def reruns(name):
    return Reruns(qp_cases.CASES[name])


def full_P(case):
    U = sp.csc_matrix(case.P)
    return (U + sp.triu(U, 1).T).tocsc()


def _ld_matvec(M, v):
    """M v in long double (M scipy sparse, v long double)."""
    M = M.tocoo()
    out = np.zeros(M.shape[0], dtype=LD)
    np.add.at(out, M.row, M.data.astype(LD) * v[M.col])
    return out


class Star:
    pass


def _inv_norm1(lu, N):
    x = np.full(N, 1.0 / N)
    est = 0.0
    for _ in range(8):
        y = lu.solve(x)
        est = max(est, float(np.abs(y).sum()))
        z = lu.solve(np.where(y >= 0, 1.0, -1.0), "T")
        j = int(np.argmax(np.abs(z)))
        if np.abs(z[j]) <= z @ x:
            break
        x = np.zeros(N)
        x[j] = 1.0
    return est


def kkt_star_of(case, y):
    """x*, y* of the active set read from y (y < 0: the lower bound, y > 0: the
    upper bound; equality rows always), by LU in double and refinement with
    long-double residuals until the correction stalls."""
    n, m = case.n, case.m
    eq = case.l == case.u
    low = (y < 0) & ~eq
    upp = (y > 0) & ~eq
    act = np.flatnonzero(low | upp | eq)
    b = np.where(upp, case.u, case.l)[act]
    Aa = sp.csc_matrix(case.A)[act, :] if m else sp.csc_matrix((0, n))
    P = full_P(case)
    K = sp.bmat([[P, Aa.T], [Aa, None]], format="csc") if len(act) else P
    rhs = np.concatenate([-case.q, b]).astype(LD)
    lu = spla.splu(K.astype(np.float64))
    z = lu.solve(np.asarray(rhs, dtype=np.float64)).astype(LD)
    last = np.inf
    for _ in range(20):
        r = rhs - _ld_matvec(K, z)
        dz = lu.solve(np.asarray(r, dtype=np.float64)).astype(LD)
        z = z + dz
        step = float(np.abs(dz).max())
        if step == 0.0 or step >= last:
            break
        last = step
    s = Star()
    s.act = act
    s.x = z[:n]
    s.y = np.zeros(m, dtype=LD)
    s.y[act] = z[n:]
    s.residual = float(np.abs(rhs - _ld_matvec(K, z)).max())
    N = K.shape[0]
    if N <= 600:
        Kd = K.toarray()
        s.cond = float(np.linalg.norm(Kd, 1) * np.linalg.norm(np.linalg.inv(Kd), 1))
    else:
        # |K^-1|_1 by Hager's estimator from the fixed start e / N: deterministic, and a lower
        # estimate, so a tolerance from it errs on the strict side
        s.cond = float(abs(K).sum(axis=0).max() * _inv_norm1(lu, N))
    s.scale = float(max(np.abs(z).max(), 1e-300))
    s.forward = s.cond * EPS * s.scale  # forward-error bound of the reduced KKT solve in double
    return s


@functools.lru_cache(maxsize=None)
def kkt_star(name):
    """The long-double reference of a solved catalogue case, from the oracle's own y."""
    return kkt_star_of(qp_cases.CASES[name], reruns(name).y)


def termination_gaps(case, x, y, **over):
    """(primal gap, primal tolerance, dual gap, dual tolerance) of OSQP's
    termination test, in long double from (x, y):
        dist_inf(Ax, [l, u])   <= eps_abs + eps_rel max(|Ax|, |z|),   z = Ax clipped to [l, u]
        |Px + q + A'y|_inf     <= eps_abs + eps_rel max(|Px|, |A'y|, |q|)"""
    s = qp_cases.settings_of(case, **over)
    x = np.asarray(x, dtype=LD)
    y = np.asarray(y, dtype=LD)
    nrm = lambda v: float(np.abs(v).max(initial=0.0))  # noqa: E731
    Ax = _ld_matvec(sp.csc_matrix(case.A), x) if case.m else np.zeros(0, dtype=LD)
    z = np.minimum(np.maximum(Ax, case.l.astype(LD)), case.u.astype(LD))
    Px = _ld_matvec(full_P(case), x)
    Aty = _ld_matvec(sp.csc_matrix(case.A).T, y) if case.m else np.zeros(case.n, dtype=LD)
    prim = nrm(Ax - z)
    dual = nrm(Px + case.q.astype(LD) + Aty)
    return (prim, s.eps_abs + s.eps_rel * max(nrm(Ax), nrm(z)), dual,
            s.eps_abs + s.eps_rel * max(nrm(Px), nrm(Aty), nrm(case.q)))


def err_inf(a, b):
    return float(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)).max(initial=0.0))


# ---------------------------------------------------------------- resident sequences
class Sequence:
    """The update-in-place sequence of the direct tests on one catalogue case, as
    a list of steps (op, arguments, the problem data after the step):
      setup, solve | update_vec(q), solve (the factor a polish left dirty) |
      update_vec(l, u): one range row becomes an equality and one a free row, solve |
      update_mat(P), solve | update_mat(A) | warm_start(x), solve | warm_start(y), solve |
      update_vec with l > u (error 1, rejected), solve | update_mat to -1e4 P (error 5, the
      solver object is gone), solve_gone | setup, solve.
    All arrays are fixed by the case and its name's seed: the oracle and the
    device are driven with the same numbers."""

    def __init__(self, name):
        c = qp_cases.CASES[name]
        self.name, self.case = name, c
        rng = np.random.default_rng(sum(name.encode()))
        n, m = c.n, c.m
        rows = np.flatnonzero((c.l > -1e29) & (c.u < 1e29) & (c.u - c.l > 1e-3))
        e, f = int(rows[len(rows) // 3]), int(rows[2 * len(rows) // 3])
        self.to_eq, self.to_free = e, f
        q2 = c.q + 0.5 * np.abs(c.q).max() * rng.normal(size=n)
        l3, u3 = c.l.copy(), c.u.copy()
        l3[e] = u3[e] = 0.25 * c.l[e] + 0.75 * c.u[e]
        l3[f], u3[f] = -qp_cases.INF, qp_cases.INF
        d = rng.uniform(0.8, 1.25, n)  # D P D stays positive definite
        coo = c.P.tocoo()
        order = np.lexsort((coo.row, coo.col))
        P4 = c.P.data * d[coo.row[order]] * d[coo.col[order]]
        A5 = c.A.data * (1.0 + 0.05 * rng.normal(size=c.A.nnz))
        xw, yw = 0.1 * rng.normal(size=n), 0.1 * rng.normal(size=m)
        lbad, ubad = l3.copy(), u3.copy()
        lbad[e] = ubad[e] + 1.0
        mk = lambda **kw: self._data(c, **kw)  # noqa: E731
        d0 = mk()
        d2 = mk(q=q2)
        d3 = mk(q=q2, l=l3, u=u3)
        d4 = mk(q=q2, l=l3, u=u3, Px=P4)
        d5 = mk(q=q2, l=l3, u=u3, Px=P4, Ax=A5)
        S = "solve"
        self.steps = [
            ("setup", (), d0), (S, (), d0),
            ("update_vec", (q2, None, None), d2), (S, (), d2),
            ("update_vec", (None, l3, u3), d3), (S, (), d3),
            ("update_mat", (P4, None), d4), (S, (), d4),
            ("update_mat", (None, A5), d5),
            ("warm_start", (xw, None), d5), (S, (), d5),
            ("warm_start", (None, yw), d5), (S, (), d5),
            ("update_vec", (None, lbad, ubad), d5), (S, (), d5),
            ("update_mat", (-1e4 * c.P.data, None), None), ("solve_gone", (), None),
            ("setup", (), d0), (S, (), d0),
        ]
        self.expect_err = {13: 1, 15: 5}  # step index -> OSQP error code

    @staticmethod
    def _data(c, q=None, l=None, u=None, Px=None, Ax=None):
        P, A = c.P.copy(), c.A.copy()
        if Px is not None:
            P.data = np.asarray(Px, dtype=np.float64).copy()
        if Ax is not None:
            A.data = np.asarray(Ax, dtype=np.float64).copy()
        return qp_cases.Case(c.name, P, c.q if q is None else q, A, c.l if l is None else l, c.u if u is None else u,
                             c.settings, c.tier)

    def run(self, backend):
        """backend: setup(case, settings), update_vec(q, l, u), update_mat(Px, Ax),
        warm_start(x, y) -> error code; solve() -> (x, y, info); solve_gone() -> anything.
        Returns one record per step: the error code or the solve's result."""
        s = qp_cases.settings_of(self.case)
        out = []
        for op, args, data in self.steps:
            if op == "setup":
                out.append(backend.setup(data, s))
            elif op == "solve":
                out.append(backend.solve())
            else:
                out.append(getattr(backend, op)(*args))
        return out


class OracleBackend:
    def __init__(self, variant="exact"):
        self.ses = _oracle().QpSession(variant)

    def setup(self, c, s):
        return self.ses.setup(c.P, c.q, c.A, c.l, c.u, s)

    def update_vec(self, q, l, u):
        return self.ses.update_vec(q, l, u)

    def update_mat(self, Px, Ax):
        return self.ses.update_mat(Px, Ax)

    def warm_start(self, x, y):
        return self.ses.warm_start(x, y)

    def solve(self):
        return self.ses.solve()

    def solve_gone(self):
        return self.ses.solve()


class SequenceRef:
    """The oracle's ten runs of a sequence: per solve step the exact build's
    result, the discrete keys of all ten and the spreads, as Reruns."""

    def __init__(self, name):
        o = _oracle()
        self.seq = Sequence(name)
        self.runs = []
        for variant, seed in [("exact", None), ("fast", None)] + [("exact", k) for k in SEEDS]:
            if seed is not None:
                o.set_jitter(kkt_rel=JITTER, seed=seed, variant=variant)
            try:
                self.runs.append(self.seq.run(OracleBackend(variant)))
            finally:
                if seed is not None:
                    o.set_jitter(variant=variant)
        self.exact = self.runs[0]
        self.solves = [k for k, (op, _, _) in enumerate(self.seq.steps) if op == "solve"]
        self.keys, self.spread = {}, {}
        for k in self.solves:
            x0, y0, i0 = self.exact[k]
            self.keys[k] = {tuple(r[k][2][f] for f in DISCRETE) for r in self.runs}
            sp_ = {"x": max(err_inf(r[k][0], x0) for r in self.runs), "y": max(err_inf(r[k][1], y0) for r in self.runs)}
            for f in ("rho", "prim_res", "dual_res"):
                sp_[f] = max(abs(r[k][2][f] - i0[f]) for r in self.runs)
            self.spread[k] = sp_

    @functools.lru_cache(maxsize=None)
    def star(self, k):
        return kkt_star_of(self.seq.steps[k][2], self.exact[k][1])


@functools.lru_cache(maxsize=None)
def sequence_ref(name):
    return SequenceRef(name)
