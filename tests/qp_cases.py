"""A catalogue of seeded QPs for the direct tests of the generic QP kernel
(csrc/qp_csc.hip) against the OSQP oracle.

    minimise 1/2 x'Px + q'x   subject to   l <= A x <= u

Every entry is a `Case`: P (upper-triangular scipy CSC), q, A (CSC), l, u,
overrides of abi.default_osqp_settings(), the storage tier thip_qp_create must
choose for its pattern and the OSQP status (and setup error) it must end with.
Beside "solved" the catalogue holds primal infeasible (3), dual infeasible (5),
max iterations (7), solved inaccurate (2), a failed polish (polish_status -1)
and the setup errors 1 and 5.  Pure numpy / scipy: tests/test_qp_cases.py proves the catalogue on the CPU
oracle (the statuses, the stability rule, a long-double reference) before
tests/test_gpu_qp_direct.py runs the device against it.

Tiers (thip_qp_create): 1 the whole factor staged in LDS with 16-bit indices,
2 only the solve vector in LDS (N = n + m <= 8192, the factor in HBM), 3 the
solve vector in HBM (N > 8192).  The shapes are the smallest that reach each
path: tier 2 needs about 20 k entries of L (a dense P of n = 160 under 40
dense rows), tier 3 needs N > 8192 and keeps 610 dense 7 x 7 blocks coupled
by one row per neighbouring pair, through the variable the minimum-degree
order takes last in each block, so that the elimination tree -- the serial
depth of every solve -- has 617 levels instead of 4271.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

INF = 1e30  # OSQP_INFTY


@dataclass
class Case:
    name: str
    P: sp.csc_matrix
    q: np.ndarray
    A: sp.csc_matrix
    l: np.ndarray
    u: np.ndarray
    settings: dict = field(default_factory=dict)
    tier: int = 1
    status: int = 1       # OSQP status; -1: osqp_setup fails with setup_error
    setup_error: int = 0
    polish: int = None    # polish_status the solve must end with (None: 1 when a solved case polishes, else 0)

    @property
    def polish_status(self):
        if self.polish is not None:
            return self.polish
        return 1 if self.status == 1 and self.settings.get("polishing", 1) else 0

    @property
    def n(self):
        return self.P.shape[0]

    @property
    def m(self):
        return self.A.shape[0]

    @property
    def solved(self):
        return self.status == 1

    def with_settings(self, name, **over):
        return Case(name, self.P, self.q, self.A, self.l, self.u, {**self.settings, **over}, self.tier, self.status,
                    self.setup_error, self.polish)


def settings_of(case, **over):
    """abi.OsqpSettings of a case: the reference's defaults and the case's overrides."""
    from trajopt_amd import abi

    s = abi.default_osqp_settings()
    for k, v in {**case.settings, **over}.items():
        assert hasattr(s, k), k
        setattr(s, k, v)
    return s


def _csc(M, shape=None):
    """CSC with sorted indices that keeps explicit zeros out and int32 indices."""
    M = sp.csc_matrix(M, shape=shape, dtype=np.float64)
    M.eliminate_zeros()
    M.sort_indices()
    M.indptr = M.indptr.astype(np.int32)
    M.indices = M.indices.astype(np.int32)
    return M


def _triu(Pd):
    return _csc(sp.triu(sp.csc_matrix(Pd)))


def _spd(rng, n, shift=1.0):
    M = rng.normal(size=(n, n))
    return M @ M.T / n + shift * np.eye(n)


# ------------------------------------------------------------------ tier 1
def _n1m1():
    # minimise x^2 - x under -0.2 <= x <= 0.2: x = 0.2, y = 0.6
    return Case("n1m1", _csc([[2.0]]), np.array([-1.0]), _csc([[1.0]]), np.array([-0.2]), np.array([0.2]))


def _n5m0():
    rng = np.random.default_rng(50)
    return Case("n5m0", _triu(_spd(rng, 5)), rng.normal(size=5), _csc(np.zeros((0, 5)), shape=(0, 5)), np.zeros(0),
                np.zeros(0))


def _mixed(name, seed, n, m0, pscale=1.0):
    """m0 random rows over the n box rows: the first two random rows are
    equalities, the next two free, then one-sided rows alternate with ranges.
    A small pscale makes ADMM slow enough for rho to adapt."""
    rng = np.random.default_rng(seed)
    Pd = _spd(rng, n) * pscale
    R = rng.normal(size=(m0, n)) * (rng.random((m0, n)) < 0.5)
    R[np.arange(m0), rng.integers(0, n, m0)] += 1.0  # no empty row
    A = np.vstack([R, np.eye(n)])
    x0 = rng.normal(size=n) * 0.3
    c = R @ x0
    lo = np.concatenate([c - rng.uniform(0.05, 0.5, m0), np.full(n, -1.0)])
    up = np.concatenate([c + rng.uniform(0.05, 0.5, m0), np.full(n, 1.0)])
    lo[0:2] = up[0:2] = c[0:2]          # equalities
    lo[2:4], up[2:4] = -INF, INF        # free rows
    lo[4:m0:2] = -INF                   # upper bound only
    if m0 > 5:
        up[5] = INF                     # lower bound only
    return Case(name, _triu(Pd), rng.normal(size=n) * 2, _csc(A), lo, up)


def _lp():
    # empty P: minimise c'x over the box and three range rows
    rng = np.random.default_rng(31)
    n = 6
    R = rng.normal(size=(3, n))
    A = np.vstack([R, np.eye(n)])
    lo = np.concatenate([np.full(3, -1.0), np.full(n, -1.0)])
    up = np.concatenate([np.full(3, 1.0), np.full(n, 1.0)])
    return Case("lp", _csc(np.zeros((n, n))), rng.normal(size=n), _csc(A), lo, up)


def _nodiag():
    # columns 1, 3 and 5 of P are empty (no diagonal entry: sigma alone is on the KKT diagonal)
    rng = np.random.default_rng(32)
    n = 7
    Pd = np.zeros((n, n))
    keep = [0, 2, 4, 6]
    Pd[np.ix_(keep, keep)] = _spd(rng, 4)
    R = rng.normal(size=(3, n))
    A = np.vstack([R, np.eye(n)])
    lo = np.concatenate([np.full(3, -0.5), np.full(n, -1.0)])
    up = np.concatenate([np.full(3, 0.5), np.full(n, 1.0)])
    return Case("nodiag", _triu(Pd), rng.normal(size=n), _csc(A), lo, up)


def _empty_row_col():
    # column 2 and row 1 of A are empty (x2 is free of constraints, row 1 reads 0 in [-1, 1])
    rng = np.random.default_rng(33)
    n, m = 5, 6
    A = rng.normal(size=(m, n))
    A[:, 2] = 0.0
    A[1, :] = 0.0
    return Case("empty_row_col", _triu(_spd(rng, n)), rng.normal(size=n), _csc(A, shape=(m, n)), np.full(m, -1.0),
                np.full(m, 1.0))


# ------------------------------------------------------------------ tier 2
def _tier2(pscale=1.0):
    rng = np.random.default_rng(160)
    n, m0 = 160, 40
    Pd = _spd(rng, n) * pscale
    R = rng.normal(size=(m0, n)) / np.sqrt(n)
    A = np.vstack([R, np.eye(n)])
    x0 = rng.normal(size=n) * 0.2
    c = R @ x0
    lo = np.concatenate([c - rng.uniform(0.05, 0.3, m0), np.full(n, -0.5)])
    up = np.concatenate([c + rng.uniform(0.05, 0.3, m0), np.full(n, 0.5)])
    lo[:5] = up[:5] = c[:5]  # 5 equalities
    # from rho = 3 the solve adapts rho once: the factor in HBM is rebuilt inside the loop
    return Case("tier2", _triu(Pd), rng.normal(size=n), _csc(A), lo, up, dict(rho=3.0), tier=2)


# ------------------------------------------------------------------ tier 3
def _blocks(name, nb, seed, qscale, n_eq, settings, tier):
    """nb dense 7 x 7 blocks, the box rows, and one row x_last(k) - x_last(k + 1)
    per neighbouring pair, n_eq of them equalities.  The coupled variable of a
    block has the highest degree of it, so the minimum-degree order takes it
    last: the elimination tree is the chain of the nb coupled variables with a
    block hanging from each (nb + 7 levels), not one path through all 7 nb
    variables."""
    rng = np.random.default_rng(seed)
    bs = 7
    n = nb * bs
    blocks = [_spd(rng, bs) for _ in range(nb)]
    Pd = sp.block_diag(blocks, format="csc")
    rows = np.repeat(np.arange(nb - 1), 2)
    cols = np.stack([np.arange(nb - 1) * bs + bs - 1, np.arange(1, nb) * bs + bs - 1], axis=1).ravel()
    vals = np.tile([1.0, -1.0], nb - 1)
    Cpl = sp.csc_matrix((vals, (rows, cols)), shape=(nb - 1, n))
    A = sp.vstack([sp.identity(n, format="csc"), Cpl], format="csc")
    lo = np.concatenate([np.full(n, -1.0), np.full(nb - 1, -0.1)])
    up = np.concatenate([np.full(n, 1.0), np.full(nb - 1, 0.1)])
    if n_eq:
        eq = n + rng.choice(nb - 1, n_eq, replace=False)
        lo[eq] = up[eq] = rng.uniform(-0.05, 0.05, n_eq)
    return Case(name, _triu(Pd), rng.normal(size=n) * qscale, _csc(A), lo, up, settings, tier)


def _tier3():
    # 610 blocks (n = 4270), 50 equalities among the 609 coupling rows: N = 9149
    return _blocks("tier3", 610, 3, 2.0, 50, dict(polishing=0), 3)


def _polish_failed():
    # a steep q drives most variables into their bounds: the polished point does not
    # improve on the ADMM iterate and OSQP keeps the latter (polish_status -1)
    c = _blocks("polish_failed", 10, 1, 20.0, 0, {}, 1)
    c.polish = -1
    return c


# ------------------------------------------------------------------ statuses
def _primal_infeasible():
    # the rows x0 >= 1 and x0 <= -1
    n = 3
    A = np.array([[1.0, 0, 0], [1.0, 0, 0], [0, 1.0, 1.0]])
    return Case("primal_infeasible", _triu(np.eye(n)), np.ones(n), _csc(A), np.array([1.0, -INF, -1.0]),
                np.array([INF, -1.0, 1.0]), status=3)


def _dual_infeasible():
    # minimise -x0 with x0 >= 0 and an empty P
    n = 2
    A = np.eye(n)
    return Case("dual_infeasible", _csc(np.zeros((n, n))), np.array([-1.0, 0.0]), _csc(A), np.array([0.0, -1.0]),
                np.array([INF, 1.0]), status=5)


def _non_convex():
    # P = diag(1, -1), x1 under no constraint: the KKT matrix is not quasi-definite
    return Case("non_convex", _triu(np.diag([1.0, -1.0])), np.zeros(2), _csc(np.array([[1.0, 0.0]])), np.array([-1.0]),
                np.array([1.0]), status=-1, setup_error=5)


def _l_above_u():
    c = _n1m1()
    return Case("l_above_u", c.P, c.q, c.A, np.array([0.3]), np.array([0.2]), status=-1, setup_error=1)


def build():
    # 275 iterations and one rho update under the defaults; every settings variant
    # below takes another number of iterations or of rho updates
    mixed12 = _mixed("mixed12", 13, 12, 8, pscale=0.05)
    t3 = _tier3()
    t2 = _tier2()
    cases = [
        _n1m1(), _n5m0(), mixed12, _lp(), _nodiag(), _empty_row_col(),
        _mixed("odd53", 53, 23, 7),  # N = 53: no multiple of the wavefront or the workgroup
        t2, t2.with_settings("tier2_unpolished", polishing=0),
        t3, t3.with_settings("tier3_polished", polishing=1),
        _primal_infeasible(), _dual_infeasible(), _polish_failed(),
        Case("max_iter", mixed12.P, mixed12.q, mixed12.A, mixed12.l, mixed12.u, dict(max_iter=10), 1, 7),
        _non_convex(), _l_above_u(),
        # one settings branch each, on the n = 12 case
        mixed12.with_settings("mixed12_check0", check_termination=0, max_iter=400),
        # only the last iterate is checked, and it passes the tenfold tolerances alone
        Case("solved_inaccurate", mixed12.P, mixed12.q, mixed12.A, mixed12.l, mixed12.u,
             dict(check_termination=0, max_iter=200), 1, 2),
        mixed12.with_settings("mixed12_rho_interval30", adaptive_rho_interval=30),
        mixed12.with_settings("mixed12_no_adaptive_rho", adaptive_rho=0),
        mixed12.with_settings("mixed12_no_scaling", scaling=0),
        mixed12.with_settings("mixed12_alpha1", alpha=1.0),
        mixed12.with_settings("mixed12_unpolished", polishing=0),
    ]
    return {c.name: c for c in cases}


CASES = build()
SOLVED = [k for k, c in CASES.items() if c.status == 1]
