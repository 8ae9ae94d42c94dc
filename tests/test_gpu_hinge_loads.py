"""The ADMM segment's hinge-row phases against recorded bits (MI355X).

hinge_gather_seg, hinge_e and hinge_a (admm_segment() in csrc/sqp_kernel.hip)
issue a chunk's or a row's loads together, behind scheduling barriers, before
the first wait.  That changes the order of the loads and nothing else: every
expression and its order are those of the build before, so each case here
solves its workload and asks for the bits of that build, recorded in
tests/golden/segment_hinge_bits.npz: the trajectories with np.array_equal and
every Result field.

The fixture pins bits.  It is written on the GPU by
tests/golden/make_golden_segment_bits.py (which takes the cases from this file)
and is regenerated when the arithmetic of the solve changes on purpose, from a
build that the other suites have passed; a restructuring that is meant to keep
the arithmetic must reproduce it as it stands.

Shapes: the cases of tests/test_gpu_segment_cache.py that have hinge rows --
config C at batch 8, the 8-dof torso_right_arm (D = 8: the full octet, no
clamped term), problem 435 alone (hinge pack in HBM, A_HCT in LDS) and problem
833 alone (both in HBM) -- and config C at 3 waypoints, batch 4, problems 4..7:
two step pairs, so that the chunk table is short, with a problem that never has
a hinge row (the hinge phases' empty loops), one whose mean is below the 8 rows
of a chunk (partial chunks: the clamped, masked loads) and two with dozens to
hundreds of rows.

As in test_gpu_segment_cache.py a case proves something only if the segment runs
(layout()["seg_ok"]), some QP ran more than 25 iterations (check_termination =
25: the stand-alone hinge_a of a second pass) and some QP ended with
rho != rho0; every case asserts that from the QP trace.  A shape that misses one
gets another first_problem, never a weaker assertion.
"""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from trajopt_amd import abi, problems
from trajopt_amd.runtime import BatchTrustRegionSQP

pytestmark = pytest.mark.gpu

CHECK_TERMINATION = 25
H_CHUNK = 8  # kHChunk: hinge rows per chunk of hinge_gather_seg
GOLDEN = Path(__file__).resolve().parent / "golden" / "segment_hinge_bits.npz"

# id -> (config, batch, make_workload keywords)
CASES = {
    "C-8": ("C", 8, dict(first_problem=0)),
    "C-torso": ("C", 4, dict(robot="torso_right_arm", first_problem=0)),
    "C-435": ("C", 1, dict(first_problem=435)),
    "C-833": ("C", 1, dict(first_problem=833)),
    "C-n3": ("C", 4, dict(n_steps=3, first_problem=4)),
}
SHORT_CASE = "C-n3"
RESULT_FIELDS = [name for name, _ in abi.Result._fields_]


def solve(name):
    """(x, results, per-problem QP trace, layout) of case name."""
    cfg, batch, kw = CASES[name]
    wl = problems.make_workload(cfg, batch, **kw)
    s = BatchTrustRegionSQP(wl, device=0)
    s.enable_trace(512)
    x, res = s.optimize()
    tr = s.get_trace()
    lay = s.layout()
    s.close()
    return x, res, tr, lay


def result_arrays(name, x, res):
    """The fixture's entries of one case: x and one array per Result field."""
    out = {f"{name}/x": np.asarray(x)}
    for f in RESULT_FIELDS:
        vals = [getattr(r, f) for r in res]
        assert not any(isinstance(v, C.Array) for v in vals)
        out[f"{name}/{f}"] = np.array(vals)
    return out


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()  # raises if the HIP library is missing
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(CASES))
def test_hinge_phases_reproduce_recorded_bits(golden, name):
    x, res, tr, lay = solve(name)
    assert lay["seg_ok"] == 1, f"{name}: not on the segment ({lay}), the case is vacuous"
    for b, t in enumerate(tr):
        assert len(t) == res[b].n_qp_solves, f"{name}: problem {b}'s QP trace is cut short ({len(t)} records)"
    qps = [rec for t in tr for rec in t]
    assert any(rec[2] > CHECK_TERMINATION for rec in qps), f"{name}: no QP of more than 25 iterations"
    assert any(rec[5] != rec[1] for rec in qps), f"{name}: no QP that ended with rho != rho0"
    assert any(r.n_hinge_admm > 0 for r in res), f"{name}: no hinge row at all"
    if name == SHORT_CASE:
        mean_rows = [r.n_hinge_admm / max(r.n_admm_iters, 1) for r in res]
        assert any(r.n_hinge_admm == 0 for r in res), f"{name}: every problem has hinge rows ({mean_rows})"
        assert any(0 < m < H_CHUNK for m in mean_rows), f"{name}: no problem with a chunk of fewer than 8 rows ({mean_rows})"
    got = result_arrays(name, x, res)
    assert set(got) == {k for k in golden if k.startswith(name + "/")}, f"{name}: the fixture's entries differ"
    gx = golden[f"{name}/x"]
    assert x.shape == gx.shape and np.array_equal(x, gx), f"{name}: max |x - x recorded| = {np.abs(x - gx).max():.3e}"
    for f in RESULT_FIELDS:
        g, v = golden[f"{name}/{f}"], got[f"{name}/{f}"]
        assert g.dtype == v.dtype and np.array_equal(g, v), f"{name}: Result.{f} differs: {v} vs recorded {g}"
