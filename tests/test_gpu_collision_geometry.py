"""The collision geometry's edge cases on every device kernel (MI355X).

All collision work on the device goes through collision_device.hpp
(sphere_prim_distance, swept_sphere_prim_distance with its box breakpoints and
candidates, self_sphere_distance / sseg_params, swept_lower_bound), and the
config C / E scenes of the other GPU tests only ever show it sphere centres
outside a primitive, centimetres away, in general position.  Here a point robot
(tests/geometry_cases.py: the sphere's centre is q) puts one case per problem of
a batch, so that each kernel runs the whole table in a launch:

  static     centres outside a face / edge / corner of a box (identity and rotated),
             inside nearest each of the six faces, at equal depth to two faces, on a
             face / edge / corner / the centre; on a sphere's centre, on a capsule's
             axis and end point, beyond each cap, beside the shaft; a capsule a == b
  swept      a == b, motions of 1e-7, closest at t = 0 / 1 / strictly inside, through
             the centre, in -> out and out -> in, wholly inside a box across a face
             switch, grazing an edge and a corner, parallel to a face (over it, past
             its edge, inside) and to a capsule's axis with the flat minimum's left end
             written down, a rotated box entered, crossed and left
  self       twobot: both still, one still, parallel (same / opposite direction,
             overlapping, disjoint), crossing, motions of 1e-3 and 1e-7
  threshold  margin 0.1, buffer 0.01: pairs of problems 1e-7 under and over the contact
             distance, static and swept, on a sphere, a (0.5, 0.01, 0.01) box and a
             capsule of length 1 (the loosest bounding spheres of swept_lower_bound)
  substate   4 LVS sub-states through a box, LVS_DISCRETE and LVS_CONTINUOUS

against tests/geometry_reference.py (long double, textbook SDFs, golden-section
search) at geometry_cases.TOL_*: distance 1e-12, the distance at the returned cast
time within 1e-12 of the minimum, a flat minimum's time within 1e-12 of its left
end, well-conditioned normals 1e-9, degenerate normals the stated convention
exactly; and against oracle.collision_rows under test_gpu_dropin._check_rows.  The
point chains go through thip_create as they are (a config C descriptor with the
chain and sphere table swapped, n_cart = 0): the fused kernel needs no arm.

Where a normal is neither stated nor well conditioned (a cast whose deepest point lies
on a face switch or touches an edge: the last bit of the point picks the face, and the
device contracts multiply-adds while the oracle does not -- box_inside_face_switch gave
the x face on the device and the y face on the oracle, distance and time equal to
1e-16), the row must carry one of the normals the point can take
(geometry_reference.near_normals), and the oracle comparison keeps keys, distance,
cc_time and counts (check_oracle).

What a kernel cannot express is listed in geometry_cases.py (the DISCRETE kinds
and thip_csets see one state; thip_terms_run shows a threshold only at the hinge).
Every threshold pair gives exactly (1, 0) contacts in all six kernels (for the kinds
that look at each waypoint on its own, the robot is far away at the second one).

Worst differences, device against reference, MI355X (each test prints its own; the
oracle's, on the CPU, in tests/test_geometry_reference.py):
  kernel                                   distance   time(*)   flat time  normal
  thip_eval_collision (coll_eval_kernel)   8.6e-17    3.5e-17   5.6e-17    3.3e-15
  thip_collision_rows (fused scan)         8.6e-17    3.5e-17   5.6e-17    3.3e-15
  thip_check_run (traj_check_kernel)       8.6e-17    3.5e-17   5.6e-17    -
  thip_csets_run (value = 10 - distance)   8.8e-16    -         -          2.2e-16
  thip_ccsets_run (value = 10 - distance)  9.5e-16    3.5e-17   5.6e-17    3.3e-15
  thip_terms_run (cost 20 (10 - distance)) 5.7e-14    -         -          -
(*) the reference distance at the returned cast time above the minimum.  No device
code changed: the module found no bug.
"""
import numpy as np
import pytest

import ccsets_model as cm
import geometry_cases as gc
import geometry_reference as gr
from test_gpu_dropin import _check_rows
from trajopt_amd import abi
from trajopt_amd.runtime import (BatchTrustRegionSQP, CollisionSets, ContinuousCollisionSets, TermEvaluator, TermValues,
                                 TrajectoryChecker)

pytestmark = pytest.mark.gpu

SUITE_IDS = [s[0] for s in gc.SUITES]


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


_WL, _ORACLE = {}, {}


def workload(label):
    if label not in _WL:
        _, cases, kind, desc_kw, _ = next(s for s in gc.SUITES if s[0] == label)
        _WL[label] = gc.make_workload(cases, kind, **desc_kw)
    return _WL[label]


def oracle_rows(oracle_mod, label):
    """The oracle's rows of a suite, made once and shared (never modified)."""
    if label not in _ORACLE:
        wl = workload(label)
        _ORACLE[label] = [oracle_mod.collision_rows(wl, b, wl.init[b]) for b in range(wl.batch)]
        for r in _ORACLE[label]:
            r.setflags(write=False)
    return _ORACLE[label]


def twice(run):
    """Two runs, the same bytes."""
    a, b = run(), run()
    flat = lambda o: b"".join(np.ascontiguousarray(v).tobytes() for v in o)  # noqa: E731
    assert flat(a) == flat(b), "two runs differ"
    return a


def check_oracle(rows, ref, loose, label):
    """A problem's records against the oracle's under _check_rows' tolerances.  The contacts
    in `loose` (row indices: a normal neither stated nor well conditioned, e.g. the deepest
    point of a cast sitting on a face switch, where the last bit of the point picks the face
    and the device contracts multiply-adds while the oracle does not) are compared in their
    keys, distance, cc_time and count; their rows are held to the normals the point can take
    by geometry_cases.check_rows."""
    assert rows.shape == ref.shape, f"{label}: {len(rows)} contact rows vs {len(ref)}"
    keep = np.array([k not in loose for k in range(len(rows))], dtype=bool)
    _check_rows(rows[keep], ref[keep], label)
    if not keep.all():
        W = rows.shape[1]
        cut = lambda r: np.concatenate([r[~keep][:, :7], np.zeros((int((~keep).sum()), W - 7))], axis=1)  # noqa: E731
        _check_rows(cut(rows), cut(ref), label + " (keys, distance, cc_time)")


def pairs_ok(counts):
    assert list(counts) == [1, 0] * (len(counts) // 2), f"threshold pairs: {list(counts)}"


# ------------------------------------------------------------------ thip_eval_collision
@pytest.mark.parametrize("suite", gc.SUITES, ids=SUITE_IDS)
def test_eval_collision(oracle_mod, suite):
    """coll_eval_kernel: count, keys, distance, cc_time and the normal read off the row
    against the reference; the full records against the oracle's."""
    label, cases, kind, _, check_kw = suite
    wl = workload(label)
    ev = TermEvaluator(wl)
    try:
        rows = twice(lambda: ev.collision(0, wl.init))
    finally:
        ev.close()
    loose = []
    worst = gc.check_rows(rows, cases, kind, label=f"eval/{label}/", loose=loose, **check_kw)
    print(f"thip_eval_collision {label}: worst vs reference {worst}; loose normals {[cases[b]['name'] for b, _ in loose]}")
    for b, ref in enumerate(oracle_rows(oracle_mod, label)):
        check_oracle(rows[b], ref, {k for p, k in loose if p == b}, f"eval/{label}/{cases[b]['name']} vs oracle")
    if check_kw.get("threshold"):
        pairs_ok([len(r) for r in rows])


# ------------------------------------------------------------------ thip_collision_rows
@pytest.mark.parametrize("suite", gc.SUITES, ids=SUITE_IDS)
def test_fused_collision_rows(oracle_mod, suite):
    """The fused kernel's contact scan (coll_rows_kernel; the casts behind
    swept_lower_bound) on the point chains: the reference, the oracle's records and the
    evaluator's."""
    label, cases, kind, _, check_kw = suite
    wl = workload(label)
    s = BatchTrustRegionSQP(wl)
    try:
        fused = twice(lambda: s.collision_rows(wl.init))
    finally:
        s.close()
    ev = TermEvaluator(wl)
    try:
        rows = ev.collision(0, wl.init)
    finally:
        ev.close()
    loose = []
    worst = gc.check_rows(fused, cases, kind, label=f"fused/{label}/", loose=loose, **check_kw)
    print(f"thip_collision_rows {label}: worst vs reference {worst}")
    for b, ref in enumerate(oracle_rows(oracle_mod, label)):
        _check_rows(fused[b], rows[b], f"fused/{label}/{cases[b]['name']} vs evaluator")
        check_oracle(fused[b], ref, {k for p, k in loose if p == b}, f"fused/{label}/{cases[b]['name']} vs oracle")
    if check_kw.get("threshold"):
        pairs_ok([len(r) for r in fused])


# ------------------------------------------------------------------ thip_check_run
def run_checker(wl, kind, lvs=gc.ONE_CAST, margin=0.0):
    chk = TrajectoryChecker(wl.desc, wl.batch, wl.scene, abi.CheckConfig(kind, lvs, margin, 0, -1))
    try:
        return twice(lambda: [bytes((abi.CheckResult * wl.batch)(*chk.run(wl.init)))])[0]
    finally:
        chk.close()


def check_results(raw, n):
    return list((abi.CheckResult * n).from_buffer_copy(raw))


CHECKS = [("static", abi.CHECK_DISCRETE, "static-discrete", 2), ("swept", abi.CHECK_LVS_CONTINUOUS, "swept-one-cast", 2),
          ("self", abi.CHECK_LVS_CONTINUOUS, "self-one-cast", 2), ("self-static", abi.CHECK_DISCRETE, "self-discrete", 2),
          ("substate", abi.CHECK_LVS_CONTINUOUS, "substate-cast", 4)]


@pytest.mark.parametrize("name,kind,label,n_states", CHECKS, ids=[c[0] for c in CHECKS])
def test_checker(name, kind, label, n_states):
    """traj_check_kernel at margin 0: min_distance, where it is, min_cc_time and found."""
    _, cases, _, desc_kw, _ = next(s for s in gc.SUITES if s[0] == label)
    wl = workload(label)
    res = check_results(run_checker(wl, kind, desc_kw.get("lvs", gc.ONE_CAST)), wl.batch)
    worst = dict(distance=0.0, time=0.0, flat_time=0.0)
    for c, r in zip(cases, res):
        units = gc.units_of(c, kind, n_states)
        dist = [gc.ref_static(c, u[2])[0] if u[3] is None else gc.ref_cast(c, *u[3])[0] for u in units]
        # the units within 1e-9 of the minimum: the device may name any of them, and the
        # earliest when they tie exactly
        dmin = min(dist)
        near = [i for i, d in enumerate(dist) if float(d - dmin) <= 1e-9]
        named = [i for i in near if (units[i][0], units[i][1]) == (r.min_t, r.min_substate)]
        assert named, (c["name"], r.min_t, r.min_substate, [float(d) for d in dist])
        k = named[0]
        if all(dist[i] == dmin for i in near):
            assert k == near[0], (c["name"], "an exact tie goes to the earlier unit")
        d_ref = dist[k]
        t, sub, state, cast = units[k]
        dd = abs(float(gr.LD(r.min_distance) - d_ref))
        worst["distance"] = max(worst["distance"], dd)
        assert dd <= gc.TOL_DIST, (c["name"], r.min_distance, float(d_ref))
        other = -2 if c["prim"] is None else 0
        assert (r.min_t, r.min_link, r.min_other, r.min_sphere, r.min_substate) == (t, 3, other, 0, sub), c["name"]
        assert r.n_candidates == len(units)
        assert all(abs(float(d)) > 1e-9 for d in dist), "ambiguous verdict"
        assert r.found == int(float(d_ref) < 0), c["name"]
        assert r.n_contacts == sum(float(d) < 0 for d in dist), c["name"]
        if cast is None:
            assert r.min_cc_time == 0.0
            continue
        ts = r.min_cc_time * (n_states - 1) - sub
        assert 0.0 <= ts <= 1.0
        if c["t_left"] is not None and n_states == 2:
            worst["flat_time"] = max(worst["flat_time"], abs(ts - c["t_left"]))
            assert abs(ts - c["t_left"]) <= gc.TOL_TIME, (c["name"], ts)
        dt = abs(float(gc.ref_at(c, ts, *cast)[0] - d_ref))
        worst["time"] = max(worst["time"], dt)
        assert dt <= gc.TOL_TIME, (c["name"], ts)
    print(f"thip_check_run {name}: worst vs reference {worst}")


@pytest.mark.parametrize("kind,label", [(abi.CHECK_DISCRETE, "threshold-static"),
                                        (abi.CHECK_LVS_CONTINUOUS, "threshold-static-as-cast"),
                                        (abi.CHECK_LVS_CONTINUOUS, "threshold-swept")],
                         ids=["static", "static-as-cast", "swept"])
def test_checker_threshold(kind, label):
    """A candidate is a contact when its distance < margin: margin = 0.1 + 0.01."""
    wl = workload(label)
    res = check_results(run_checker(wl, kind, margin=gc.THRESHOLD), wl.batch)
    pairs_ok([r.n_contacts for r in res])
    assert [r.found for r in res] == [1, 0] * (wl.batch // 2)


# ------------------------------------------------------------------ thip_csets_run
def _stated_or_reference(c, got, n_ref, p, worst, exact):
    """A unit vector the device gives against the stated convention (exactly) or the
    reference's gradient direction (1e-9, where well conditioned)."""
    if c["normal"] is not None and exact:
        assert np.array_equal(got, np.array(c["normal"])), (c["name"], got)
    elif n_ref is not None and gc.well_conditioned(c, p):
        dn = float(np.abs(got - n_ref.astype(np.float64)).max())
        worst["normal"] = max(worst["normal"], dn)
        assert dn <= gc.TOL_NORMAL, (c["name"], got, n_ref)
    else:
        return False
    return True


def run_csets(wl, margin, buffer):
    cs = CollisionSets(wl.desc, wl.batch, wl.scene, abi.CsetsConfig(margin, gc.COEFF, buffer, 1, 0, 0))
    try:
        return twice(lambda: cs.run(wl.init))
    finally:
        cs.close()


@pytest.mark.parametrize("label", ["static-discrete", "self-discrete"])
def test_discrete_sets(label):
    """csets_kernel, R = 1, node 0: on a single pair the value is margin - distance and
    the row the normal (a self pair with both links moved: half of it on each side)."""
    _, cases, _, _, _ = next(s for s in gc.SUITES if s[0] == label)
    wl = workload(label)
    values, jac, coeffs, counts, keys = run_csets(wl, gc.BIG_MARGIN, 0.0)
    worst = dict(value=0.0, normal=0.0)
    for b, c in enumerate(cases):
        d_ref, n_ref = gc.ref_static(c)
        assert counts[b, 0] == 1 and coeffs[b, 0, 0] == gc.COEFF
        dv = abs(float(gr.LD(values[b, 0, 0]) - (gr.LD(gc.BIG_MARGIN) - d_ref)))
        worst["value"] = max(worst["value"], dv)
        assert dv <= gc.TOL_DIST, (c["name"], values[b, 0, 0])
        if c["prim"] is None:
            assert list(keys[b, 0, 0]) == [3, -7, 0, 1]
            assert np.abs(jac[b, 0, 0, :3] + jac[b, 0, 0, 3:]).max() <= 1e-15
            _stated_or_reference(c, 2.0 * jac[b, 0, 0, :3], n_ref, c["a"], worst, True)
        else:
            assert list(keys[b, 0, 0]) == [3, 0, 0, -1]
            _stated_or_reference(c, jac[b, 0, 0], n_ref, c["a"], worst, True)
    print(f"thip_csets_run {label}: worst vs reference {worst}")


def test_discrete_sets_threshold():
    wl = workload("threshold-static")
    values, jac, coeffs, counts, keys = run_csets(wl, gc.THR_MARGIN, gc.THR_BUFFER)
    pairs_ok(counts[:, 0])
    for b, c in enumerate(gc.THRESHOLD_STATIC_ALONE):
        want = gc.THR_MARGIN - float(gc.ref_static(c)[0]) if c["contacts"] else -gc.THR_BUFFER
        assert abs(values[b, 0, 0] - want) <= gc.TOL_DIST, (c["name"], values[b, 0, 0])


# ------------------------------------------------------------------ thip_ccsets_run
def run_ccsets(wl, etype, margin, buffer, lvs=gc.ONE_CAST):
    cfg = abi.CcsetsConfig(margin, gc.COEFF, buffer, 1, 0, 1, etype, lvs)
    cs = ContinuousCollisionSets(wl.desc, wl.batch, wl.scene, cfg)
    try:
        return cfg, twice(lambda: cs.run(wl.init))
    finally:
        cs.close()


def against_restatement(oracle_mod, wl, cfg, got, cases, loose=()):
    """The rows against tests/ccsets_model.py over the oracle's geometry (1e-12); the
    problems in `loose` (check_oracle's contacts) in their value, count, key and coefficient."""
    worst = 0.0
    for b, c in enumerate(cases):
        exp = cm.expected(oracle_mod, wl.desc, wl.scene[b], wl.init[b], cfg)[0][0]
        assert got[3][b, 0] == exp[3] and np.array_equal(got[4][b, 0], exp[4]), c["name"]
        worst = max(worst, float(np.abs(got[0][b, 0] - exp[0]).max()))
        assert np.abs(got[0][b, 0] - exp[0]).max() <= 1e-12, c["name"]
        assert np.array_equal(got[2][b, 0], exp[2])
        if b not in loose:
            worst = max(worst, float(np.abs(got[1][b, 0] - exp[1]).max()))
            assert np.abs(got[1][b, 0] - exp[1]).max() <= 1e-12, c["name"]
    return worst


@pytest.mark.parametrize("label", ["swept-one-cast", "static-as-cast", "self-one-cast"])
def test_continuous_sets_one_cast(oracle_mod, label):
    """ccsets_kernel, CONTINUOUS, R = 1: value = margin - the cast's distance; the two ends'
    rows are (1 - t) n and t n, so their sum is the normal and their ratio the cast time."""
    _, cases, _, _, _ = next(s for s in gc.SUITES if s[0] == label)
    wl = workload(label)
    cfg, got = run_ccsets(wl, cm.CONTINUOUS, gc.BIG_MARGIN, 0.0)
    values, jac, coeffs, counts, keys = got
    worst = dict(value=0.0, time=0.0, flat_time=0.0, normal=0.0)
    loose = set()
    for b, c in enumerate(cases):
        d_ref, _ = gc.ref_cast(c)
        assert counts[b, 0] == 1 and coeffs[b, 0, 0] == gc.COEFF
        dv = abs(float(gr.LD(values[b, 0, 0]) - (gr.LD(gc.BIG_MARGIN) - d_ref)))
        worst["value"] = max(worst["value"], dv)
        assert dv <= gc.TOL_DIST, (c["name"], values[b, 0, 0])
        if c["prim"] is None:
            assert list(keys[b, 0, 0]) == [3, -7, 0, 1]
            continue  # (the sides' times can differ: the rows are checked against the restatement)
        assert list(keys[b, 0, 0]) == [3, 0, 0, -1]
        j0, j1 = jac[b, 0, 0, 0], jac[b, 0, 0, 1]
        n = j0 + j1
        ts = float(np.linalg.norm(j1) / (np.linalg.norm(j0) + np.linalg.norm(j1)))
        assert abs(np.linalg.norm(n) - 1.0) <= 1e-12, (c["name"], n)
        if c["t_left"] is not None:
            worst["flat_time"] = max(worst["flat_time"], abs(ts - c["t_left"]))
            assert abs(ts - c["t_left"]) <= gc.TOL_TIME, (c["name"], ts)
        d_at, n_ref, _ = gc.ref_at(c, ts)
        worst["time"] = max(worst["time"], abs(float(d_at - d_ref)))
        assert abs(float(d_at - d_ref)) <= gc.TOL_TIME, (c["name"], ts)
        p = c["a"].astype(gr.LD) + gr.LD(ts) * (c["b"].astype(gr.LD) - c["a"].astype(gr.LD))
        # (a stated normal: up to the rounding of (1 - t) n + t n)
        if c["normal"] is not None:
            assert np.abs(n - np.array(c["normal"])).max() <= 2.5e-16, (c["name"], n)
        elif not _stated_or_reference(c, n, n_ref, p, worst, False):
            loose.add(b)
            can = gr.near_normals(p, c["prim"])
            assert can is None or min(np.abs(n - v.astype(np.float64)).max() for v in can) <= gc.TOL_NORMAL, (c["name"], n)
    rest = against_restatement(oracle_mod, wl, cfg, got, cases, loose)
    print(f"thip_ccsets_run CONTINUOUS {label}: worst vs reference {worst}, vs the restatement {rest:.3e}")


@pytest.mark.parametrize("label", ["swept-ends", "self-ends"])
def test_continuous_sets_lvs_discrete(oracle_mod, label):
    """ccsets_kernel, LVS_DISCRETE with the two end states: value = margin - the smaller of
    the ends' distances; end e's row is the normal at waypoint e."""
    _, cases, _, _, _ = next(s for s in gc.SUITES if s[0] == label)
    wl = workload(label)
    cfg, got = run_ccsets(wl, cm.LVS_DISCRETE, gc.BIG_MARGIN, 0.0)
    values, jac, coeffs, counts, keys = got
    worst = dict(value=0.0, normal=0.0)
    loose = set()
    for b, c in enumerate(cases):
        ends = [gc.ref_static(c, c["a"]), gc.ref_static(c, c["b"])]
        d_ref = min(ends[0][0], ends[1][0])
        assert counts[b, 0] == 1
        dv = abs(float(gr.LD(values[b, 0, 0]) - (gr.LD(gc.BIG_MARGIN) - d_ref)))
        worst["value"] = max(worst["value"], dv)
        assert dv <= gc.TOL_DIST, (c["name"], values[b, 0, 0])
        for e, p in enumerate((c["a"], c["b"])):
            row = jac[b, 0, 0, e]
            if c["prim"] is None:
                assert np.abs(row[:3] + row[3:]).max() <= 1e-15
                row = 2.0 * row[:3]
            if not _stated_or_reference(c, row, ends[e][1], p, worst, False):
                loose.add(b)
    rest = against_restatement(oracle_mod, wl, cfg, got, cases, loose)
    print(f"thip_ccsets_run LVS_DISCRETE {label}: worst vs reference {worst}, vs the restatement {rest:.3e}")


@pytest.mark.parametrize("label,etype", [("threshold-swept", cm.CONTINUOUS), ("threshold-static-as-cast", cm.CONTINUOUS),
                                         ("threshold-static", cm.LVS_DISCRETE)],
                         ids=["swept-continuous", "static-continuous", "static-lvs_discrete"])
def test_continuous_sets_threshold(label, etype):
    """The pre-filtered casts (swept_lower_bound) and the end states (of the static pairs:
    a swept pair's ends are beyond the threshold): exactly (1, 0) sets."""
    _, cases, _, _, _ = next(s for s in gc.SUITES if s[0] == label)
    wl = workload(label)
    cfg, (values, jac, coeffs, counts, keys) = run_ccsets(wl, etype, gc.THR_MARGIN, gc.THR_BUFFER)
    pairs_ok(counts[:, 0])
    for b, c in enumerate(cases):
        d = gc.ref_static(c)[0] if c["family"] == "threshold_static" else gc.ref_cast(c)[0]
        want = gc.THR_MARGIN - float(d) if c["contacts"] else -gc.THR_BUFFER
        assert abs(values[b, 0, 0] - want) <= gc.TOL_DIST, (c["name"], values[b, 0, 0])


# ------------------------------------------------------------------ thip_terms_run
def run_terms(wl):
    tv = TermValues(wl)
    try:
        slots = [i for i, s in enumerate(tv.slots) if s.kind == abi.TERM_COLL]
        units = [tv.slots[i].unit for i in slots]
        assert all(not tv.slots[i].is_cnt for i in slots)
        costs, _ = twice(lambda: tv.run(wl.init))
        return costs[:, slots], units
    finally:
        tv.close()


@pytest.mark.parametrize("label", [s for s in SUITE_IDS if not s.startswith("threshold")])
def test_term_values(oracle_mod, label):
    """coll_values_kernel: the collision slots' costs against the same sum over the oracle's
    rows (tests/test_gpu_terms.py numpy_slots: coeff * max(margin - distance, 0) per contact)
    and over the reference's distances."""
    _, cases, kind, _, check_kw = next(s for s in gc.SUITES if s[0] == label)
    wl = workload(label)
    costs, units = run_terms(wl)
    worst = dict(oracle=0.0, reference=0.0)
    n_states = check_kw.get("n_states", 2)
    for b, c in enumerate(cases):
        rows = oracle_rows(oracle_mod, label)[b]
        for k, t in enumerate(units):
            r = rows[rows[:, 0].astype(int) == t]
            want = sum(gc.COEFF * max(gc.BIG_MARGIN - row[5], 0.0) for row in r)
            tol = 1e-12 * max(1, len(r)) * gc.COEFF  # test_gpu_terms.slot_tols
            worst["oracle"] = max(worst["oracle"], abs(costs[b, k] - want))
            assert abs(costs[b, k] - want) <= tol, (c["name"], t, costs[b, k], want)
            ref = [gc.ref_static(c, u[2])[0] if u[3] is None else gc.ref_cast(c, *u[3])[0]
                   for u in gc.units_of(c, kind, n_states) if u[0] == t]
            assert len(ref) == len(r) > 0
            want = float(sum(gr.LD(gc.COEFF) * (gr.LD(gc.BIG_MARGIN) - d) for d in ref))
            worst["reference"] = max(worst["reference"], abs(costs[b, k] - want))
            assert abs(costs[b, k] - want) <= tol, (c["name"], t, costs[b, k], want)
    print(f"thip_terms_run {label}: worst {worst}")


@pytest.mark.parametrize("label", ["threshold-static", "threshold-static-as-cast", "threshold-swept"])
def test_term_values_threshold(label):
    """A cost shows a contact only through its hinge, so the pairs are probed at the hinge's
    own threshold: margin 0.1 + 0.01 and no buffer give coeff * 1e-7 against exactly 0.  With
    the family's margin 0.1 and buffer 0.01 both problems of a pair cost exactly 0."""
    _, cases, kind, _, _ = next(s for s in gc.SUITES if s[0] == label)
    costs, _ = run_terms(workload(label))
    assert not costs.any()
    costs, units = run_terms(gc.make_workload(cases, kind, margin=gc.THRESHOLD, buffer=0.0))
    for b, c in enumerate(cases):
        for k in range(len(units)):
            if c["contacts"] and k == 0:
                assert abs(costs[b, k] - gc.COEFF * gc.EPS) <= 1e-12 * gc.COEFF, (c["name"], costs[b, k])
            else:
                assert costs[b, k] == 0.0, (c["name"], costs[b, k])
