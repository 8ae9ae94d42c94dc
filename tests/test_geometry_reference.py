"""The oracle's collision geometry against the independent long-double reference
(tests/geometry_reference.py) over the whole case table (tests/geometry_cases.py),
on the CPU.  This module is what validates the table: an entry that fails here is
wrong and is corrected, not removed.  tests/test_gpu_collision_geometry.py runs
the same table through every device kernel.

Tolerances (geometry_cases.TOL_*): distances 1e-12 (the suite's tolerance for row
distances, tests/test_gpu_dropin.py _check_rows); a cast time with a unique
minimiser: the reference distance at the returned t within 1e-12 of the minimum;
a flat minimum: t within 1e-12 of the written left end; a well-conditioned normal
(centre at least 1e-3 from the closest point, the two smallest face depths at least
1e-3 apart) within 1e-9 of the gradient direction; a degenerate normal equal to the
stated convention exactly.

Worst differences measured, oracle against reference (printed by every test), 128
cases: distance 4.2e-17 (sphere_prim), 4.8e-17 (swept_sphere_prim), 8.6e-17
(collision_rows); the reference distance at the returned cast time above the minimum
3.5e-17; flat cast times 5.6e-17 from the written left end; normals 1.4e-15.
Mutating a copy of oracle/src/collision.cpp (the inside tie to `<=`, no face-switch
candidates, ties to the larger t, no mid-plane breakpoints) fails this module each time.
"""
import numpy as np
import pytest

import geometry_cases as gc
import geometry_reference as gr

LD = gr.LD
POINT = gc.STATIC + gc.SWEPT + gc.THRESHOLD_CASES + gc.SUBSTATE


# ------------------------------------------------------------------ the table itself
def test_table_has_every_family():
    names = [c["name"] for c in POINT + gc.SELF]
    assert len(names) == len(set(names))
    types = lambda cases: {int(c["prim"][0]) for c in cases}  # noqa: E731
    everything = {gc.abi.PRIM_SPHERE, gc.abi.PRIM_BOX, gc.abi.PRIM_CAPSULE}
    assert types(gc.STATIC) == types(gc.SWEPT) == types(gc.THRESHOLD_CASES) == everything
    for word in ("a_eq_b", "motion_1e-7", "closest_at_0", "closest_at_1", "closest_inside_cast", "through_",
                 "in_to_out", "out_to_in"):
        for prim in ("sphere", "capsule", "box"):
            assert any(word in n and n.startswith(prim) for n in names), (word, prim)
    for name in ("box_inside_face_switch", "box_grazing_edge_touch", "box_grazing_corner_touch", "box_parallel_over_face",
                 "box_parallel_past_edge", "box_parallel_inside", "capsule_parallel_over_shaft", "boxrot_entering",
                 "boxrot_crossing", "both_still", "a_still", "b_still", "parallel_same_direction",
                 "parallel_opposite_direction", "parallel_overlapping", "parallel_disjoint", "crossing", "motion_1e-3",
                 "motion_1e-7", "box_tie_xy_mx", "box_on_face_px", "box_on_edge_xy", "box_on_corner", "sphere_on_centre",
                 "capsule_on_axis", "capsule_a_eq_b_outside"):
        assert name in names, name
    assert len(gc.SUBSTATE) >= 1 and len(gc.THRESHOLD_STATIC) >= 2 and len(gc.THRESHOLD_SWEPT) >= 2


def test_exact_coordinates_are_exact():
    """What the degenerate cases rely on holds bitwise in double and in long double."""
    for c in gc.STATIC:
        if "tie" in c:
            i, j = c["tie"]
            for f in (np.float64, LD):
                depth = np.asarray(gc.H, dtype=f) - np.abs(c["a"].astype(f))
                assert depth[i] == depth[j] and depth[i] < np.delete(depth, [i, j])[0], (c["name"], depth)
        if c.get("depth0"):
            depth = np.asarray(gc.H) - np.abs(c["a"])
            assert depth.min() == 0.0, (c["name"], depth)
            assert gr.sdf(c["a"], c["prim"]) == 0
    R = gc.ROT.astype(LD)
    assert np.abs(R @ R.T - np.eye(3)).max() < 2e-16 and abs(np.linalg.det(gc.ROT) - 1.0) < 1e-15


def test_flat_minima_start_where_the_table_says():
    """t_left is the left end of the minimiser interval: the reference distance there is
    the minimum, stays there just after it, and is higher just before it."""
    for c in gc.SWEPT + gc.SELF:
        if c["t_left"] is None:
            continue
        dmin, _ = gc.ref_cast(c)
        tl = c["t_left"]
        assert abs(float(gc.ref_at(c, tl)[0] - dmin)) <= 1e-17, c["name"]
        if np.array_equal(c["a"][:3], c["b"][:3]):
            continue  # the sphere does not move: every t is the same point
        assert abs(float(gc.ref_at(c, min(tl + 1e-3, 1.0))[0] - dmin)) <= 1e-17, c["name"]
        if tl > 0:
            assert float(gc.ref_at(c, tl - 1e-6)[0] - dmin) > 1e-14, c["name"]


def test_threshold_pairs_straddle_the_threshold():
    for c in gc.THRESHOLD_CASES:
        d = gc.ref_static(c)[0] if c["family"] == "threshold_static" else gc.ref_cast(c)[0]
        assert abs(float(d - (LD(gc.THRESHOLD) + LD(c["offset"])))) <= 1e-14, (c["name"], float(d))
        assert (float(d) < gc.THRESHOLD) == bool(c["contacts"])


def test_self_casts_keep_their_distance():
    for c in gc.SELF:
        d, _ = gc.ref_cast(c)
        assert float(d) + gc.R_BOT + gc.R_BOT_B >= 0.05, c["name"]


# ------------------------------------------------------------------ the oracle's functions
def _check_normal(c, n, n_ref, p, worst):
    if c["normal"] is not None:
        assert n_ref is None or not gc.well_conditioned(c, p), f"{c['name']}: a convention where the gradient exists"
        assert np.array_equal(n, np.array(c["normal"])), f"{c['name']}: normal {n}, stated {c['normal']}"
    elif n_ref is not None and gc.well_conditioned(c, p):
        dn = float(np.abs(n - n_ref.astype(np.float64)).max())
        worst["normal"] = max(worst["normal"], dn)
        assert dn <= gc.TOL_NORMAL, f"{c['name']}: normal {n} vs {n_ref}"
        return True
    return False


def test_sphere_prim_against_the_reference(oracle_mod):
    worst = dict(distance=0.0, normal=0.0)
    compared = 0
    for c in gc.STATIC + gc.THRESHOLD_STATIC:
        d, n, pt = oracle_mod.sphere_prim(c["a"], gc.R_BOT, c["prim"])
        d_ref, n_ref = gc.ref_static(c)
        dd = abs(float(LD(d) - d_ref))
        worst["distance"] = max(worst["distance"], dd)
        assert dd <= gc.TOL_DIST, (c["name"], d, float(d_ref))
        compared += _check_normal(c, n, n_ref, c["a"], worst)
        assert np.abs(pt - (c["a"] + gc.R_BOT * n)).max() <= 1e-15
    print(f"sphere_prim vs reference: {worst}, {compared} normals compared")
    assert compared >= 25


def test_swept_sphere_prim_against_the_reference(oracle_mod):
    worst = dict(distance=0.0, time=0.0, flat_time=0.0, normal=0.0)
    compared = 0
    for c in gc.SWEPT + gc.THRESHOLD_SWEPT + gc.STATIC + gc.SUBSTATE:
        d, n, pt, t = oracle_mod.swept_sphere_prim(c["a"], c["b"], gc.R_BOT, c["prim"])
        d_ref, t_ref = gc.ref_cast(c)
        dd = abs(float(LD(d) - d_ref))
        worst["distance"] = max(worst["distance"], dd)
        assert dd <= gc.TOL_DIST, (c["name"], d, float(d_ref))
        assert 0.0 <= t <= 1.0
        if c["family"] == "static":
            assert t == 0.0, c["name"]
        elif c["t_left"] is not None:
            worst["flat_time"] = max(worst["flat_time"], abs(t - c["t_left"]))
            assert abs(t - c["t_left"]) <= gc.TOL_TIME, (c["name"], t)
        d_at, n_ref, _ = gc.ref_at(c, t)
        worst["time"] = max(worst["time"], abs(float(d_at - d_ref)))
        assert abs(float(d_at - d_ref)) <= gc.TOL_TIME, (c["name"], t, float(t_ref))
        p = c["a"].astype(LD) + LD(t) * (c["b"].astype(LD) - c["a"].astype(LD))
        compared += _check_normal(c, n, n_ref, p, worst)
    print(f"swept_sphere_prim vs reference: {worst}, {compared} normals compared")
    assert compared >= 50


# ------------------------------------------------------------------ the oracle's rows
@pytest.mark.parametrize("suite", gc.SUITES, ids=[s[0] for s in gc.SUITES])
def test_collision_rows_against_the_reference(oracle_mod, suite):
    """oracle.collision_rows on the point robots, every evaluator: count, keys, distance,
    cc_time and the normal read off the row (a_t + a_t+1 = -n on the point robot)."""
    label, cases, kind, desc_kw, check_kw = suite
    wl = gc.make_workload(cases, kind, **desc_kw)
    rows = [oracle_mod.collision_rows(wl, b, wl.init[b]) for b in range(wl.batch)]
    worst = gc.check_rows(rows, cases, kind, label=f"{label}/", **check_kw)
    print(f"{label}: oracle rows vs reference, worst {worst}")
    if check_kw.get("threshold"):
        assert [len(r) for r in rows] == [1, 0] * (len(cases) // 2)
