"""The batched trajectory checker (thip_check_*, traj_check.hip) on the GPU
against the oracle's collision_rows.

The witness: the descriptor rewritten as dropin_cases.continuous_check_found
does, but with coll_margin = 1e3, no buffer, no per-pair margins, no fixed
steps and contact test ALL, so that the oracle returns EVERY candidate with its
distance, in unit order and then ContactResultMap order.  Distances agree
within 1e-12 (test_gpu_dropin._check_rows' tolerance for distances); counts,
candidate numbers and first units agree exactly, with margins taken from gaps
of the oracle's sorted distances so rounding cannot move a candidate across."""
import ctypes as C
import functools

import numpy as np
import pytest

import dropin_cases as dc
from trajopt_amd import abi, problems
from trajopt_amd.runtime import BatchTrustRegionSQP, TrajectoryChecker

pytestmark = pytest.mark.gpu

TOL = 1e-12
KINDS = [abi.CHECK_LVS_DISCRETE, abi.CHECK_LVS_CONTINUOUS, abi.CHECK_DISCRETE]
LVS = 0.05  # 1 to 4 sub-states per step pair on the 6-waypoint workloads


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


def cfg(kind, lvs=LVS, margin=0.0, first=0, last=-1):
    return abi.CheckConfig(kind, lvs, margin, first, last)


def oracle_rows(oracle_mod, desc, scene, x, kind, lvs, first=0, last=-1):
    """Every candidate of trajectory x [N, D]: rows [n, 7] = t, link, other, sphere,
    sub-state, distance, cc_time."""
    d = abi.ProblemDesc.from_buffer_copy(desc)
    d.coll_enabled, d.coll_continuous, d.coll_lvs = 1, kind, lvs
    d.coll_margin, d.coll_buffer, d.n_coll_pairs, d.n_coll_extra = 1e3, 0.0, 0, 0
    d.coll_first_step, d.coll_last_step, d.coll_n_fixed = first, last, 0
    d.coll_contact_test = abi.CONTACT_ALL
    x = np.ascontiguousarray(x, dtype=np.float64)
    sc = np.ascontiguousarray(scene, dtype=np.float64)
    L = oracle_mod.lib()
    dp = C.POINTER(C.c_double)
    L.oracle_collision_rows_term.argtypes = [C.POINTER(abi.ProblemDesc), C.c_int, dp, dp, dp, C.c_int]
    L.oracle_collision_rows_term.restype = C.c_int
    W = 8 + 2 * d.chain.n_dof + 1
    out = np.zeros((1, W))
    n = L.oracle_collision_rows_term(C.byref(d), 0, sc.ctypes.data_as(dp), x.ctypes.data_as(dp), out.ctypes.data_as(dp), 0)
    assert n >= 0, L.oracle_last_error().decode()
    out = np.zeros((max(n, 1), W))  # cap = the candidate count
    m = L.oracle_collision_rows_term(C.byref(d), 0, sc.ctypes.data_as(dp), x.ctypes.data_as(dp), out.ctypes.data_as(dp), n)
    assert m == n
    return out[:n, :7].copy()


def run_checker(desc, scene, x, config):
    """Two runs of a fresh checker: results, unit minima, and both as bytes."""
    chk = TrajectoryChecker(desc, len(x), scene, config)
    try:
        res, um = chk.run(x, unit_min=True)
        raw = bytes((abi.CheckResult * len(res))(*res)) + um.tobytes()
        res2, um2 = chk.run(x, unit_min=True)
        assert bytes((abi.CheckResult * len(res2))(*res2)) + um2.tobytes() == raw, "two runs differ"
    finally:
        chk.close()
    return res, um


def agree(r, um, rows, first=0, counts_margin=None):
    """One problem's result against its oracle rows (the issue's agreement)."""
    dist = rows[:, 5]
    mn = dist.min()
    print(f"min_distance {r.min_distance!r} oracle {mn!r} diff {abs(r.min_distance - mn):.3e} rows {len(rows)}")
    assert abs(r.min_distance - mn) <= TOL
    # exact ties are real (two units share a waypoint): compare against the set
    near = {tuple(int(v) for v in row[:5]) for row in rows[np.abs(dist - mn) <= TOL]}
    assert (r.min_t, r.min_link, r.min_other, r.min_sphere, r.min_substate) in near
    assert 0.0 <= r.min_cc_time <= 1.0
    assert r.n_candidates == len(rows)
    ts = rows[:, 0].astype(int)
    for u in range(len(um)):
        du = dist[ts == first + u]
        assert len(du) and abs(um[u] - du.min()) <= TOL, (u, um[u])
    if counts_margin is not None:
        hit = dist < counts_margin
        assert r.n_contacts == int(hit.sum())
        assert r.found == (1 if hit.any() else 0)
        assert r.first_unit == (int(ts[hit].min()) if hit.any() else -1)


@functools.lru_cache(maxsize=None)
def workload(config):
    """(workload, trajectories): init and init + 0.03 N(0, 1), two problems each."""
    wl = problems.make_workload(config, 2, n_steps=6)
    rng = np.random.default_rng(7)
    return wl, (wl.init.copy(), wl.init + 0.03 * rng.standard_normal(wl.init.shape))


_ROWS = {}


def rows_of(oracle_mod, config, which, kind, b):
    key = (config, which, kind, b)
    if key not in _ROWS:
        wl, xs = workload(config)
        _ROWS[key] = oracle_rows(oracle_mod, wl.desc, wl.scene[b], xs[which][b], kind, LVS)
        _ROWS[key].setflags(write=False)
    return _ROWS[key]


# ------------------------------------------------------------------ 1. agreement
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", [0, 1], ids=["init", "perturbed"])
@pytest.mark.parametrize("config", ["C", "E"])
def test_agreement_with_oracle(oracle_mod, config, which, kind):
    wl, xs = workload(config)
    if config == "C":
        types = set(wl.scene[0][:, 0].astype(int))
        assert {abi.PRIM_SPHERE, abi.PRIM_BOX, abi.PRIM_CAPSULE} <= types
        assert wl.desc.n_prims == 10
    else:
        assert wl.n_dof == 14 and wl.desc.chain.is_tree and wl.desc.n_self_pairs == 37
    res, um = run_checker(wl.desc, wl.scene, xs[which], cfg(kind))
    for b in range(wl.batch):
        agree(res[b], um[b], rows_of(oracle_mod, config, which, kind, b))


# ------------------------------------------------------------------ 2. verdict and count
def gap_margin(dist, q=0.02):
    """Midpoint of the first gap >= 1e-9 of the sorted distances at or above the q quantile."""
    d = np.sort(dist)
    k = int(q * len(d))
    while d[k + 1] - d[k] < 1e-9:
        k += 1
    assert d[k + 1] - d[k] >= 1e-9 and k < 0.1 * len(d)
    return 0.5 * (d[k] + d[k + 1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("config", ["C", "E"])
def test_verdict_and_count(oracle_mod, config, kind):
    wl, xs = workload(config)
    lowest = np.inf
    for b in range(wl.batch):
        rows = rows_of(oracle_mod, config, 0, kind, b)
        lowest = min(lowest, rows[:, 5].min())
        m = gap_margin(rows[:, 5])
        res, um = run_checker(wl.desc, wl.scene, xs[0], cfg(kind, margin=m))
        assert res[b].n_contacts > 0
        agree(res[b], um[b], rows, counts_margin=m)
    res, _ = run_checker(wl.desc, wl.scene, xs[0], cfg(kind, margin=lowest - 1e-3))
    for r in res:
        assert (r.found, r.n_contacts, r.first_unit) == (0, 0, -1)


# ------------------------------------------------------------------ 3. penetration
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ptype", [abi.PRIM_SPHERE, abi.PRIM_BOX, abi.PRIM_CAPSULE], ids=["sphere", "box", "capsule"])
def test_penetration_is_found_in_its_own_problem_only(oracle_mod, ptype, kind):
    wl, xs = workload("C")
    x, t, s = xs[0], 3, 2
    d = wl.desc
    T = oracle_mod.fwd_kin(d.chain, x[0, t])[0, d.sphere_link[s]].reshape(3, 4)
    c = T[:, :3] @ np.array([d.sphere_center[s][i] for i in range(3)]) + T[:, 3]
    scene = wl.scene.copy()
    p = int(np.flatnonzero(scene[0][:, 0].astype(int) == ptype)[0])
    if ptype == abi.PRIM_CAPSULE:
        mid = 0.5 * (scene[0, p, 1:4] + scene[0, p, 4:7])
        scene[0, p, 1:4] += c - mid
        scene[0, p, 4:7] += c - mid
    else:
        scene[0, p, 1:4] = c
    res, um = run_checker(d, scene, x, cfg(kind, margin=0.0))
    rows = oracle_rows(oracle_mod, d, scene[0], x[0], kind, LVS)
    assert res[0].found == 1 and res[0].min_distance < 0
    agree(res[0], um[0], rows, counts_margin=None)
    # the count at margin 0, when no oracle distance is within rounding of it
    if np.abs(rows[:, 5]).min() > 1e-9:
        agree(res[0], um[0], rows, counts_margin=0.0)
    # the other problem's scene is untouched: nothing found there
    assert res[1].found == 0 and res[1].first_unit == -1
    agree(res[1], um[1], rows_of(oracle_mod, "C", 0, kind, 1), counts_margin=0.0)


# ------------------------------------------------------------------ 4. chunking
@pytest.mark.parametrize("kind", [abi.CHECK_LVS_CONTINUOUS, abi.CHECK_LVS_DISCRETE])
def test_step_pairs_longer_than_one_chunk(oracle_mod, kind):
    """A step pair with more sub-states than the kernel's chunk (THIP_CHECK_CHUNK
    sub-states' sphere centres in LDS at a time) loops over chunks."""
    wl, xs = workload("C")
    x = xs[1][:1]
    steps = np.linalg.norm(np.diff(x[0], axis=0), axis=1)
    lvs = float(steps.max() / (2.5 * abi.CHECK_CHUNK))  # 2.5 chunks in the longest pair
    rows = oracle_rows(oracle_mod, wl.desc, wl.scene[0], x[0], kind, lvs)
    n_sub = int(rows[:, 4].max()) + 1
    assert n_sub > 2 * abi.CHECK_CHUNK, n_sub
    assert len(rows) < 2e5
    m = gap_margin(rows[:, 5])
    res, um = run_checker(wl.desc, wl.scene[:1], x, cfg(kind, lvs=lvs, margin=m))
    agree(res[0], um[0], rows, counts_margin=m)


# ------------------------------------------------------------------ 5. beyond the LDS scene
@pytest.mark.parametrize("kind", [abi.CHECK_LVS_CONTINUOUS, abi.CHECK_DISCRETE])
def test_large_scene_and_long_horizon(oracle_mod, kind):
    """19 primitives (more than the THIP_MAX_PRIMS the kernel stages in LDS: read
    from global memory) and 100 waypoints (beyond THIP_MAX_STEPS)."""
    wl0 = problems.make_workload("C", 1, n_steps=100)
    far = np.zeros((16, 16))
    far[:, 0] = abi.PRIM_SPHERE
    far[:, 1:4] = np.array([3.0, 3.0, 3.0]) + 0.3 * np.arange(16)[:, None]
    far[:, 4] = 0.05
    scene = np.ascontiguousarray(np.concatenate([wl0.scene[0][:3], far]))[None]
    d = abi.ProblemDesc.from_buffer_copy(wl0.desc)
    d.n_prims = 19
    assert d.n_prims > abi.MAX_PRIMS and d.n_steps > abi.MAX_STEPS
    lvs = float("inf")  # one cast per step pair
    rows = oracle_rows(oracle_mod, d, scene[0], wl0.init[0], kind, lvs)
    m = gap_margin(rows[:, 5])
    res, um = run_checker(d, scene, wl0.init, cfg(kind, lvs=lvs, margin=m))
    assert res[0].n_contacts > 0
    agree(res[0], um[0], rows, counts_margin=m)


# ------------------------------------------------------------------ 6. device path
def test_check_on_the_device_trajectories():
    """BatchTrustRegionSQP.check() reads thip_device_x: the same bytes as a
    TrajectoryChecker on the downloaded trajectories."""
    wl = problems.make_workload("C", 4)
    config = cfg(abi.CHECK_LVS_CONTINUOUS, lvs=wl.desc.coll_lvs, margin=0.02)
    s = BatchTrustRegionSQP(wl, device=0)
    try:
        x, _ = s.optimize()
        res_d, um_d = s.check(config, unit_min=True)
    finally:
        s.close()
    res_h, um_h = run_checker(wl.desc, wl.scene, x, config)
    assert bytes((abi.CheckResult * 4)(*res_d)) == bytes((abi.CheckResult * 4)(*res_h))
    assert um_d.tobytes() == um_h.tobytes()
    assert all(r.n_candidates > 0 and np.isfinite(r.min_distance) for r in res_d)


# ------------------------------------------------------------------ 7. the reference's EXPECTs
def test_reference_expects_through_the_front_door(oracle_mod):
    """planning_unit.cpp:92-101, 143-148 on arm_around_table.json: checkTrajectory
    with a CONTINUOUS manager and margin 0 finds the initial trajectory in
    collision and the optimised one free of it (thost_check_json_batch), the
    oracle's continuous_check_found agreeing on both."""
    from trajopt_amd import host

    text = dc.text("arm_around_table.json")
    scenes = np.stack([dc.arm_around_table_scene()] * 4)
    wl = dc.json_workload(text, host, scenes[0])
    init = np.stack([wl.init[0]] * 4)
    config = abi.default_check_config()
    before = host.check_json_batch([text] * 4, scenes, init, config)
    x, res = host.solve_json_batch([text] * 4, scenes)
    after = host.check_json_batch([text] * 4, scenes, x, config)
    for b in range(4):
        assert before[b].found == 1 and before[b].min_distance < 0  # EXPECT_TRUE(found)
        assert dc.continuous_check_found(wl.desc, init[b], scenes[b], oracle_mod)
        assert after[b].found == 0 and after[b].min_distance >= 0  # EXPECT_FALSE(found)
        assert not dc.continuous_check_found(wl.desc, x[b], scenes[b], oracle_mod)
    # and the clearance figures against the oracle's candidates
    for traj, rs in ((init, before), (x, after)):
        rows = oracle_rows(oracle_mod, wl.desc, scenes[0], traj[0], abi.CHECK_LVS_CONTINUOUS, float("inf"))
        assert abs(rs[0].min_distance - rows[:, 5].min()) <= TOL
        assert rs[0].n_candidates == len(rows)
