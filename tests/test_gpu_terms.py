"""Per-term cost values and constraint violations on the GPU (thip_terms_*,
term_values.hip) against the solver's own evaluation (A_COST / A_VIOL of the
fused kernel's workspace), the oracle's primitives and the oracle's totals.

Both sides of every comparison evaluate the same x bits, so they differ only by
rounding and summation order: per slot
    tol = 1e-12 * (summands of the slot) * max(1, largest |coefficient| of the slot).

A_COST / A_VIOL: sqp_optimize() evaluates into them at X (first evaluation) and
copies NCOST / NVIOL over them whenever X := XN (sqp_kernel.hip), and
solve_problem() gathers the returned trajectory from that same X, so they hold
the values of the returned x; under THIP_DEBUG_STATIC_DISPATCH problem b keeps
workspace b."""
import ctypes as C
import functools

import numpy as np
import pytest

from trajopt_amd import abi, problems
from trajopt_amd.runtime import BatchTrustRegionSQP, HipError, TermValues

pytestmark = pytest.mark.gpu

BAR = 1e-12
LVS = 0.05


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


# ------------------------------------------------------------------ workloads
def _six_prims(wl):
    """14 robot spheres against 6 primitives: 84 candidates per sub-state."""
    wl.desc.n_prims = 6
    wl.scene = np.ascontiguousarray(wl.scene[:, :6])
    assert wl.desc.n_spheres == 14
    return wl


def coll_workload(kind, is_cnt, n_steps=6, batch=3, pairs=False, fixed_end=False, contact_test=abi.CONTACT_ALL):
    """Config C; kind 0 LVS_DISCRETE, 1 LVS_CONTINUOUS, 2 DISCRETE, 3 CONTINUOUS (one cast per pair)."""
    wl = _six_prims(problems.make_workload("C", batch, n_steps=n_steps))
    d = wl.desc
    d.coll_continuous = 1 if kind == 3 else kind
    d.coll_lvs = float("inf") if kind == 3 else LVS
    d.coll_is_cnt = 1 if is_cnt else 0
    d.coll_max_contacts = 4096
    d.coll_contact_test = contact_test
    # wide enough that every problem has contacts at its initial trajectory, some of them
    # between margin and margin + buffer (contacts that add nothing to the value)
    d.coll_margin, d.coll_buffer = 0.10, 0.03
    if fixed_end:
        d.coll_n_fixed = 1
        d.coll_fixed_steps[0] = 0
    if pairs:
        d.n_coll_pairs = 0
        links = sorted({d.sphere_link[s] for s in range(d.n_spheres)})
        problems.add_coll_pair(d, links[-1], 5, 0.15, 30.0)  # wider, heavier
        problems.add_coll_pair(d, links[-1], 3, 0.0, 0.0)    # zero coefficient: dropped
        problems.add_coll_pair(d, links[2], 4, 0.05, 4.0)    # narrower, lighter
    return wl


def dual_arm(contact_test=abi.CONTACT_ALL, pairs=False):
    wl = problems.make_workload("E", 2, n_steps=6)
    assert wl.desc.n_self_pairs > 0 and wl.desc.coll_continuous == 1
    wl.desc.coll_max_contacts = 8192
    wl.desc.coll_margin, wl.desc.coll_buffer = 0.10, 0.03
    wl.desc.coll_contact_test = contact_test
    if pairs:
        # a pairs table with scene entries, a dropped pair and a self pair named in the (b, a) order
        d = wl.desc
        problems.with_pair_data(wl, self_pairs=True)
        a, b = d.self_pair[1][0], d.self_pair[1][1]
        problems.add_coll_pair(d, a, -1 - b, 0.14, 7.0)
        assert any(d.coll_pairs[k].other < 0 for k in range(d.n_coll_pairs))
    return wl


VARIANTS = {
    "A6": lambda: problems.make_workload("A", 3, n_steps=6),
    "A7": lambda: problems.make_workload("A", 3, n_steps=7),
    "cart_cnt_tol7": lambda: problems.with_cart_tolerances(problems.make_workload("A", 3, n_steps=7), pos=0.01, rot=0.05),
    "cart_cost_tol6": lambda: problems.with_cart_tolerances(problems.make_workload("B", 3, n_steps=6), pos=0.01, rot=0.05),
    "dynamic6": lambda: problems.with_dynamic_target(problems.make_workload("B", 3, n_steps=6)),
    "dynamic7": lambda: problems.with_dynamic_target(problems.make_workload("B", 3, n_steps=7)),
    "jpos6": lambda: problems.make_workload("J", 3, n_steps=6, goal_offset=0.1),
    "jpos7": lambda: problems.make_workload("J", 3, n_steps=7, goal_offset=0.1),
    "jpos_ineq": lambda: problems.make_reference_unit("joint_pos_ineq", 3),
    "jvel_ineq": lambda: problems.make_reference_unit("joint_vel_ineq", 3),
    "jacc6": lambda: problems.make_workload("HA", 3, n_steps=6),
    # a JointAccEqCost on 2 dofs: the solver runs narrow waypoint-pair blocks (2 and 3 of them)
    "jacc4_2dof": lambda: problems.make_workload("HA", 3, n_steps=4, robot="right_arm_2dof"),
    "jacc6_2dof": lambda: problems.make_workload("HA", 3, n_steps=6, robot="right_arm_2dof"),
    "pairs6": lambda: coll_workload(0, False, pairs=True),
    "fixed_end_cast7": lambda: coll_workload(1, False, n_steps=7, fixed_end=True),
    "C30": lambda: coll_workload(1, False, n_steps=30),
    "dual_arm": dual_arm,
    "first6": lambda: coll_workload(0, False, contact_test=abi.CONTACT_FIRST),
    "closest7": lambda: coll_workload(1, False, n_steps=7, contact_test=abi.CONTACT_CLOSEST),
    "closest_cnt6": lambda: coll_workload(0, True, pairs=True, contact_test=abi.CONTACT_CLOSEST),
    "closest_dual_pairs": lambda: dual_arm(abi.CONTACT_CLOSEST, pairs=True),
    "first_dual_pairs": lambda: dual_arm(abi.CONTACT_FIRST, pairs=True),
}
for _kind, _kn in enumerate(("lvs_discrete", "lvs_continuous", "discrete", "continuous")):
    for _cnt in (0, 1):
        VARIANTS[f"C_{_kn}_{'cnt' if _cnt else 'cost'}"] = functools.partial(coll_workload, _kind, _cnt,
                                                                             n_steps=6 if (_kind + _cnt) % 2 else 7)


# ------------------------------------------------------------------ tolerance
def slot_tols(desc, slots, contacts=None):
    """tol per slot; contacts [n_slots] = contact count of a collision slot (its summands)."""
    N, D = desc.n_steps, desc.chain.n_dof
    out = []
    for i, s in enumerate(slots):
        k = s.index
        if s.kind == abi.TERM_JOINT_VEL:
            ineq = any(abs(desc.jv_upper_tols[j]) >= 1e-5 or abs(desc.jv_lower_tols[j]) >= 1e-5 for j in range(D))
            n, cf = (N - 1) * D * (2 if ineq else 1), max(abs(desc.jv_coeffs[j]) for j in range(D))
        elif s.kind == abi.TERM_JVX:
            n, cf = 2 * (N - 1) * D, max(abs(desc.jvx_coeffs[k][j]) for j in range(D))
        elif s.kind == abi.TERM_JPOS:
            n, cf = 2 * N * D, max(abs(desc.jpos_coeffs[k][j]) for j in range(D))
        elif s.kind == abi.TERM_JDT:
            n, cf = (N - 2) * D, max(abs(desc.jdt_coeffs[k][j]) for j in range(D))
        elif s.kind == abi.TERM_CART:
            n = 6
            cf = max([abs(desc.cart_pos_coeffs[k][i]) for i in range(3)] + [abs(desc.cart_rot_coeffs[k][i]) for i in range(3)])
        else:
            n = max(1, int(contacts[i])) if contacts is not None else 1
            cf = max([abs(desc.coll_coeff)] + [abs(desc.coll_pairs[p].coeff) for p in range(desc.n_coll_pairs)])
        out.append(BAR * n * max(1.0, cf))
    return np.array(out)


def agree(name, got, want, tol, names):
    assert got.shape == want.shape, (name, got.shape, want.shape)
    for i in range(got.shape[-1]):
        diff = np.abs(got[..., i] - want[..., i]).max() if got.size else 0.0
        print(f"{name} {names[i]}: max |diff| {diff:.3e} tol {tol[i]:.3e} max |value| {np.abs(want[..., i]).max():.6g}")
    for i in range(got.shape[-1]):
        assert np.all(np.abs(got[..., i] - want[..., i]) <= tol[i]), (name, names[i])


# ------------------------------------------------------------------ 1. the solver's own evaluation
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_slots_against_the_solvers_own_evaluation(hip, variant):
    wl = VARIANTS[variant]()
    assert hip.thip_debug_set_path(abi.DEBUG_STATIC_DISPATCH) == 0
    try:
        s = BatchTrustRegionSQP(wl, device=0)
    finally:
        hip.thip_debug_set_path(0)
    try:
        x, res = s.optimize()
        costs, viols = s.term_values()
        dws, iws, doff, ioff = s.debug_values()
        # the contacts of every unit at the returned x (after the workspace was read: this call writes it)
        rows = s.collision_rows(x, cap=8192) if wl.desc.coll_enabled else None
    finally:
        s.close()
    tv = TermValues(wl)
    try:
        slots, names = tv.slots, tv.slot_names()
        nc, nv = tv.n_costs, tv.n_cnts
        costs_h, viols_h = tv.run(x)
    finally:
        tv.close()
    assert all(r.n_costs == nc and r.n_cnts == nv for r in res)
    assert all(not (r.flags & 1) for r in res), "contact overflow"
    a_cost = dws[:, doff[abi.WS_A_COST]: doff[abi.WS_A_COST] + nc]
    a_viol = dws[:, doff[abi.WS_A_VIOL]: doff[abi.WS_A_VIOL] + nv]
    contacts = np.array([max((r[:, 0].astype(int) == sl.unit).sum() for r in rows) if sl.kind == abi.TERM_COLL else 0
                         for sl in slots])
    tol = slot_tols(wl.desc, slots, contacts)
    agree(variant, costs, a_cost, tol[:nc], names[:nc])
    agree(variant, viols, a_viol, tol[nc:], names[nc:])
    # host-pointer and device-pointer runs: the same bits
    assert costs.tobytes() == costs_h.tobytes() and viols.tobytes() == viols_h.tobytes()
    # the solver's totals are sums / maxima of the same slots
    for b, r in enumerate(res):
        assert abs(costs[b].sum() - r.total_cost) <= tol[:nc].sum()
        if nv:
            assert abs(viols[b].max() - r.max_cnt_viol) <= tol[nc:].max()
    if wl.desc.coll_enabled:
        coll = [i for i, sl in enumerate(slots) if sl.kind == abi.TERM_COLL]
        # DISCRETE: one unit per waypoint that is not a fixed step of the term; else one per step pair
        assert len(coll) == (wl.n_steps - wl.desc.coll_n_fixed if wl.desc.coll_continuous == 2 else wl.n_steps - 1)


# ------------------------------------------------------------------ 2. the oracle's primitives
def all_candidates(oracle_mod, desc, scene, x):
    """Every candidate's distance (the term with margin 1e3, no buffer, pairs or fixed steps)."""
    d = abi.ProblemDesc.from_buffer_copy(desc)
    d.coll_margin, d.coll_buffer, d.n_coll_pairs, d.coll_n_fixed = 1e3, 0.0, 0, 0
    d.coll_contact_test = abi.CONTACT_ALL
    wl =problems.Workload("cand", d, x[None], np.zeros((1, 0, 12)), scene[None], x[None])
    n = len(oracle_mod.collision_rows(wl, 0, x, cap=1))
    rows = oracle_mod.collision_rows(wl, 0, x, cap=60000)
    assert n == 1 and len(rows) < 60000
    return rows


def _vec(a, D):
    return np.array([a[j] for j in range(D)])


def _zero(tols):
    """trajopt_common::doubleEquals(tol, 0.) for every joint: the Eq forms."""
    return bool(np.all(np.abs(tols) < 1e-5))


def _vel_steps(N, first, last):
    """JointVelTermInfo::hatch's step clamping (problem_description.cpp:1228-1245): velocities f .. l - 1."""
    if last <= -1:
        last = N - 1
    first, last = min(first, N - 2), min(last, N - 1)
    if last == first:
        last += 1
    return (last, first) if last < first else (first, last)


def _pos_steps(N, first, last):
    """JointPosTermInfo::hatch's step clamping (problem_description.cpp:1097-1120): waypoints f .. l."""
    if last <= -1:
        last = N - 1
    first, last = min(first, N - 1), min(last, N - 1)
    return (last, first) if last < first else (first, last)


def numpy_slots(oracle_mod, wl, x, slots):
    """costs / viols of every slot restated in numpy from x and the oracle's primitives."""
    d, B, N, D = wl.desc, wl.batch, wl.n_steps, wl.n_dof
    err = oracle_mod.linearize(wl, x)[0] if d.n_cart else None
    over = problems.pair_overrides(d)
    out = np.zeros((B, len(slots)))
    contacts = np.zeros(len(slots))
    vel = np.diff(x, axis=1)
    for b in range(B):
        rows = oracle_mod.collision_rows(wl, b, x[b], cap=20000) if d.coll_enabled else None
        for i, s in enumerate(slots):
            k = s.index
            if s.kind in (abi.TERM_JOINT_VEL, abi.TERM_JVX):
                # JointVelEqCost, or the tolerance forms (JointVelIneqCost / JointVelIneqConstraint:
                # the sum of the two hinges per (step, joint))
                jv = s.kind == abi.TERM_JOINT_VEL
                f, l = _vel_steps(N, d.jv_first_step if jv else d.jvx_first_step[k],
                                  d.jv_last_step if jv else d.jvx_last_step[k])
                cf = _vec(d.jv_coeffs if jv else d.jvx_coeffs[k], D)
                up = _vec(d.jv_upper_tols if jv else d.jvx_upper_tols[k], D)
                lo = _vec(d.jv_lower_tols if jv else d.jvx_lower_tols[k], D)
                dd = vel[b, f:l] - _vec(d.jv_targets if jv else d.jvx_targets[k], D)
                if _zero(up) and _zero(lo):
                    out[b, i] = (dd * dd * cf).sum()
                else:
                    out[b, i] = np.maximum((dd - up) * cf, 0.0).sum() + np.maximum((lo - dd) * cf, 0.0).sum()
            elif s.kind == abi.TERM_JPOS:
                f, l = _pos_steps(N, d.jpos_first_step[k], d.jpos_last_step[k])
                tg = wl.jpos_targets[b, k] if wl.jpos_targets is not None else _vec(d.jpos_targets[k], D)
                cf, up, lo = _vec(d.jpos_coeffs[k], D), _vec(d.jpos_upper_tols[k], D), _vec(d.jpos_lower_tols[k], D)
                dd = x[b, f:l + 1] - tg
                if _zero(up) and _zero(lo):
                    out[b, i] = np.abs(dd * dd * cf).sum()
                else:
                    out[b, i] = np.maximum((dd - up) * cf, 0.0).sum() + np.maximum((lo - dd) * cf, 0.0).sum()
            elif s.kind == abi.TERM_JDT:
                f, l = d.jdt_first_step[k], d.jdt_last_step[k]
                acc = np.diff(np.diff(x[b, f:l + 1], axis=0), axis=0) - np.array(d.jdt_targets[k][:D])
                out[b, i] = (acc * acc * np.array(d.jdt_coeffs[k][:D])).sum()
            elif s.kind == abi.TERM_CART:
                cf = np.array([d.cart_pos_coeffs[k][j] for j in range(3)] + [d.cart_rot_coeffs[k][j] for j in range(3)])
                keep = np.abs(cf) > 1e-5
                out[b, i] = np.abs(err[b, k][keep] * cf[keep]).sum()
            elif s.kind == abi.TERM_COLL:
                r = rows[rows[:, 0].astype(int) == s.unit]
                contacts[i] = max(contacts[i], len(r))
                v = 0.0
                for row in r:
                    link, other = int(row[1]), int(row[2])
                    if other < 0:  # a self contact: robot sphere -1 - other
                        other = -1 - d.sphere_link[-1 - other]
                    m, c = over.get((link, other), (d.coll_margin, d.coll_coeff))
                    v += c * max(m - row[5], 0.0)
                out[b, i] = v
            else:
                raise AssertionError(f"unknown slot kind {s.kind}")
    return out, contacts


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_slots_against_the_oracles_primitives(oracle_mod, variant):
    """At trajectories the solver never saw: the initial one, and it plus a seeded 0.05 rad perturbation."""
    wl = VARIANTS[variant]()
    d = wl.desc
    rng = np.random.default_rng(11)
    xs = [wl.init.copy(), wl.init + 0.05 * rng.standard_normal(wl.init.shape)]
    tv = TermValues(wl)
    try:
        slots, names, nc = tv.slots, tv.slot_names(), tv.n_costs
        for which, x in enumerate(xs):
            if d.coll_enabled:
                # no candidate within 1e-9 of a contact threshold: the contact sets are unambiguous
                over = problems.pair_overrides(d)
                for b in range(wl.batch):
                    cand = all_candidates(oracle_mod, d, wl.scene[b], x[b])
                    for row in cand:
                        link, other = int(row[1]), int(row[2])
                        if other < 0:
                            other = -1 - d.sphere_link[-1 - other]
                        m = over.get((link, other), (d.coll_margin, 0))[0]
                        assert abs(row[5] - (m + d.coll_buffer)) > 1e-9, "ambiguous contact: pick another seed"
            want, contacts = numpy_slots(oracle_mod, wl, x, slots)
            costs, viols = tv.run(x)
            tol = slot_tols(d, slots, contacts)
            agree(f"{variant}/{which}", costs, want[:, :nc], tol[:nc], names[:nc])
            agree(f"{variant}/{which}", viols, want[:, nc:], tol[nc:], names[nc:])
            if d.coll_enabled and which == 0:
                assert contacts.sum() > 0, "the collision slots are all empty: the case shows nothing"
    finally:
        tv.close()


# ------------------------------------------------------------------ 3. the oracle's totals
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_totals_against_the_oracle(oracle_mod, variant):
    wl = VARIANTS[variant]()
    xo, ro = oracle_mod.solve(wl, n_threads=3)
    tv = TermValues(wl)
    try:
        costs, viols = tv.run(xo)
        slots, nc = tv.slots, tv.n_costs
    finally:
        tv.close()
    # a collision slot's summands: the oracle's contacts of its unit at that x
    contacts = np.zeros(len(slots))
    for b in range(wl.batch if wl.desc.coll_enabled else 0):
        rows = oracle_mod.collision_rows(wl, b, xo[b], cap=20000)
        for i, sl in enumerate(slots):
            if sl.kind == abi.TERM_COLL:
                contacts[i] = max(contacts[i], (rows[:, 0].astype(int) == sl.unit).sum())
    tol = slot_tols(wl.desc, slots, contacts)
    for b, r in enumerate(ro):
        assert r.n_costs == tv.n_costs and r.n_cnts == tv.n_cnts
        print(f"{variant}[{b}] total_cost {r.total_cost!r} sum {costs[b].sum()!r} max_cnt_viol {r.max_cnt_viol!r} "
              f"max {viols[b].max() if viols.shape[1] else 0.0!r}")
        assert abs(costs[b].sum() - r.total_cost) <= tol[:nc].sum()
        if viols.shape[1]:
            assert abs(viols[b].max() - r.max_cnt_viol) <= tol[nc:].max()


# ------------------------------------------------------------------ 6. repeatability
@pytest.mark.parametrize("variant", ["A7", "jpos6", "C_lvs_continuous_cost", "dual_arm"])
def test_bitwise_repeatable_and_independent_of_the_batch(variant):
    wl = VARIANTS[variant]()
    rng = np.random.default_rng(5)
    x = wl.init + 0.05 * rng.standard_normal(wl.init.shape)
    tv = TermValues(wl)
    try:
        c1, v1 = tv.run(x)
        c2, v2 = tv.run(x)
    finally:
        tv.close()
    assert c1.tobytes() == c2.tobytes() and v1.tobytes() == v2.tobytes()
    for b in range(wl.batch):
        one = TermValues(wl.slice(b, b + 1))
        try:
            cb, vb = one.run(x[b:b + 1])
        finally:
            one.close()
        assert cb.tobytes() == c1[b:b + 1].tobytes() and vb.tobytes() == v1[b:b + 1].tobytes(), b


def test_slot_table_and_refusals():
    wl = VARIANTS["C_lvs_discrete_cnt"]()
    tv = TermValues(wl)
    try:
        kinds = [(s.kind, s.is_cnt) for s in tv.slots]
        assert kinds[0] == (abi.TERM_JOINT_VEL, 0)
        assert kinds[1:tv.n_costs] == [(abi.TERM_CART, 0)] * wl.desc.n_cart
        assert kinds[tv.n_costs:] == [(abi.TERM_COLL, 1)] * (wl.n_steps - 1)
        assert [s.unit for s in tv.slots[tv.n_costs:]] == list(range(wl.n_steps - 1))
        with pytest.raises(HipError, match="x has"):
            tv.run(np.zeros((1, 2, 3)))
    finally:
        tv.close()
    wl.desc.n_coll_extra = 1
    with pytest.raises(HipError, match="host loop"):
        TermValues(wl)


# ------------------------------------------------------------------ 4. order and names: the host term objects
def _json_cases():
    import dropin_cases as dc
    from trajopt_amd import host

    out = {}
    # the lowerable JSON fixture of tests/golden/json (numerical_ik1.json has one waypoint and
    # simple_collision_test.json one waypoint and two collision terms: both run the host loop only,
    # tests/test_terms_frontdoor.py pins their refusal)
    out["arm_around_table.json"] = ([dc.text("arm_around_table.json")] * 2, np.stack([dc.arm_around_table_scene()] * 2))
    for key, wl in (("A6", VARIANTS["A6"]()), ("jpos7", VARIANTS["jpos7"]()),
                    ("C_lvs_discrete_cost", VARIANTS["C_lvs_discrete_cost"]()),
                    ("C_discrete_cnt", VARIANTS["C_discrete_cnt"]()), ("dual_arm", dual_arm())):
        out[key] = ([host.workload_to_json(wl, b) for b in range(wl.batch)], wl.scene if wl.scene.size else None)
    return out


def _entry_tols(hip, text, scene, x):
    """(tol per getCosts() entry, tol per getConstraints() entry) from the slot table, the
    slot map and the contacts thip_eval_collision finds at x."""
    import dropin_cases as dc
    from trajopt_amd import host
    from trajopt_amd.runtime import TermEvaluator

    wl = dc.json_workload(text, host, scene)
    nc, nv = C.c_int(), C.c_int()
    tab = (abi.TermSlot * 512)()
    assert hip.thip_terms_slot_table(C.byref(wl.desc), tab, 512, C.byref(nc), C.byref(nv)) == 0
    slots = list(tab)[: nc.value + nv.value]
    contacts = np.zeros(len(slots))
    if wl.desc.coll_enabled:
        ev = TermEvaluator(wl)
        try:
            rows = ev.collision(0, x[None])[0]
        finally:
            ev.close()
        contacts = np.array([(rows[:, 0].astype(int) == s.unit).sum() if s.kind == abi.TERM_COLL else 0 for s in slots])
    tol = slot_tols(wl.desc, slots, contacts)
    smap = host.eval_json_batch([text], None if scene is None else scene[None], None, route=host.EVAL_NAMES)["slot_map"]
    ct, vt = np.zeros(nc.value), np.zeros(nv.value)
    for s in range(nc.value):
        ct[smap[s]] = tol[s]
    for s in range(nv.value):
        vt[smap[nc.value + s]] = tol[nc.value + s]
    return ct, vt


@pytest.mark.parametrize("case", ["arm_around_table.json", "A6", "jpos7", "C_lvs_discrete_cost", "C_discrete_cnt",
                                  "dual_arm"])
def test_device_route_equals_the_host_term_objects(hip, case):
    from trajopt_amd import host

    texts, scenes = _json_cases()[case]
    names = host.eval_json_batch(texts, scenes, None, route=host.EVAL_NAMES)  # raises unless lowerable
    assert len(names["cost_names"]) + len(names["cnt_names"]) > 0
    init = np.stack([host.lower_json(t, None if scenes is None else scenes[b])[1] for b, t in enumerate(texts)])
    rng = np.random.default_rng(3)
    for which, x in enumerate((init, init + 0.05 * rng.standard_normal(init.shape))):
        dev = host.eval_json_batch(texts, scenes, x, route=host.EVAL_DEVICE)
        obj = host.eval_json_batch(texts, scenes, x, route=host.EVAL_OBJECTS)
        assert dev["cost_names"] == obj["cost_names"] == names["cost_names"]
        assert dev["cnt_names"] == obj["cnt_names"] == names["cnt_names"]
        for b in range(len(texts)):
            ct, vt = _entry_tols(hip, texts[b], None if scenes is None else scenes[b], x[b])
            agree(f"{case}/{which}[{b}]", dev["cost_vals"][b], obj["cost_vals"][b], ct, dev["cost_names"])
            agree(f"{case}/{which}[{b}]", dev["cnt_viols"][b], obj["cnt_viols"][b], vt, dev["cnt_names"])


# ------------------------------------------------------------------ 5. the front door's results
@pytest.mark.parametrize("case", ["A6", "jpos7", "C_discrete_cnt"])
@pytest.mark.parametrize("drop_in", [False, True], ids=["batch", "drop_in"])
def test_front_door_results_carry_the_term_values(hip, case, drop_in):
    from trajopt_amd import host

    texts, scenes = _json_cases()[case]
    names = host.eval_json_batch(texts, scenes, None, route=host.EVAL_NAMES)
    x, res, cv, vv = host.solve_json_batch_terms(texts, scenes, drop_in=drop_in)
    assert cv.shape[1] == len(names["cost_names"]) > 0  # cost_vals.size() == getCosts().size()
    assert vv.shape[1] == len(names["cnt_names"])
    again = host.eval_json_batch(texts, scenes, x, route=host.EVAL_DEVICE)
    for b, r in enumerate(res):
        ct, vt = _entry_tols(hip, texts[b], None if scenes is None else scenes[b], x[b])
        print(f"{case}[{b}] total_cost {r.total_cost!r} vecSum {cv[b].sum()!r} max_cnt_viol {r.max_cnt_viol!r}")
        assert abs(cv[b].sum() - r.total_cost) <= ct.sum()
        if vv.shape[1]:
            assert abs(vv[b].max() - r.max_cnt_viol) <= vt.max()
        # and they are the evaluator's values at the returned trajectory, in the same order
        assert cv[b].tobytes() == again["cost_vals"][b].tobytes()
        assert vv[b].tobytes() == again["cnt_viols"][b].tobytes()
