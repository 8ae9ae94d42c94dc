"""The front door's map from kernel slots to term objects (trajopt::termSlotMap,
through thost_eval_json_batch's names-only route) without a GPU: for every
lowerable JSON problem the map is a permutation that covers every getCosts() /
getConstraints() entry exactly once, the counts are the slot table's, and the
names are the term objects'."""
import ctypes as C
import json
from pathlib import Path

import pytest

import dropin_cases as dc
from trajopt_amd import abi, host, problems

JSON_DIR = Path(__file__).resolve().parent / "golden" / "json"


@pytest.fixture(scope="module")
def built():
    if not host.HOST_LIB.exists():
        import __graft_entry__

        __graft_entry__.build()
    return host.load_host()


def _slot_table(desc):
    lib = abi.load_hip()
    nc, nv = C.c_int(), C.c_int()
    tab = (abi.TermSlot * 512)()
    rc = lib.thip_terms_slot_table(C.byref(desc), tab, 512, C.byref(nc), C.byref(nv))
    return rc, nc.value, nv.value, list(tab)[: nc.value + nv.value]


def _scene_of(name):
    return dc.arm_around_table_scene() if name == "arm_around_table.json" else None


def _cases():
    out = [(p.name, dc.text(p.name), _scene_of(p.name)) for p in sorted(JSON_DIR.glob("*.json"))]
    for config, n in (("A", 6), ("B", 7), ("C", 6), ("E", 6), ("J", 7)):
        wl = problems.make_workload(config, 1, n_steps=n)
        out.append((f"workload_{config}{n}", host.workload_to_json(wl, 0), wl.scene[0] if wl.scene.size else None))
    wl = problems.make_workload("C", 1, n_steps=6)
    wl.desc.coll_is_cnt, wl.desc.coll_continuous = 1, 2
    out.append(("workload_C6_discrete_cnt", host.workload_to_json(wl, 0), wl.scene[0]))
    return out


# the fixtures the fused kernel does not lower, and the reason each refusal must give
REFUSED = {"numerical_ik1.json": "n_steps", "simple_collision_test.json": "n_steps"}
CASES = [c for c in _cases() if c[0] not in REFUSED]
REFUSED_CASES = [c for c in _cases() if c[0] in REFUSED]


def test_every_json_fixture_is_accounted_for():
    names = {p.name for p in JSON_DIR.glob("*.json")}
    assert names == {c[0] for c in CASES if c[0].endswith(".json")} | set(REFUSED)
    assert "arm_around_table.json" in {c[0] for c in CASES} and len(CASES) == 7


@pytest.mark.parametrize("name, text, scene", REFUSED_CASES, ids=[c[0] for c in REFUSED_CASES])
def test_fixtures_the_fused_kernel_does_not_lower_are_refused(built, name, text, scene):
    """One waypoint (and, for simple_collision_test.json, a second collision term): refused by the C-ABI
    and by the front door, before any device call, with the reason and the host loop named."""
    desc = host.lower_json(text, scene)[0]
    assert desc.n_steps == 1
    assert _slot_table(desc)[0] == -1
    msg = abi.load_hip().thip_terms_last_error(None).decode()
    assert REFUSED[name] in msg and "host loop" in msg, msg
    with pytest.raises(host.HostError) as e:
        host.eval_json_batch([text], None, None, route=host.EVAL_NAMES)
    assert REFUSED[name] in str(e.value) and "host loop" in str(e.value), str(e.value)


@pytest.mark.parametrize("name, text, scene", CASES, ids=[c[0] for c in CASES])
def test_slot_map_is_a_permutation_over_every_term(built, name, text, scene):
    desc = host.lower_json(text, scene)[0]
    rc, nc, nv, table = _slot_table(desc)
    assert rc == 0, abi.load_hip().thip_terms_last_error(None).decode()  # every case here is lowerable
    scenes = None if scene is None or len(scene) == 0 else scene[None]
    r = host.eval_json_batch([text], scenes, None, route=host.EVAL_NAMES)
    doc = json.loads(text)
    assert len(r["cost_names"]) == nc and len(r["cnt_names"]) == nv
    assert len(table) == nc + nv and [s.is_cnt for s in table] == [0] * nc + [1] * nv
    assert sorted(r["slot_map"][:nc]) == list(range(nc))
    assert sorted(r["slot_map"][nc:]) == list(range(nv))
    assert all(n for n in r["cost_names"] + r["cnt_names"])
    # a collision term hatches one object per unit; every other JSON term one object
    n_coll = sum(1 for s in table if s.kind == abi.TERM_COLL)
    others = [t for t in doc.get("costs", []) + doc.get("constraints", []) if t["type"] != "collision"]
    assert nc + nv - n_coll == len(others)
    # collision units keep their waypoint order among the term objects
    pos = [r["slot_map"][i] for i, s in enumerate(table) if s.kind == abi.TERM_COLL]
    assert pos == sorted(pos)


def test_the_cases_cover_every_kind_the_fixtures_have(built):
    kinds = set()
    for _, text, scene in CASES:
        kinds |= {s.kind for s in _slot_table(host.lower_json(text, scene)[0])[3]}
    assert {abi.TERM_JOINT_VEL, abi.TERM_CART, abi.TERM_JPOS, abi.TERM_COLL} <= kinds


def test_trajectories_must_match_the_batch(built):
    wl = problems.make_workload("A", 1, n_steps=6)
    text = host.workload_to_json(wl, 0)
    with pytest.raises(host.HostError, match="trajectories"):
        host.eval_json_batch([text, text], None, wl.init)
