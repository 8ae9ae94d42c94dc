"""The one place a problem descriptor is lowered (csrc/desc_lowering.hpp), without a
GPU: every refusal message of thip_create, thip_terms_create and
thip_terms_slot_table, and the slot numbering of thip_terms_slot_table, are
exactly those recorded in tests/golden/desc_lowering.json from the build before
the two entry points shared their validator and their term plan
(tests/golden/make_golden_desc_lowering.py; the cases are tests/desc_cases.py)."""
import json
from pathlib import Path

import pytest

import desc_cases
from trajopt_amd import abi

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "desc_lowering.json").read_text())


@pytest.fixture(scope="module")
def lib():
    if not abi.HIP_LIB.exists():
        import __graft_entry__

        __graft_entry__.build()
    return abi.load_hip()


def test_the_recording_covers_the_cases():
    assert sorted(GOLDEN["refusals"]) == sorted(desc_cases.REFUSALS)
    assert sorted(GOLDEN["slot_tables"]) == sorted(desc_cases.SLOT_TABLES)


@pytest.mark.parametrize("name", sorted(desc_cases.REFUSALS))
def test_refusal_messages_are_the_recorded_ones(lib, name):
    got = desc_cases.refusals_of(lib, desc_cases.refusal_desc(name))
    assert got == GOLDEN["refusals"][name]


@pytest.mark.parametrize("name", sorted(desc_cases.SLOT_TABLES))
def test_slot_tables_are_the_recorded_ones(lib, name):
    got = desc_cases.slot_table_of(lib, desc_cases.SLOT_TABLES[name]())
    assert got == GOLDEN["slot_tables"][name]
    assert len(got["slots"]) == got["n_costs"] + got["n_cnts"]


@pytest.mark.parametrize("name", sorted(desc_cases.UNRECORDED_REFUSALS))
def test_every_call_refuses_what_the_recorded_build_let_through(lib, name):
    """coll_n_fixed outside [0, THIP_MAX_STEPS] (thip_create reads coll_fixed_steps[k] for
    k < coll_n_fixed) and a negative first step of a JointVel term (the kernels index the
    trajectory with it) are refused by every entry point, with one wording."""
    d, want = desc_cases.unrecorded_refusal(name)
    assert desc_cases.refusals_of(lib, d) == want
