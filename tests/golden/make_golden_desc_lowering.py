"""Writes tests/golden/desc_lowering.json: what the installed build of
libtrajopt_hip.so says about the descriptors of tests/desc_cases.py --

    python tests/golden/make_golden_desc_lowering.py [output.json]

* "refusals": for every mutation of desc_cases.REFUSALS, the whole message of
  thip_last_error(NULL) after thip_create, and of thip_terms_last_error(NULL)
  after thip_terms_create and after thip_terms_slot_table;
* "slot_tables": for every problem of desc_cases.SLOT_TABLES, n_costs, n_cnts and
  the (kind, index, unit, is_cnt) rows of thip_terms_slot_table.

Every call returns before any device call, so no GPU is needed.  The fixture pins
messages and numbering: run this on the build that is the reference (the commit
before a restructuring that must keep them), never on the build under test.  The
cases are taken from tests/desc_cases.py, which the test reads too, so the two
cannot drift apart.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent / "trajopt-1_amd"))
sys.path.insert(0, str(HERE.parent))

import desc_cases  # noqa: E402
from trajopt_amd import abi  # noqa: E402

lib = abi.load_hip()
out = {
    "refusals": {name: desc_cases.refusals_of(lib, desc_cases.refusal_desc(name)) for name in desc_cases.REFUSALS},
    "slot_tables": {name: desc_cases.slot_table_of(lib, build()) for name, build in desc_cases.SLOT_TABLES.items()},
}
dst = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "desc_lowering.json"
# one line per case
text = "{\n" + ",\n".join(
    json.dumps(sec) + ": {\n" + ",\n".join(
        json.dumps(name) + ": " + json.dumps(out[sec][name], separators=(",", ":"), sort_keys=True)
        for name in sorted(out[sec])) + "\n}" for sec in sorted(out)) + "\n}\n"
assert json.loads(text) == out
dst.write_text(text)
print(f"wrote {dst} ({dst.stat().st_size} bytes, {len(out['refusals'])} refusals, "
      f"{len(out['slot_tables'])} slot tables)")
