"""Writes tests/golden/handle_states.json: what the installed build of
libtrajopt_hip.so answers to the out-of-order and missing-argument calls of
tests/handle_states.py on every C-ABI handle, and to one good upload and run --

    python tests/golden/make_golden_handle_states.py [output.json]

Needs the GPU (the handles are live).  The fixture pins return codes and whole
messages: run this on the build that is the reference (the commit before a
restructuring that must keep them), never on the build under test.  The calls
are taken from tests/handle_states.py, which the test reads too.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent / "trajopt-1_amd"))
sys.path.insert(0, str(HERE.parent))

import handle_states  # noqa: E402
from trajopt_amd import abi  # noqa: E402

lib = abi.load_hip()
out = {name: states(lib) for name, states in handle_states.HANDLES.items()}
dst = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "handle_states.json"
# one line per call
text = "{\n" + ",\n".join(
    json.dumps(h) + ": {\n" + ",\n".join(
        json.dumps(call) + ": " + json.dumps(out[h][call], separators=(",", ":")) for call in out[h]) + "\n}"
    for h in out) + "\n}\n"
assert json.loads(text) == out
dst.write_text(text)
print(f"wrote {dst} ({dst.stat().st_size} bytes, {sum(len(v) for v in out.values())} calls of {len(out)} handles)")
