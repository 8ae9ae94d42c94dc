"""Writes tests/golden/collsets_bits.npz: values, jac, coeffs, counts and keys of
the cases of tests/test_gpu_collsets_bits.py, as the installed build of
libtrajopt_hip.so computes them on the GPU (MI355X):

    python tests/golden/make_golden_collsets_bits.py [output.npz]

The fixture pins bits: run this on the build whose arithmetic is the reference
(the commit before a restructuring that must keep every bit), never on the build
under test.  The cases and the entry layout are taken from the test module, so
the two cannot drift apart.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent / "trajopt-1_amd"))
sys.path.insert(0, str(HERE.parent))

import test_gpu_collsets_bits as T  # noqa: E402

out = {}
for name in T.CASES:
    got = T.run_case(name)
    T.check_case(name, got)
    again = T.run_case(name)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got), f"{name}: two runs differ"
    out.update(got)
dst = Path(sys.argv[1]) if len(sys.argv) > 1 else T.GOLDEN
packed = T.pack(out)
back = T.unpack(packed)
assert all(back[k].dtype == out[k].dtype and back[k].tobytes() == out[k].tobytes() for k in out)
np.savez_compressed(dst, **packed)
print(f"wrote {dst} ({dst.stat().st_size} bytes, {len(out)} arrays in {len(packed)} entries)")
