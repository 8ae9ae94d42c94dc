"""Writes tests/golden/segment_hinge_bits.npz: the trajectories and every Result
field of the cases of tests/test_gpu_hinge_loads.py, as the installed build of
libtrajopt_hip.so solves them on the GPU (MI355X):

    python tests/golden/make_golden_segment_bits.py [output.npz]

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

import test_gpu_hinge_loads as T  # noqa: E402

out = {}
for name in T.CASES:
    x, res, tr, lay = T.solve(name)
    assert lay["seg_ok"] == 1, f"{name}: not on the segment ({lay})"
    out.update(T.result_arrays(name, x, res))
    print(f"{name}: x {x.shape}, statuses {[r.status for r in res]}, admm {[r.n_admm_iters for r in res]}", flush=True)
dst = Path(sys.argv[1]) if len(sys.argv) > 1 else T.GOLDEN
np.savez_compressed(dst, **out)
print(f"wrote {dst} ({dst.stat().st_size} bytes, {len(out)} arrays)")
