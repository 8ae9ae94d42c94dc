#!/usr/bin/env python3
"""The measured gaps of the direct QP tests and the tolerances they were held to.

Runs tests/test_gpu_qp_direct.py in this process (an MI355X is needed), then
writes every (solve, quantity, device gap, tolerance) the tests recorded to
profiles/qp_direct_gaps.json, with the worst gap / tolerance ratio per
quantity on top: DESIGN.md section 5 quotes that table.  The tolerances come
from the oracle alone (tests/qp_reference.py); the gaps are what the device
left of them.  The run stops at the first test that fails with a device error
instead of launching more work on a device in an unknown state.

    python tools/qp_direct_gaps.py [--out FILE] [-k EXPR]
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "trajopt-1_amd", REPO / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


class StopOnDeviceError:
    def pytest_runtest_logreport(self, report):
        import pytest

        if report.failed:
            text = str(report.longrepr)
            if "(-2," in text or "hipError" in text or "illegal memory" in text or "qp_csc_kernel:" in text:
                pytest.exit("device error: nothing more is launched", returncode=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "qp_direct_gaps.json"))
    ap.add_argument("-k", default=None)
    args = ap.parse_args()
    import pytest

    argv = [str(REPO / "tests" / "test_gpu_qp_direct.py"), "-m", "gpu", "-v", "-s", "--durations=0", "-p",
            "no:cacheprovider"]
    if args.k:
        argv += ["-k", args.k]
    rc = int(pytest.main(argv, plugins=[StopOnDeviceError()]))
    gaps = sys.modules["test_gpu_qp_direct"].GAPS if "test_gpu_qp_direct" in sys.modules else []
    worst = {}
    for label, what, gap, tol in gaps:
        key = what
        ratio = gap / tol if tol > 0 else (0.0 if gap == 0 else float("inf"))
        if key not in worst or ratio > worst[key]["ratio"]:
            worst[key] = {"ratio": ratio, "gap": gap, "tolerance": tol, "solve": label}
    out = {"pytest_exit": rc, "solves": len({g[0] for g in gaps}), "worst_by_quantity": worst,
           "records": [{"solve": g[0], "quantity": g[1], "gap": g[2], "tolerance": g[3]} for g in gaps]}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"{len(gaps)} records of {out['solves']} solves -> {args.out}; pytest exit {rc}")
    for k, w in sorted(worst.items()):
        print(f"  {k:12s} worst gap/tol {w['ratio']:.3g} ({w['gap']:.3e} / {w['tolerance']:.3e}) at {w['solve']}")
    return rc


if __name__ == "__main__":
    sys.exit(main())
