#!/usr/bin/env python3
"""Time a batch of trajopt_sqp problems solved in lock step
(thost_tsqp_solve_batch: one thip_qp_step launch per round and QP pattern)
against the same problems solved one after another (a loop of thost_tsqp_solve
calls: one thip_qp and five launches per convexification each).

  python tools/tsqp_batch_bench.py [--sizes 1,16,64,256] [--repeats 5] [--out FILE.json]

The problems are tests/tsqp_cases.py's "smooth" trajectories (20 nodes x 7
joints), seeds 0..B-1.  For each batch size B the two alternate in one process:
one warm-up of each, then --repeats timed runs of each, wall time of the whole
call(s) including the problems' construction on the host.  Reported per size:
median and min-max of both, their ratio, the batch's launch counts (rounds,
thip_qp_step launches, thip_qp objects = symbolic analyses, largest group) and,
for the loop, the symbolic analyses (one per problem) and launches read from the
problems' counters (a setup and a warm-start launch per setup, four update
launches per in-place convexification, one launch per solve; the bounds pushed
after each trust-region step come on top, so 2 * setups + 4 * updates + solves
is a lower bound).  Every batch result is checked bitwise
against the loop's.  Needs an AMD GPU; there is no fallback."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "trajopt-1_amd"))
sys.path.insert(0, str(ROOT / "tests"))

import tsqp_cases  # noqa: E402
from trajopt_amd import abi, tsqp  # noqa: E402


def spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,64,256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tsqp_batch_bench.json"))
    a = ap.parse_args()
    abi.load_hip()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tsqp_batch_bench: no GPU")
    sizes = [int(s) for s in a.sizes.split(",")]
    specs = [tsqp_cases.synthetic("smooth", s, n=20) for s in range(max(sizes))]
    rows = []
    for B in sizes:
        sp = specs[:B]

        def loop():
            t0 = time.perf_counter()
            out = [tsqp.solve(s) for s in sp]
            return time.perf_counter() - t0, out

        def batch():
            t0 = time.perf_counter()
            out = tsqp.solve_batch(sp)
            return time.perf_counter() - t0, out

        _, ref = loop()  # warm-up of each
        _, (xs, rs, rounds, st) = batch()
        for b in range(B):
            assert xs[b].tobytes() == ref[b][0].tobytes() and rs[b].qp_solves == ref[b][1].qp_solves, b
        t_loop, t_batch = [], []
        for _ in range(a.repeats):
            t_loop.append(loop()[0])
            t_batch.append(batch()[0])
        r = [x[1] for x in ref]
        row = {
            "batch": B,
            "loop": spread(t_loop),
            "lock_step": spread(t_batch),
            "loop_over_lock_step": statistics.median(t_loop) / statistics.median(t_batch),
            "lock_step_counts": {"rounds": st.rounds, "step_launches": st.step_launches, "thip_qp_objects": st.groups,
                                 "max_group": st.max_group, "qp_rounds_max": int(rounds.max())},
            "loop_counts": {"thip_qp_objects": sum(x.qp_setups for x in r),
                            "launches_at_least": sum(2 * x.qp_setups + 4 * x.qp_updates + x.qp_solves for x in r),
                            "qp_solves": sum(x.qp_solves for x in r), "admm_iters": sum(x.admm_iters for x in r)},
            "bitwise_equal": True,
        }
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"problem": "tsqp_cases.synthetic('smooth', seed, n=20), seeds 0..B-1", "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
