#!/usr/bin/env python3
"""Time the batched trajectory checker (thip_check_*) on config C's 1,024
30-waypoint trajectories -- LVS_CONTINUOUS with the config's own
longest_valid_segment_length -- next to thip_eval_collision on the same inputs
with a margin wide enough to keep every candidate, which is the only way to get
every candidate's distance without the checker.

  python tools/check_bench.py [--batch 1024] [--runs 15] [--out FILE.json]

Checker: HIP events around its two kernels (thip_check_last_ms), trajectories
already on the device, and the wall time of the whole host call
(thip_check_run: trajectories up, 64 bytes per problem back).  Evaluator: the
wall time of thip_eval_collision (synchronous: trajectories up, one record of
8 + 2 n_dof + 1 doubles per candidate back).  Warm runs first, then the median
of --runs (at least 10).  The two must agree: the same candidate count and the
same minimum distance per problem.  Needs an AMD GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "trajopt-1_amd"))

from trajopt_amd import abi, problems  # noqa: E402
from trajopt_amd.problems import Workload  # noqa: E402
from trajopt_amd.runtime import TermEvaluator, TrajectoryChecker  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "check_bench.json"))
    a = ap.parse_args()
    runs = max(a.runs, 10)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("check_bench: no GPU")
    wl = problems.make_workload("C", a.batch)
    B, N, D = wl.batch, wl.n_steps, wl.n_dof
    x = np.ascontiguousarray(wl.init)
    lvs = wl.desc.coll_lvs
    cfg = abi.CheckConfig(abi.CHECK_LVS_CONTINUOUS, lvs, 0.0, 0, -1)

    # ---- the checker
    chk = TrajectoryChecker(wl.desc, B, wl.scene, cfg)
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        res = chk.run_device(d_x.data_ptr())
        chk.run(x)
    kernel_ms, call_ms = [], []
    for _ in range(runs):
        res = chk.run_device(d_x.data_ptr())
        kernel_ms.append(chk.kernel_ms())
        t0 = time.perf_counter()
        res_h = chk.run(x)
        call_ms.append(1e3 * (time.perf_counter() - t0))
    assert bytes((abi.CheckResult * B)(*res)) == bytes((abi.CheckResult * B)(*res_h))
    n_cand = sum(r.n_candidates for r in res)
    chk.close()

    # ---- the evaluator, every candidate kept
    d = abi.ProblemDesc.from_buffer_copy(wl.desc)
    d.coll_enabled, d.coll_continuous, d.coll_lvs = 1, 1, lvs
    d.coll_margin, d.coll_buffer, d.n_coll_pairs, d.n_coll_extra = 1e3, 0.0, 0, 0
    d.coll_first_step, d.coll_last_step, d.coll_n_fixed = 0, N - 1, 0
    d.coll_contact_test = abi.CONTACT_ALL
    ev = TermEvaluator(Workload("check", d, x, wl.targets, wl.scene, x, None))
    W = 8 + 2 * D + 1
    dp = C.POINTER(C.c_double)
    cnt = (C.c_int * B)()
    one = np.zeros(W)
    for _ in range(2):  # counts only (cap 0); the first call also sizes the per-unit staging
        rc = ev.lib.thip_eval_collision(ev.ev, 0, x.ctypes.data_as(dp), one.ctypes.data_as(dp), 0, cnt)
        assert rc == 0, ev.lib.thip_eval_last_error(ev.ev).decode()
    cap = max(cnt)
    rec = np.zeros((B, cap, W))
    eval_ms = []
    for k in range(1 + runs):
        t0 = time.perf_counter()
        rc = ev.lib.thip_eval_collision(ev.ev, 0, x.ctypes.data_as(dp), rec.ctypes.data_as(dp), cap, cnt)
        dt = 1e3 * (time.perf_counter() - t0)
        assert rc == 0, ev.lib.thip_eval_last_error(ev.ev).decode()
        if k:
            eval_ms.append(dt)
    ev.close()
    counts = np.array(list(cnt))
    assert int(counts.sum()) == n_cand, (int(counts.sum()), n_cand)
    worst = 0.0
    for b in range(B):
        worst = max(worst, abs(rec[b, : counts[b], 5].min() - res[b].min_distance))
    assert worst <= 1e-12, worst

    out = {
        "workload": f"config C, {B} problems x {N} waypoints, LVS_CONTINUOUS, lvs {lvs}",
        "candidates": int(n_cand),
        "runs": runs,
        "checker_kernels_ms_median": statistics.median(kernel_ms),
        "checker_kernels_ms_min_max": [min(kernel_ms), max(kernel_ms)],
        "checker_call_ms_median": statistics.median(call_ms),
        "checker_call_ms_min_max": [min(call_ms), max(call_ms)],
        "checker_bytes_back": B * C.sizeof(abi.CheckResult),
        "eval_collision_call_ms_median": statistics.median(eval_ms),
        "eval_collision_call_ms_min_max": [min(eval_ms), max(eval_ms)],
        "eval_collision_bytes_back": int(B * cap * W * 8),
        "max_abs_min_distance_difference": worst,
        "n_in_contact_at_margin_0": int(sum(r.found for r in res)),
    }
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
