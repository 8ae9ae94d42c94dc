#!/usr/bin/env python3
"""Time one continuous-collision-set launch (thip_ccsets_*, coll_sets_cont.hip) on
config C's robot and scene -- 1,024 problems x 29 segments, LVS_CONTINUOUS with
the workload's own longest valid segment length, max_num_cnt 3 -- next to
thip_eval_collision on the same descriptor with the same evaluator type, which
linearises every contact and returns every record to the host.

  python tools/ccsets_bench.py [--batch 1024] [--runs 30] [--out FILE.json]

Continuous sets: the HIP-event time of ccsets_kernel (thip_ccsets_last_ms) and
the wall time of the synchronous thip_ccsets_run_device call (trajectories
already on the device; values, jacobians, coefficients, counts and keys back on
the host).  thip_eval_collision: the wall time of its synchronous call (host
trajectories in, records out with a per-problem capacity sized to the fullest
problem).  The two alternate inside one timed loop after warm runs; medians and
the spread (min, max) of --runs repeats (at least 20).  Both use config C's
margin, coefficient and buffer on the initial trajectories moved by
0.03 N(0, 1) so that there are contacts.  For the first 64 problems every
segment's number of sets must equal the number of distinct (link, other,
sphere) keys among thip_eval_collision's records of that segment.  Needs an AMD
GPU; there is no fallback."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "trajopt-1_amd"))

from trajopt_amd import abi, problems  # noqa: E402
from trajopt_amd.runtime import ContinuousCollisionSets, TermEvaluator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ccsets_bench.json"))
    a = ap.parse_args()
    runs = max(a.runs, 20)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("ccsets_bench: no GPU")
    wl = problems.make_workload("C", a.batch)
    B, N, D = wl.batch, wl.n_steps, wl.n_dof
    rng = np.random.default_rng(1)
    x = np.ascontiguousarray(wl.init + 0.03 * rng.standard_normal(wl.init.shape))
    d = abi.ProblemDesc.from_buffer_copy(wl.desc)
    margin, coeff, buffer, lvs = d.coll_margin, d.coll_coeff, d.coll_buffer, d.coll_lvs
    # the same term for thip_eval_collision: LVS_CONTINUOUS, every step pair, no fixed steps
    d.coll_continuous, d.coll_first_step, d.coll_last_step, d.coll_n_fixed = 1, 0, N - 1, 0
    d.coll_contact_test = abi.CONTACT_ALL
    ev_wl = problems.Workload("ccsets-bench", d, x, wl.targets, wl.scene, x)

    cs = ContinuousCollisionSets(d, B, wl.scene, abi.CcsetsConfig(margin, coeff, buffer, a.rows, 0, N - 1,
                                                                   abi.EVALUATOR_LVS_CONTINUOUS, lvs))
    ev = TermEvaluator(ev_wl)
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    # thip_eval_collision returns [batch][cap] records: size cap to the fullest problem, not to a default
    cap = 64 * (max(len(r) for r in ev.collision(0, x)) // 64 + 1)
    for _ in range(a.warmup):
        out = cs.run_device(d_x.data_ptr())
        recs = ev.collision(0, x, cap=cap)
    kernel_ms, call_ms, eval_ms = [], [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = cs.run_device(d_x.data_ptr())
        call_ms.append((time.perf_counter() - t0) * 1e3)
        kernel_ms.append(cs.kernel_ms())
        t0 = time.perf_counter()
        recs = ev.collision(0, x, cap=cap)
        eval_ms.append((time.perf_counter() - t0) * 1e3)
    values, jac, coeffs, counts, keys = out
    # agreement: a segment's set count is the number of distinct keys among its records
    bad = 0
    for b in range(min(B, 64)):
        r = recs[b]
        for t in range(N - 1):
            rt = r[r[:, 0] == t]
            n_keys = len({(int(v[1]), int(v[2]), int(v[3])) for v in rt})
            if n_keys != counts[b, t]:
                bad += 1
    contacts = int(sum(len(r) for r in recs))
    cs.close()
    ev.close()

    def stat(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}

    res = {
        # the settings that shape the measurement (where the file goes does not)
        "cmd": f"python tools/ccsets_bench.py --batch {a.batch} --runs {runs} --warmup {a.warmup} --rows {a.rows}",
        "workload": f"config C, {B} problems x {N - 1} segments, LVS_CONTINUOUS, lvs {lvs}, {d.n_spheres} robot "
                    f"spheres, {d.n_prims} primitives, {len(abi_self_pairs(d))} self sphere pairs, max_num_cnt {a.rows}",
        "runs": runs, "warmup": a.warmup,
        "contacts_in_batch": contacts, "sets_in_batch": int(counts.sum()),
        "sets_kept": int(np.minimum(counts, a.rows).sum()),
        "ccsets_kernel": stat(kernel_ms),
        "ccsets_run_device_call": stat(call_ms),
        "eval_collision_lvs_continuous_call": stat(eval_ms),
        "eval_collision_record_capacity_per_problem": cap,
        "output_bytes_ccsets": int(sum(o.nbytes for o in out)),
        "output_bytes_eval_collision": int(contacts * (8 + 2 * D + 1) * 8),
        "segments_disagreeing_of_first_64_problems": bad,
    }
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    if bad:
        raise SystemExit(f"ccsets_bench: {bad} segments disagree with thip_eval_collision")


def abi_self_pairs(d):
    return [(i, j) for k in range(d.n_self_pairs) for i in range(d.n_spheres) if d.sphere_link[i] == d.self_pair[k][0]
            for j in range(d.n_spheres) if d.sphere_link[j] == d.self_pair[k][1]]


if __name__ == "__main__":
    main()
