#!/usr/bin/env python3
"""Time one collision-set launch (thip_csets_*, coll_sets.hip) on config C's
robot and scene -- 1,024 problems x 30 nodes, max_num_cnt 3 -- next to
thip_eval_collision on the same inputs with the DISCRETE evaluator, which
computes every contact's jacobian and returns every record to the host.

  python tools/csets_bench.py [--batch 1024] [--runs 30] [--out FILE.json]

Collision sets: the HIP-event time of csets_kernel (thip_csets_last_ms) and the
wall time of the synchronous thip_csets_run_device call (trajectories already
on the device; values, jacobians, coefficients, counts and keys back on the
host).  thip_eval_collision: the wall time of its synchronous call (host
trajectories in, records out with a per-problem capacity sized to the fullest
problem; it has no device-trajectory form).  The two
alternate inside one timed loop after warm runs; medians and the spread
(min, max) of --runs repeats (at least 20).  Both use margin 0.025, coefficient
20 and buffer 0.05 (config C's), on the initial trajectories moved by
0.03 N(0, 1) so that there are contacts.  The first rows agree: every
collision-set value is margin - distance of a record of the same node.  Needs
an AMD GPU; there is no fallback."""
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
from trajopt_amd.runtime import CollisionSets, TermEvaluator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "csets_bench.json"))
    a = ap.parse_args()
    runs = max(a.runs, 20)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("csets_bench: no GPU")
    wl = problems.make_workload("C", a.batch)
    B, N, D = wl.batch, wl.n_steps, wl.n_dof
    rng = np.random.default_rng(1)
    x = np.ascontiguousarray(wl.init + 0.03 * rng.standard_normal(wl.init.shape))
    d = abi.ProblemDesc.from_buffer_copy(wl.desc)
    margin, coeff, buffer = d.coll_margin, d.coll_coeff, d.coll_buffer
    # the same term for thip_eval_collision: DISCRETE, every node, no fixed steps
    d.coll_continuous, d.coll_first_step, d.coll_last_step, d.coll_n_fixed = 2, 0, N - 1, 0
    d.coll_contact_test = abi.CONTACT_ALL
    ev_wl = problems.Workload("csets-bench", d, x, wl.targets, wl.scene, x)

    cs = CollisionSets(d, B, wl.scene, abi.CsetsConfig(margin, coeff, buffer, a.rows, 0, N - 1))
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
    # agreement: a node's set count is its record count, its first value the largest margin - distance
    bad = 0
    for b in range(min(B, 64)):
        r = recs[b]
        for t in range(N):
            rt = r[r[:, 0] == t]
            if len(rt) != counts[b, t] or (len(rt) and abs(values[b, t, 0] - (margin - rt[:, 5].min())) > 1e-12):
                bad += 1
    contacts = int(sum(len(r) for r in recs))
    cs.close()
    ev.close()

    def stat(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}

    res = {
        # the settings that shape the measurement (where the file goes does not)
        "cmd": f"python tools/csets_bench.py --batch {a.batch} --runs {runs} --warmup {a.warmup} --rows {a.rows}",
        "workload": f"config C, {B} problems x {N} nodes, {d.n_spheres} robot spheres, {d.n_prims} primitives, "
                    f"{len(abi_self_pairs(d))} self sphere pairs, max_num_cnt {a.rows}",
        "runs": runs, "warmup": a.warmup,
        "contacts_in_batch": contacts, "sets_kept": int(np.minimum(counts, a.rows).sum()),
        "csets_kernel": stat(kernel_ms),
        "csets_run_device_call": stat(call_ms),
        "eval_collision_discrete_call": stat(eval_ms),
        "eval_collision_record_capacity_per_problem": cap,
        "output_bytes_csets": int(sum(o.nbytes for o in out)),
        "output_bytes_eval_collision": int(contacts * (8 + 2 * D + 1) * 8),
        "nodes_disagreeing_of_first_64_problems": bad,
    }
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    if bad:
        raise SystemExit(f"csets_bench: {bad} nodes disagree with thip_eval_collision")


def abi_self_pairs(d):
    return [(i, j) for k in range(d.n_self_pairs) for i in range(d.n_spheres) if d.sphere_link[i] == d.self_pair[k][0]
            for j in range(d.n_spheres) if d.sphere_link[j] == d.self_pair[k][1]]


if __name__ == "__main__":
    main()
