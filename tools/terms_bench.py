#!/usr/bin/env python3
"""Time the batched term-value evaluator (thip_terms_*) on config C's 1,024
30-waypoint problems next to the route that gave per-term values before it:
thip_eval_cart_pose_all for the CartPose errors plus thip_eval_collision for
every contact record of the collision term, the costs summed on the host.

  python tools/terms_bench.py [--batch 1024] [--runs 15] [--out FILE.json]

New route: the wall time of thip_terms_run_device (synchronous: trajectories
already on the device, [batch][n_costs] doubles back) and the HIP-event time of
its kernels (thip_terms_last_ms).  Earlier route: the wall time of the two
thip_eval_* calls (synchronous, host arrays) and of the numpy sums, and the two
calls' share of it apart.  Warm runs first, then the median of --runs (at least
10).  The two must agree per slot within 1e-12 x summands x max(1,
coefficient).  Needs an AMD GPU; there is no fallback."""
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
from trajopt_amd.runtime import TermEvaluator, TermValues  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "terms_bench.json"))
    a = ap.parse_args()
    runs = max(a.runs, 10)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("terms_bench: no GPU")
    wl = problems.make_workload("C", a.batch)
    d = wl.desc
    B, N, D = wl.batch, wl.n_steps, wl.n_dof
    # the initial trajectories moved a little, so that the collision slots are not all empty
    rng = np.random.default_rng(1)
    x = np.ascontiguousarray(wl.init + 0.03 * rng.standard_normal(wl.init.shape))

    # ---- the term-value evaluator
    tv = TermValues(wl)
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        costs, viols = tv.run_device(d_x.data_ptr())
    kernel_ms, call_ms = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        costs, viols = tv.run_device(d_x.data_ptr())
        call_ms.append(1e3 * (time.perf_counter() - t0))
        kernel_ms.append(tv.kernel_ms())
    slots = tv.slots
    tv.close()

    # ---- the earlier route: CartPose errors and every contact record, summed on the host
    ev = TermEvaluator(wl)
    lib = ev.lib
    dp = C.POINTER(C.c_double)
    lib.thip_eval_cart_pose_all.argtypes = [C.c_void_p, dp, dp, dp]
    lib.thip_eval_cart_pose_all.restype = C.c_int
    W = 8 + 2 * D + 1
    err = np.zeros((B, d.n_cart, 6))
    cnt = (C.c_int * B)()
    one = np.zeros(W)
    for _ in range(2):  # counts only (cap 0); the first call also sizes the per-unit staging
        assert lib.thip_eval_collision(ev.ev, 0, x.ctypes.data_as(dp), one.ctypes.data_as(dp), 0, cnt) == 0
    cap = max(max(cnt), 1)
    rec = np.zeros((B, cap, W))
    cf = np.array([[d.cart_pos_coeffs[k][i] for i in range(3)] + [d.cart_rot_coeffs[k][i] for i in range(3)]
                   for k in range(d.n_cart)])
    cf = np.where(np.abs(cf) > 1e-5, cf, 0.0)
    jv_c, jv_t = np.array(d.jv_coeffs[:D]), np.array(d.jv_targets[:D])
    units = [s.unit for s in slots if s.kind == abi.TERM_COLL]
    old_ms, old_calls_ms, old_costs = [], [], None
    for k in range(a.warmup + runs):
        t0 = time.perf_counter()
        assert lib.thip_eval_cart_pose_all(ev.ev, x.ctypes.data_as(dp), err.ctypes.data_as(dp), None) == 0
        assert lib.thip_eval_collision(ev.ev, 0, x.ctypes.data_as(dp), rec.ctypes.data_as(dp), cap, cnt) == 0
        t_calls = time.perf_counter()  # the two device calls; what follows is numpy on the host
        n = np.array(list(cnt))
        vel = np.diff(x, axis=1) - jv_t
        jv = (vel * vel * jv_c).sum(axis=(1, 2))
        cart = (np.abs(err) * cf).sum(axis=2)
        live = np.arange(cap)[None, :] < n[:, None]
        pen = np.where(live, d.coll_coeff * np.maximum(d.coll_margin - rec[:, :, 5], 0.0), 0.0)
        t_of = rec[:, :, 0].astype(int)
        coll = np.stack([np.where(t_of == u, pen, 0.0).sum(axis=1) for u in units], axis=1)
        old_costs = np.concatenate([jv[:, None], cart, coll], axis=1)
        if k >= a.warmup:
            old_ms.append(1e3 * (time.perf_counter() - t0))
            old_calls_ms.append(1e3 * (t_calls - t0))
    ev.close()

    # ---- the two routes agree
    assert d.n_coll_pairs == 0 and not d.coll_is_cnt and old_costs.shape == costs.shape
    contacts = np.array([((t_of == s.unit) & live).sum(axis=1).max() if s.kind == abi.TERM_COLL else 0 for s in slots])
    worst = 0.0
    for i, s in enumerate(slots):
        summands = {abi.TERM_JOINT_VEL: (N - 1) * D, abi.TERM_CART: 6}.get(s.kind, max(1, int(contacts[i])))
        coeff = {abi.TERM_JOINT_VEL: np.abs(jv_c).max(), abi.TERM_CART: np.abs(cf).max()}.get(s.kind, abs(d.coll_coeff))
        diff = float(np.abs(costs[:, i] - old_costs[:, i]).max())
        worst = max(worst, diff)
        assert diff <= 1e-12 * summands * max(1.0, coeff), (i, diff)

    new, old = statistics.median(call_ms), statistics.median(old_ms)
    out = {
        "workload": f"config C, {B} problems x {N} waypoints, {len(slots)} slots per problem, "
                    f"{int(n.sum())} contacts in the batch",
        "runs": runs,
        "terms_run_device_call_ms_median": new,
        "terms_run_device_call_ms_min_max": [min(call_ms), max(call_ms)],
        "terms_kernels_ms_median": statistics.median(kernel_ms),
        "terms_kernels_ms_min_max": [min(kernel_ms), max(kernel_ms)],
        "eval_route_call_ms_median": old,
        "eval_route_call_ms_min_max": [min(old_ms), max(old_ms)],
        "eval_route_device_calls_only_ms_median": statistics.median(old_calls_ms),
        "eval_route_device_calls_only_ms_min_max": [min(old_calls_ms), max(old_calls_ms)],
        "ratio_eval_device_calls_only_over_terms": statistics.median(old_calls_ms) / new,
        "ratio_eval_route_over_terms": old / new,
        "max_abs_slot_difference": worst,
    }
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
