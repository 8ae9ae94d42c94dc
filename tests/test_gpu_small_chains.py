"""1- to 5-DoF chains on the fused SQP kernel (MI355X): the widths below the lane octet.

Every other solve the suite checks against the oracle runs a chain of 6, 7, 8 or
14 dofs, so the narrow path's width-dependent code -- a waypoint block padded with
identity from D up to 8 lanes, the clamped ic / kc of seg_chain_solve,
masked_dot<kOct>'s runtime length, chol_inv_block_reg's padding inside an octet,
seg_b_slot's stride of 8 -- has only met pads of 0, 1 and 2 lanes.  The chains here
are robots.ROBOTS' right_arm_1dof ... right_arm_5dof: the PR2 right arm with all but
its first k moving joints held fixed at 0 (the way right_arm_6dof holds the wrist
roll), so the links, the tool frame, the collision spheres and the scenes are those
of right_arm.

Three paths, each named by the layout the context reports (thip_debug_solve_layout)
and asserted before anything is solved:
  * the register-resident ADMM segment (one waypoint per block, D = 1..5);
  * the generic step with narrow blocks (64 waypoints: outside the segment);
  * waypoint pairs (a JointAccEqCost: Layout::grp = 2, blocks of 2 k dofs over N / 2
    pairs).  With k <= 4 the pair block is narrow (sD = 2, 4, 6, 8 <= 8) and must
    still run the generic step: the segment's chain pack, its middle block and its
    P x know one waypoint per block and no (t, t + 2) coupling.  k = 5 gives
    sD = 10, the first width past the octet (the wide path, so far run at 14 and
    16 only).

Every solve goes through the frozen parity gate (tests/parity.py check_parity,
default arguments) against the oracle, batch 8, first_problem 0.  On the CPU the
oracle's exact build under the gate's jitter (six seeds) moves these workloads'
trajectories by at most 1e-5 with no status flip, so the reference determines the
outcomes and a kernel that is subtly wrong on them finds no excuse.  Two shapes of
the grid miss that CPU check at first_problem 0 and run on another window, chosen
by the same check (exact build, the gate's JITTER, seeds 1..6, plus the fast build):
  * B on 2 dofs at 3 waypoints: 1.4e-5 at first_problem 0; problems 8..15 stay at 4.2e-7;
  * C on 4 dofs: 8.6e-4 at first_problem 0; problems 8..15 stay at 5.7e-8
(MOVED; no status flips in either window).
"""
import numpy as np
import pytest

from parity import check_parity
from trajopt_amd import abi, problems
from trajopt_amd.runtime import BatchTrustRegionSQP, HipError

pytestmark = pytest.mark.gpu

BATCH = 8
# shapes whose oracle outcome is not stable at first_problem 0 (module docstring): id -> first_problem
MOVED = {"B-d2-n3": 8, "C-d4": 8}


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()  # raises if the HIP library is missing
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


def _base(name):
    """'<cfg>-d<k>[-n<N>]' -> the workload (config J starts 0.05 off its goal)."""
    parts = name.split("-")
    cfg, k = parts[0], int(parts[1][1:])
    n_steps = int(parts[2][1:]) if len(parts) > 2 else None
    return problems.make_workload(cfg, BATCH, first_problem=MOVED.get(name, 0), n_steps=n_steps,
                                  goal_offset=0.05 if cfg == "J" else 0.0, robot=f"right_arm_{k}dof")


def _workload(name):
    if name == "B-acc2-d2":
        # two JointAccEqCost terms, the second on steps 10..20 (test_gpu.py's B-acc-two-terms)
        wl = problems.with_joint_acc(_base("B-d2"), coeff=1.0)
        return problems.with_joint_acc(wl, coeff=3.0, target=-0.002, first_step=10, last_step=20)
    if "-acc-" in name:
        return problems.with_joint_acc(_base(name.replace("-acc", "")))
    return _base(name)


SEGMENT = ([f"{cfg}-d{k}" for cfg in "JBC" for k in range(1, 6)] + [f"B-d{k}-n3" for k in range(1, 6)])
GENERIC = [f"B-d{k}-n64" for k in range(1, 5)]
PAIRS = ([f"{cfg}-acc-d{k}" for cfg in "JBC" for k in range(1, 5)]
         + [f"B-acc-d{k}-n{n}" for n in (4, 64) for k in range(1, 5)]
         + ["J-acc-d5", "B-acc-d5", "B-acc2-d2"])


def _dofs(name):
    return int(next(p for p in name.split("-") if p[0] == "d" and p[1:].isdigit())[1:])


def _layout(wl):
    s = BatchTrustRegionSQP(wl)  # creates the context; nothing is solved
    lay = s.layout()
    s.close()
    return lay


def _expect(lay, **want):
    got = {k: lay[k] for k in want}
    assert got == want, f"layout {lay}, expected {want}"


@pytest.fixture(scope="module")
def reference(oracle_mod):
    """Each workload and its oracle solve, made once and shared (never modified)."""
    cache = {}

    def get(name):
        if name not in cache:
            wl = _workload(name)
            cache[name] = (wl, oracle_mod.solve(wl, n_threads=16))
        return cache[name]

    return get


def _solve(wl):
    s = BatchTrustRegionSQP(wl, device=0)
    lay = s.layout()
    x, res = s.optimize()
    s.close()
    return lay, x, res


def _gate(wl, oracle_mod, ref, x, res, label):
    assert all(r.flags == 0 for r in res), f"{label}: flags {[r.flags for r in res]}"
    rec = check_parity(wl, oracle_mod, x, res, label=label, oracle=ref)
    print(f"{label}: strict {rec['strict']}/{rec['batch']}, max_dx_strict {rec['max_dx_strict']:.2e}, "
          f"excused {rec['excused']}")
    return rec


# ------------------------------------------------------------------ layout facts (no solve)
@pytest.mark.parametrize("k", range(1, 6))
def test_layout_one_waypoint_per_block(k):
    """B / C (30 waypoints) and J (10) on k dofs run the segment on k-wide blocks; B at 64
    waypoints is outside the segment's 32 and runs the generic-step build, still narrow."""
    for cfg in "BCJ":
        _expect(_layout(_base(f"{cfg}-d{k}")), block_dofs=k, wide=0, grp=1, seg_ok=1, gen=0)
    _expect(_layout(_base(f"B-d{k}-n64")), block_dofs=k, wide=0, grp=1, seg_ok=0, gen=1)


@pytest.mark.parametrize("k", range(1, 5))
def test_layout_narrow_pairs_stay_off_the_segment(k):
    """A JointAccEqCost on k <= 4 dofs: pair blocks of 2 k <= 8 dofs are narrow, and the
    segment -- one waypoint per block -- must not take them (seg_ok == 0, the generic-step
    build), at 4, 10 and 30 waypoints alike."""
    for name, n in ((f"B-acc-d{k}-n4", 4), (f"J-acc-d{k}", 10), (f"B-acc-d{k}", 30), (f"C-acc-d{k}", 30)):
        _expect(_layout(_workload(name)), grp=2, block_dofs=2 * k, blocks=n // 2, wide=0, seg_ok=0, gen=1)


def test_layout_pairs_on_5_dofs_are_wide():
    for name in ("J-acc-d5", "B-acc-d5"):
        _expect(_layout(_workload(name)), grp=2, block_dofs=10, wide=1, seg_ok=0, gen=1)


def test_joint_acc_on_two_waypoints_is_refused():
    """with_joint_acc's hatch clamping gives first_step = -1 on 2 waypoints: thip_create
    refuses the range instead of indexing x with it."""
    wl = problems.with_joint_acc(problems.make_workload("B", 2, n_steps=2, robot="right_arm_2dof"))
    assert wl.desc.jdt_first_step[0] == -1
    with pytest.raises(HipError) as ei:
        BatchTrustRegionSQP(wl)
    assert "jdt_first_step" in str(ei.value) and "jdt_last_step" in str(ei.value)


# ------------------------------------------------------------------ parity against the oracle
@pytest.mark.parametrize("name", SEGMENT)
def test_sqp_parity_segment(oracle_mod, reference, name):
    wl, ref = reference(name)
    lay, x, res = _solve(wl)
    _expect(lay, block_dofs=_dofs(name), wide=0, grp=1, seg_ok=1, gen=0)
    _gate(wl, oracle_mod, ref, x, res, f"small-{name}")


@pytest.mark.parametrize("name", GENERIC)
def test_sqp_parity_generic_narrow_blocks(oracle_mod, reference, name):
    wl, ref = reference(name)
    lay, x, res = _solve(wl)
    _expect(lay, block_dofs=_dofs(name), wide=0, grp=1, seg_ok=0, gen=1)
    _gate(wl, oracle_mod, ref, x, res, f"small-{name}")


@pytest.mark.parametrize("name", PAIRS)
def test_sqp_parity_pairs(oracle_mod, reference, name):
    wl, ref = reference(name)
    lay, x, res = _solve(wl)
    k = _dofs(name)
    _expect(lay, grp=2, block_dofs=2 * k, blocks=wl.n_steps // 2, wide=int(k > 4), seg_ok=0, gen=1)
    _gate(wl, oracle_mod, ref, x, res, f"small-{name}")


FORCED = [("B-d2", abi.DEBUG_NO_SEGMENT), ("B-d2", abi.DEBUG_FORCE_WIDE), ("C-d3", abi.DEBUG_NO_SEGMENT),
          ("C-d3", abi.DEBUG_FORCE_WIDE), ("B-acc-d2", abi.DEBUG_FORCE_WIDE)]


@pytest.mark.parametrize("name,path", FORCED, ids=[f"{n}-{'generic' if p == abi.DEBUG_NO_SEGMENT else 'wide'}"
                                                    for n, p in FORCED])
def test_sqp_parity_forced_paths(oracle_mod, reference, hip, name, path):
    """The generic step and the wide-block solve (thip_debug_set_path) on small chains the
    segment would take, and narrow pairs run as wide pairs: the same gate, nothing else."""
    wl, ref = reference(name)
    assert hip.thip_debug_set_path(path) == 0
    try:
        lay, x, res = _solve(wl)
    finally:
        hip.thip_debug_set_path(0)
    assert lay["seg_ok"] == 0 and lay["wide"] == int(path == abi.DEBUG_FORCE_WIDE), lay
    _gate(wl, oracle_mod, ref, x, res, f"small-{name}-{'generic' if path == abi.DEBUG_NO_SEGMENT else 'wide'}")
