"""The CartPose case table (tests/pose_cases.py) and the oracle's pose arithmetic against
the independent long-double reference (tests/pose_reference.py), on the CPU.  This module
is what validates the table: an entry that fails here is wrong and is corrected, not
removed.  tests/test_gpu_pose_error.py runs the same table through every device entry.

Bars (pose_cases.TOL_*): error 1e-12 and Jacobian 1e-9, absolute, tests/test_gpu.py's own
(an error of 1e-14 becomes 1e-9 behind the forward difference's 1 / 1e-5).  They are usable
only if the oracle alone stays inside them: test_oracle_against_the_reference checks that
on every batch and prints the worst gap: over the 191 cases error 2.0e-15 and Jacobian
3.1e-10 (both on tiltbot), the restatement below 1.4e-15 and 2.2e-10 (DESIGN.md section 5
has the table with the device's figures).

Teeth: a double restatement of the kernels' rot_error, apply_tolerances and wrap switch
lives here with switchable mutations.  Unmutated it passes every case; MUTATIONS names,
for each mutation, a case that must go red.  `wrap_threshold_half_pi` is listed as
unobservable: a forward step of 1e-5 moves a [-pi, pi] rotation vector by 1e-5 unless it
wraps, and a wrap moves the component on the axis' largest entry by at least
2 pi / sqrt 3 = 3.63 > pi, so no case has a largest rotation jump between pi / 2 and pi.
"""
import math

import numpy as np
import pytest

import pose_cases as pc
import pose_reference as pr

LD = pr.LD


# ------------------------------------------------------------------ the table itself
def test_table_shape():
    assert all(1 <= len(b[4]) <= 64 for b in pc.BATCHES), [(b[0], len(b[4])) for b in pc.BATCHES]
    assert sum(len(b[4]) for b in pc.BATCHES) == len(pc.CASES)
    either = [c["name"] for c in pc.CASES if c.get("either_sign")]
    assert len(either) <= 4 and all(n.endswith("_pi_inexact") for n in either), either
    assert {c["family"] for c in pc.CASES} == {"tiny", "branches", "pi", "joint", "translation", "bands", "wrap", "seam"}
    assert {b[1] for b in pc.BATCHES} == {"posebot", "tiltbot", "posebot_dyn"}
    for fam, chains in (("joint", {"posebot", "tiltbot"}), ("translation", {"posebot", "tiltbot"}),
                        ("wrap", {"posebot", "posebot_dyn"})):
        assert {c["chain"] for c in pc.CASES if c["family"] == fam} == chains
    for c in pc.CASES:
        if c["family"] == "translation":
            assert c["offset"] == "off"
    print({b[0]: len(b[4]) for b in pc.BATCHES})


def _E(c, q=None, dtype=LD):
    return pr.error_pose(pc.CHAINS[c["chain"]], c["q"] if q is None else q, pc.TOOL, pc.OFFSETS[c["offset"]],
                         pc.target_link(c["chain"]), c["target"], dtype)


def test_posebot_error_rotation_is_the_targets_transpose():
    """What the exact cases rely on, in double and in long double."""
    n = 0
    for c in pc.CASES:
        if c["chain"] != "tiltbot" and not c["q"][3:].any() and c["offset"] == "ident":
            Rt = c["target"].reshape(3, 4)[:, :3].T
            for dt in (np.float64, LD):
                assert np.array_equal(_E(c, dtype=dt)[:3, :3], Rt.astype(dt)), c["name"]
            n += 1
        if c["family"] == "bands" and c["chain"] == "posebot" and np.array_equal(c["target"], pc.IDENT):
            assert np.array_equal(_E(c, dtype=np.float64)[:3, 3], c["q"][:3]), c["name"]
    assert n >= 100


def test_log_then_exp_returns_the_rotation():
    worst = 0.0
    angles = [1e-9, 1e-3, 1.0, 2 * math.pi / 3 - 1e-3, 2 * math.pi / 3 + 1e-3, 2.5, math.pi - 1e-5, math.pi - 1e-9]
    for _, ax in pc.AXES7 + [(None, a) for _, _, a in pc.DOMINANT]:
        a = np.asarray(ax, dtype=LD)
        a = a / np.sqrt(np.sum(a * a))
        for th in angles:
            R = pr.rodrigues(a, th)
            pm, tp = pr.rotvec(R)
            for v in (pm, tp):
                worst = max(worst, float(np.abs(pr.exp(v) - R).max()))
    print(f"exp(log R) - R: worst {worst:.3e}")
    assert worst <= 1e-17


def _double_branch(R):
    """(Shoemake branch, sign of Eigen's w) read off a double matrix."""
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return ("w", +1)
    i = pr.first_argmax(np.diag(R))
    j, k = (i + 1) % 3, (i + 2) % 3
    return (i, +1 if R[k, j] - R[j, k] >= 0 else -1)


def test_branches_are_covered():
    """Family 2 takes the branch it says it takes.  The trace branch has w > 0 by
    construction (w = sqrt(trace + 1) / 2); the three others come with both signs."""
    seen = set()
    for c in pc.CASES:
        if "branch" in c:
            got = _double_branch(_E(c, dtype=np.float64)[:3, :3])
            assert got == c["branch"], (c["name"], got)
            seen.add(got)
    assert seen == {("w", +1)} | {(i, s) for i in range(3) for s in (+1, -1)}


def test_every_decision_has_a_margin():
    """The sign of the trace and the diagonal's arg-max of every error rotation a case
    evaluates (its own and the six perturbed ones) are decided by more than rounding, or by
    an exact tie: 1e-7 against 1e-16."""
    for c in pc.CASES:
        D = pc.CHAINS[c["chain"]].n_dof
        for q in [c["q"]] + [pr.perturbed(c["q"], p) for p in range(D)]:
            R = _E(c, q)[:3, :3]
            Rd = np.asarray(R, dtype=np.float64)
            tr = float(R[0, 0] + R[1, 1] + R[2, 2])
            assert abs(tr) > 1e-7, (c["name"], tr)
            if tr < 0 and c["chain"] == "tiltbot":
                d = np.sort(np.diag(Rd))
                assert d[2] - d[1] > 1e-7, (c["name"], d)
            if "tied" in c and q is c["q"]:
                i, j = c["tied"]
                assert Rd[i, i] == Rd[j, j] and tr < 0 and pr.first_argmax(np.diag(Rd)) == i, c["name"]


def test_stated_jacobian_features():
    """The seam's jump where the table says (and nowhere else), the columns of an FD step
    across a band edge, the zero columns of the joints upstream of both frames."""
    for batch in pc.BATCHES:
        _, chain, band, _, cases = batch
        e_ref, j_ref = pc.reference(batch)
        for b, c in enumerate(cases):
            rotJ = np.abs(j_ref[b][3:]).astype(np.float64)
            for p in c.get("jump", ()):
                E0, E1 = _E(c), _E(c, pr.perturbed(c["q"], p))
                s0 = pr.eigen_w_nonneg(E0[:3, :3], *pr.quaternion(E0[:3, :3]))[0]
                s1 = pr.eigen_w_nonneg(E1[:3, :3], *pr.quaternion(E1[:3, :3]))[0]
                assert s0 != s1, c["name"]
                assert rotJ[:, p].max() > 1e5, (c["name"], rotJ[:, p])
            rotJ = np.delete(rotJ, list(c.get("jump", ())), axis=1)
            assert rotJ.max() < 10.0, (c["name"], rotJ.max())  # smooth: of order 1, not 2 pi / 1e-5
            if "column" in c:
                r, p, v = c["column"]
                assert abs(float(j_ref[b][r, p]) - v) < 1e-6, (c["name"], float(j_ref[b][r, p]))
            if c["family"] == "seam" and c["name"].endswith("straddle") and "jump" not in c and band == "none":
                E0, E1 = _E(c), _E(c, pr.perturbed(c["q"], 4))  # the control crosses trace = 0 without a jump
                assert (E0[:3, :3].trace() > 0) != (E1[:3, :3].trace() > 0), c["name"]
            if chain == "posebot_dyn":
                assert np.abs(j_ref[b][:, :4]).max() < 1e-12, c["name"]
                assert np.abs(j_ref[b][:, 4:]).max() > 0.1, c["name"]


# ------------------------------------------------------------------ the oracle
def oracle_linearize(oracle_mod, batch):
    wl = pc.make_workload(batch)
    err, jac = oracle_mod.linearize(wl, wl.init)
    return err[:, 0], jac[:, 0]


@pytest.mark.parametrize("batch", pc.BATCHES, ids=pc.BATCH_IDS)
def test_oracle_against_the_reference(oracle_mod, batch):
    err, jac = oracle_linearize(oracle_mod, batch)
    worst = pc.check(batch, err, jac, f"oracle/{batch[0]}")
    print(f"oracle {batch[0]}: worst vs reference: error {worst[0]:.3e} jacobian {worst[1]:.3e}")


# ------------------------------------------------------------------ the restatement and its mutations
TWO_PI = 2.0 * math.pi
DBL_EPS = 2.220446049250313e-16


def rot_error(R, two_pi, mut=()):
    """kin_device.hpp rot_error / oracle kin.cpp rotErr in double, with mutations."""
    f = np.float64
    t = R[0, 0] + R[1, 1] + R[2, 2]
    v = [f(0.0)] * 3
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        v = [(R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t]
    else:
        i = 0
        if "i_fixed_at_0" not in mut:
            if "last_argmax" in mut:
                if R[1, 1] >= R[0, 0]:
                    i = 1
                if R[2, 2] >= R[i, i]:
                    i = 2
            else:
                if R[1, 1] > R[0, 0]:
                    i = 1
                if R[2, 2] > R[i, i]:
                    i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        v[i] = 0.5 * t
        t = 0.5 / t
        w = (R[k, j] - R[j, k]) * t
        v[j] = (R[j, i] + R[i, j]) * t
        v[k] = (R[k, i] + R[i, k]) * t
    n = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if n < DBL_EPS:
        sc = max(abs(v[0]), abs(v[1]), abs(v[2]))
        if sc > 0:
            a, b, c = v[0] / sc, v[1] / sc, v[2] / sc
            n = sc * np.sqrt(a * a + b * b + c * c)
        else:
            n = f(0.0)
    if n != 0:
        ang = 2 * np.arctan2(n, abs(w))
        sg = -1.0 if w < 0 else 1.0
        ax = [sg * v[0] / n, sg * v[1] / n, sg * v[2] / n]
    else:
        ang, ax = f(0.0), [f(1.0), f(0.0), f(0.0)]
    if "no_sign_fix" not in mut:
        dot = v[0] * ax[0] + v[1] * ax[1] + v[2] * ax[2]
        s = -1.0 if dot < 0 else 1.0
        ang = s * ang
        ax = [s * a for a in ax]
    ang = np.copysign(np.fmod(abs(ang), TWO_PI), ang)
    if two_pi:
        if ang < 0:
            ang += TWO_PI
        elif ang > TWO_PI:
            ang -= TWO_PI
    else:
        if ang < -math.pi:
            ang += TWO_PI
        elif ang > math.pi:
            ang -= TWO_PI
    return np.array([ax[0] * ang, ax[1] * ang, ax[2] * ang], dtype=f)


def apply_tolerances(e, lower, upper, mut=()):
    out = np.zeros(6)
    for i in range(6):
        if "band_le_other_bound" in mut:
            # `<=` / `>=`, and the excess taken from the other bound
            out[i] = e[i] - upper[i] if e[i] <= lower[i] else (e[i] - lower[i] if e[i] >= upper[i] else 0.0)
        else:
            out[i] = e[i] - lower[i] if e[i] < lower[i] else (e[i] - upper[i] if e[i] > upper[i] else 0.0)
    return out


def restated(batch, mut=()):
    """(err [B, 6], jac [B, 6, D]) of a batch by the double restatement."""
    _, chain, band, _, cases = batch
    tol = pc.BANDS[band]
    errs, jacs = [], []
    with np.errstate(all="ignore"):
        for c in cases:
            D = pc.CHAINS[chain].n_dof
            E0 = _E(c, dtype=np.float64)
            e = np.concatenate([E0[:3, 3], rot_error(E0[:3, :3], False, mut)])
            errs.append(e if tol is None else apply_tolerances(e, *tol, mut))
            J = np.zeros((6, D))
            for p in range(D):
                E1 = _E(c, pr.perturbed(c["q"], p), dtype=np.float64)
                if tol is None:
                    form = "pm_in_untoleranced_fd" not in mut
                    d = np.concatenate([E1[:3, 3] - E0[:3, 3],
                                        rot_error(E1[:3, :3], form, mut) - rot_error(E0[:3, :3], form, mut)])
                else:
                    e0 = np.concatenate([E0[:3, 3], rot_error(E0[:3, :3], False, mut)])
                    e1 = np.concatenate([E1[:3, 3], rot_error(E1[:3, :3], False, mut)])
                    thr = math.pi / 2 if "wrap_threshold_half_pi" in mut else math.pi
                    if np.any(np.abs(e1[3:] - e0[3:]) > thr):
                        e0[3:] = rot_error(E0[:3, :3], True, mut)
                        e1[3:] = rot_error(E1[:3, :3], True, mut)
                    d = apply_tolerances(e1, *tol, mut) - apply_tolerances(e0, *tol, mut)
                J[:, p] = d / pr.EPS
            jacs.append(J)
    return np.array(errs), np.array(jacs)


def test_restatement_passes_every_case():
    worst = [0.0, 0.0]
    for batch in pc.BATCHES:
        w = pc.check(batch, *restated(batch), f"restated/{batch[0]}")
        worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"restatement vs reference: error {worst[0]:.3e} jacobian {worst[1]:.3e}")


# mutation -> a case that must go red (None: unobservable, see the module docstring)
MUTATIONS = {
    "no_sign_fix": "wrap_none_z_pi_m5e-6",
    "i_fixed_at_0": "pi_about_y",
    "last_argmax": "seam_none_oblique_tied_diagonal",
    "wrap_threshold_half_pi": None,
    "band_le_other_bound": "band_sym_tx_upper_on",
    "pm_in_untoleranced_fd": "wrap_none_z_pi_m5e-6",
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_mutation_goes_red(mutation):
    red = []
    for batch in pc.BATCHES:
        red += pc.failing(batch, *restated(batch, (mutation,)))
    print(f"{mutation}: {len(red)} cases red: {red[:12]}")
    if MUTATIONS[mutation] is None:
        assert not red, f"{mutation} is listed as unobservable, but fails {red}"
    else:
        assert MUTATIONS[mutation] in red, f"{mutation}: {MUTATIONS[mutation]} stays green (red: {red})"
