"""The discrete and the continuous collision sets against recorded bits (MI355X).

csets_kernel (csrc/coll_sets.hip) and ccsets_kernel (csrc/coll_sets_cont.hip)
share their key packing and their tie rule (csrc/coll_sets_common.hpp) and
repeat their prologue and their selection step.  Sharing or restructuring these
moves integer work and comparisons and no arithmetic of a distance or a
gradient, so each case here runs its sets and asks for the bits of the build
before the sharing, recorded in tests/golden/collsets_bits.npz: values, jac,
coeffs, counts and keys with np.array_equal.

The fixture pins bits.  It is written on the GPU by
tests/golden/make_golden_collsets_bits.py (which takes the cases from this file)
and is regenerated when the arithmetic of the sets changes on purpose, from a
build that tests/test_gpu_ifopt_sets.py and tests/test_gpu_ifopt_ccsets.py have
passed; a restructuring that is meant to keep the arithmetic must reproduce it
as it stands.

Cases, built with the builders of those two modules, for both kinds of set:
  spherebot   the hand cases at R = 1 and R = 3 (fewer sets than rows: padding);
  C           config C at 3 nodes, 2 problems (the second: other joint values and
              a shifted scene), R = 3 (more sets than rows) and R = 64 (fewer);
              the continuous sets with each evaluator type, seg_fixed None and
              (1, 2);
  274keys     19 primitives, 14 x 19 + 8 = 274 keys: the only case in which the
              running top R survives into a second pass;
  tie         two sets with the same error, bitwise: the order follows the key.
A case's inputs use no random numbers and no libm: the fixture holds outputs only,
one entry per field: the arrays of every run of every case, flattened, in the
order of CASES (an entry per array would cost more in headers than in data).
"""
from pathlib import Path

import numpy as np
import pytest

import ccsets_model as cm
import test_gpu_ifopt_ccsets as CC
import test_gpu_ifopt_sets as S
from trajopt_amd import abi
from trajopt_amd.runtime import CollisionSets, ContinuousCollisionSets

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "collsets_bits.npz"
FIELDS = ("values", "jac", "coeffs", "counts", "keys")
ETYPES = dict(zip(CC.ETYPE_IDS, CC.ETYPES))
SEG_FIXED = {"free": None, "fixed": (1, 2)}


def two_problems(scene, x):
    """The builders' problem and a second one: joint values moved by up to 0.03 rad in
    a fixed pattern (exact binary operations only), the scene shifted 1 cm in x."""
    step = ((np.arange(x.size) * 7 % 11) - 5.0).reshape(x.shape) * 0.006
    scenes = np.stack([scene, scene + 0.0])
    scenes[1, :, 1] += 0.01
    return scenes, np.concatenate([x, x + step])


def tie_desc(n_steps):
    """tests/test_gpu_ifopt_sets.py test_exact_tie_follows_the_key_not_the_candidate_order:
    two robot spheres and two primitives mirrored in y."""
    d = S.spherebot_desc(n_steps, n_prims=2)
    d.n_spheres = 2
    for s, y in enumerate((0.5, -0.5)):
        d.sphere_link[s], d.sphere_radius[s] = 3, 0.5
        d.sphere_center[s][0], d.sphere_center[s][1], d.sphere_center[s][2] = 0.0, y, 0.0
    scene = np.stack([S.sphere_rec((1.5, -0.75, 0.0), 0.5), S.sphere_rec((1.5, 0.75, 0.0), 0.5)])[None]
    return d, scene


def disc_runs(name):
    """The runs of a discrete case: (desc, scene [B, n_prims, 16], x [B, N, D], config)."""
    kind, _, R = name.partition("-R")
    R = int(R) if R else None
    if kind == "disc-spherebot":
        scene = np.stack([S.sphere_rec((0.0, 0.0, 0.0), 0.5)[None]] * len(S.SPHEREBOT_POSES))
        x = np.array([p for p, _, _ in S.SPHEREBOT_POSES]).reshape(len(S.SPHEREBOT_POSES), 1, 2)
        return [(S.spherebot_desc(), scene, x, abi.CsetsConfig(0.1, 1.0, 0.01, R, 0, 0))]
    if kind == "disc-C":
        d, scene, x = S.config_c(0)
        scenes, xs = two_problems(scene, x)
        return [(d, scenes, xs, abi.CsetsConfig(S.MARGIN, S.COEFF, S.BUFFER, R, 0, 2))]
    if kind == "disc-274keys":
        d, scene, x = S.config_c(9)
        return [(d, scene[None], x, abi.CsetsConfig(S.MARGIN, S.COEFF, S.BUFFER, 3, 0, 2))]
    assert kind == "disc-tie", name
    d, scene = tie_desc(1)
    return [(d, scene, np.array([[[0.5, 0.0]]]), abi.CsetsConfig(0.2, 1.0, 0.05, 2, 0, 0))]


def cont_runs(name):
    """The runs of a continuous case: (desc, scene, x, config, seg_fixed)."""
    kind, _, R = name.partition("-R")
    R = int(R) if R else None
    if kind == "cont-spherebot":
        scene = CC.sphere_rec((0.0, 0.0, 0.0), 0.5)[None, None]
        cfg = CC.ccfg(R, cm.CONTINUOUS, 1.0, 0, 1, 0.1, 1.0, 0.01)
        return [(CC.spherebot_desc(), scene, np.array([[x0, x1]]), cfg, [fx]) for x0, x1, fx, *_ in CC.SPHEREBOT_CASES]
    if kind.startswith("cont-C-"):
        _, _, etype, fixed = kind.split("-")
        d, scene, x, lvs = CC.config_c(0)
        scenes, xs = two_problems(scene, x)
        return [(d, scenes, xs, CC.ccfg(R, ETYPES[etype], lvs), SEG_FIXED[fixed])]
    if kind == "cont-274keys":
        d, scene, x, lvs = CC.config_c(9)
        return [(d, scene[None], x, CC.ccfg(3, cm.LVS_CONTINUOUS, lvs), None)]
    assert kind == "cont-tie", name
    d, scene = tie_desc(2)
    x = np.array([[[0.5, 0.0], [2.5, 0.0]]])
    return [(d, scene, x, CC.ccfg(2, cm.CONTINUOUS, 1.0, 0, 1, 0.1, 1.0, 0.05), None)]


CASES = (["disc-spherebot-R1", "disc-spherebot-R3", "disc-C-R3", "disc-C-R64", "disc-274keys", "disc-tie",
          "cont-spherebot-R1", "cont-spherebot-R3"] +
         [f"cont-C-{e}-{f}-R{R}" for e in ETYPES for f in SEG_FIXED for R in (3, 64)] +
         ["cont-274keys", "cont-tie"])


def case_runs(name):
    return disc_runs(name) if name.startswith("disc-") else cont_runs(name)


def run_case(name):
    """One case's results: {name/run/field: array}."""
    out = {}
    for i, (d, scene, x, cfg, *fixed) in enumerate(case_runs(name)):
        cs = ContinuousCollisionSets(d, len(x), scene, cfg, *fixed) if fixed else CollisionSets(d, len(x), scene, cfg)
        try:
            got = cs.run(x)
        finally:
            cs.close()
        out.update({f"{name}/{i}/{f}": a for f, a in zip(FIELDS, got)})
    return out


def pack(results):
    """The fixture's entries from the results of every case, in the order of CASES."""
    assert [k.split("/")[0] for k in results][::len(FIELDS)] == [n for n in CASES for _ in case_runs(n)]
    return {f: np.concatenate([a.ravel() for k, a in results.items() if k.endswith("/" + f)]) for f in FIELDS}


def unpack(packed):
    """pack()'s inverse; a run's shapes follow from its inputs: B problems, n nodes or
    segments, R rows, D joints."""
    out, at = {}, dict.fromkeys(FIELDS, 0)
    for name in CASES:
        for i, (d, scene, x, cfg, *fixed) in enumerate(case_runs(name)):
            n = cfg.last_step - cfg.first_step + (0 if fixed else 1)
            rows = (len(x), n, cfg.max_num_cnt)
            shapes = (rows, rows + ((2,) if fixed else ()) + (d.chain.n_dof,), rows, rows[:2], rows + (4,))
            for f, shape in zip(FIELDS, shapes):
                size = int(np.prod(shape))
                out[f"{name}/{i}/{f}"] = packed[f][at[f]:at[f] + size].reshape(shape)
                at[f] += size
    assert all(at[f] == packed[f].size for f in FIELDS), "the fixture's sizes differ from the cases'"
    return out


def check_case(name, got):
    """What makes the case worth recording: a case that misses it gets other inputs,
    never a weaker assertion."""
    counts, keys, values = (got[f"{name}/0/{f}"] for f in ("counts", "keys", "values"))
    print(name, "counts", [got[k].tolist() for k in got if k.endswith("/counts")])
    if name.endswith("-R3") and "-C" in name or "274keys" in name:
        assert counts.min() > 3, f"{name}: not more sets than rows ({counts.tolist()})"
    if name.endswith("-R64"):
        assert 0 < counts.min() and counts.max() < 64, f"{name}: not fewer sets than rows ({counts.tolist()})"
    if "274keys" in name:
        d = S.config_c(9)[0]
        assert d.n_spheres * d.n_prims + len(S.self_pairs(d)) > 256
    if name.endswith("-tie"):
        assert counts.tolist() == [[2]] and keys[0, 0].tolist() == [[3, 0, 1, -1], [3, 1, 0, -1]]
        assert values[0, 0, 0] == values[0, 0, 1]


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()  # raises if the HIP library is missing
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return unpack({k: z[k] for k in z.files})


@pytest.mark.parametrize("name", CASES)
def test_sets_reproduce_recorded_bits(golden, name):
    got = run_case(name)
    check_case(name, got)
    assert set(got) == {k for k in golden if k.startswith(name + "/")}, f"{name}: the fixture's entries differ"
    for k, v in got.items():
        g = golden[k]
        assert g.dtype == v.dtype and g.shape == v.shape and np.array_equal(g, v), \
            f"{k}: {int((g != v).sum()) if g.shape == v.shape else 'shape'} entries differ from the recorded bits"
