"""The trajectory checker's C-ABI (include/trajopt_hip.h thip_check_*) without a
GPU: struct layouts, the default config, and validation of the config and of
the descriptor fields it reads, each before any device call."""
import ctypes as C
import math

import pytest

from trajopt_amd import abi, problems


@pytest.fixture(scope="module")
def lib():
    if not abi.HIP_LIB.exists():
        import __graft_entry__

        __graft_entry__.build()
    return abi.load_hip()


def test_struct_sizes_match_the_mirrors(lib):
    assert lib.thip_sizeof_check_config() == C.sizeof(abi.CheckConfig)
    assert lib.thip_sizeof_check_result() == C.sizeof(abi.CheckResult)
    assert C.sizeof(abi.CheckResult) == 64


def test_default_config(lib):
    """planning_unit.cpp's check: a CONTINUOUS manager (LVS_CONTINUOUS with one cast
    per step pair), margin 0, the whole trajectory."""
    c = abi.CheckConfig(7, 1.0, 3.0, 5, 5)
    lib.thip_default_check_config(C.byref(c))
    assert c.type == abi.CHECK_LVS_CONTINUOUS
    assert c.lvs == math.inf
    assert c.margin == 0.0
    assert (c.first_step, c.last_step) == (0, -1)
    d = abi.default_check_config()
    for name, _ in abi.CheckConfig._fields_:
        assert getattr(c, name) == getattr(d, name), name
    lib.thip_default_check_config(None)


def _create(lib, desc, cfg, batch=2):
    chk = C.c_void_p()
    rc = lib.thip_check_create(0, C.byref(desc), C.byref(cfg), batch, C.byref(chk))
    return rc, chk


def _cfg(**kw):
    c = abi.default_check_config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize(
    "cfg, needle",
    [
        (dict(type=3), "type"),
        (dict(type=-1), "type"),
        (dict(type=0, lvs=0.0), "lvs"),
        (dict(type=1, lvs=-0.05), "lvs"),
        (dict(type=1, lvs=math.nan), "lvs"),
        (dict(margin=math.inf), "margin"),
        (dict(margin=math.nan), "margin"),
        (dict(first_step=4, last_step=2), "step range"),
        (dict(first_step=3, last_step=3), "step range"),  # a step-pair kind over one waypoint: no unit
        (dict(first_step=-2), "step range"),
        (dict(last_step=6), "step range"),
        (dict(type=2, first_step=6, last_step=-1), "step range"),
    ],
)
def test_create_rejects_invalid_configs(lib, cfg, needle):
    d = problems.make_workload("C", 1, n_steps=6).desc
    rc, chk = _create(lib, d, _cfg(**cfg))
    assert rc == -1  # THIP_E_INVALID
    assert not chk
    msg = lib.thip_check_last_error(None).decode()
    assert "thip_check_create" in msg and needle in msg, msg


@pytest.mark.parametrize(
    "mutate, needle",
    [
        (lambda d: setattr(d, "n_spheres", 0), "n_spheres"),
        (lambda d: setattr(d, "n_spheres", abi.MAX_SPHERES + 1), "n_spheres"),
        (lambda d: d.sphere_link.__setitem__(1, 0), "sphere link"),
        (lambda d: d.sphere_link.__setitem__(0, d.chain.n_links), "sphere link"),
        (lambda d: setattr(d, "n_prims", abi.EVAL_MAX_PRIMS + 1), "n_prims"),
        (lambda d: setattr(d, "n_steps", abi.EVAL_MAX_STEPS + 1), "n_steps"),
        (lambda d: setattr(d, "abi_version", abi.ABI_VERSION - 1), "abi_version"),
        (lambda d: (setattr(d, "n_self_pairs", 1), d.self_pair[0].__setitem__(0, 2), d.self_pair[0].__setitem__(1, 2)),
         "self-collision"),
    ],
)
def test_create_rejects_invalid_descriptors(lib, mutate, needle):
    d = problems.make_workload("C", 1, n_steps=6).desc
    mutate(d)
    rc, chk = _create(lib, d, abi.default_check_config())
    assert rc == -1
    assert not chk
    msg = lib.thip_check_last_error(None).decode()
    assert needle in msg, msg


def test_a_descriptor_without_a_collision_term_is_not_refused_for_it(lib):
    """Only the chain, spheres, self pairs, n_prims and n_steps are read: config A
    has no robot spheres, so the reason is the spheres, never the missing term."""
    d = problems.make_workload("A", 1).desc
    assert d.coll_enabled == 0
    rc, chk = _create(lib, d, abi.default_check_config())
    assert rc == -1 and "n_spheres" in lib.thip_check_last_error(None).decode()


def test_bad_arguments_and_null_checker_fail_cleanly(lib):
    d = problems.make_workload("C", 1, n_steps=6).desc
    cfg = abi.default_check_config()
    chk = C.c_void_p()
    assert lib.thip_check_create(0, C.byref(d), C.byref(cfg), 0, C.byref(chk)) == -1
    assert lib.thip_check_create(0, None, C.byref(cfg), 1, C.byref(chk)) == -1
    assert lib.thip_check_create(0, C.byref(d), None, 1, C.byref(chk)) == -1
    assert lib.thip_check_create(0, C.byref(d), C.byref(cfg), 1, None) == -1
    assert lib.thip_check_upload(None, None) == -1
    assert lib.thip_check_upload_device(None, None) == -1
    assert lib.thip_check_run(None, None, None, None) == -1
    assert lib.thip_check_run_device(None, None, None, None) == -1
    assert lib.thip_check_units(None) == -1
    assert lib.thip_check_last_ms(None) < 0
    lib.thip_check_destroy(None)
