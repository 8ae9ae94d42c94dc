"""The term-value evaluator's C-ABI (include/trajopt_hip.h thip_terms_*) without a
GPU: the slot struct's layout, and refusal -- before any device call, with a
message naming the host loop -- of every descriptor thip_create refuses."""
import ctypes as C

import pytest

from trajopt_amd import abi, problems


@pytest.fixture(scope="module")
def lib():
    if not abi.HIP_LIB.exists():
        import __graft_entry__

        __graft_entry__.build()
    return abi.load_hip()


def _create(lib, desc, batch=3):
    t = C.c_void_p()
    rc = lib.thip_terms_create(0, C.byref(desc), batch, C.byref(t))
    return rc, t


def test_slot_struct_size_matches_the_mirror(lib):
    assert lib.thip_sizeof_term_slot() == C.sizeof(abi.TermSlot) == 16


def test_header_symbols_are_exported_and_declared(lib):
    names = [n for n in abi.exported_symbols() if n.startswith("thip_terms_") or n == "thip_sizeof_term_slot"]
    assert len(names) == 14, names
    for n in names:
        assert getattr(lib, n).argtypes is not None, n  # declared in abi._declare, exported by the library


def test_slot_table_without_an_evaluator(lib):
    """Config C at 6 waypoints: JointVel, 5 CartPose costs, 5 collision step pairs."""
    d = problems.make_workload("C", 1, n_steps=6).desc
    nc, nv = C.c_int(), C.c_int()
    tab = (abi.TermSlot * 64)()
    assert lib.thip_terms_slot_table(C.byref(d), tab, 64, C.byref(nc), C.byref(nv)) == 0
    assert (nc.value, nv.value) == (11, 0)
    assert [(s.kind, s.index, s.unit) for s in tab[:11]] == (
        [(abi.TERM_JOINT_VEL, 0, -1)] + [(abi.TERM_CART, k, -1) for k in range(5)]
        + [(abi.TERM_COLL, u, u) for u in range(5)])
    d.coll_is_cnt = 1
    assert lib.thip_terms_slot_table(C.byref(d), None, 0, C.byref(nc), C.byref(nv)) == 0
    assert (nc.value, nv.value) == (6, 5)


def _coll_extra(d):
    d.n_coll_extra = 1


def _non_fused_jdt(d):
    # a JointAccEqCost on an odd number of waypoints is not fused (thip_jdt_fused)
    d.n_steps = 7
    d.n_jdt = 1
    d.jdt_order[0] = 2
    d.jdt_first_step[0], d.jdt_last_step[0] = 0, 6


def _joint_acc(first, last):
    # a JointAccEqCost of the fused form (6 waypoints, 7 dofs) on steps first..last as given
    def mutate(d):
        d.n_jdt = 1
        d.jdt_order[0] = 2
        d.jdt_first_step[0], d.jdt_last_step[0] = first, last

    return mutate


@pytest.mark.parametrize(
    "config, mutate, needle, host_loop",
    [
        ("A", _joint_acc(0, 6), "jdt_last_step", False),    # last = n_steps
        ("A", _joint_acc(-1, 5), "jdt_first_step", False),  # first = -1
        ("A", _joint_acc(2, 3), "jdt_first_step + 2 <= jdt_last_step", False),  # last = first + 1
        ("A", lambda d: setattr(d, "abi_version", abi.ABI_VERSION + 1), "abi_version", False),
        ("C", _coll_extra, "coll_extra", True),
        ("A", lambda d: setattr(d, "use_time", 1), "use_time", True),
        ("A", _non_fused_jdt, "jdt", True),
        ("A", lambda d: setattr(d, "n_steps", abi.MAX_STEPS + 1), "n_steps", True),
        ("C", lambda d: setattr(d, "n_prims", abi.MAX_PRIMS + 1), "n_prims", True),
        ("C", lambda d: setattr(d, "coll_contact_test", 3), "coll_contact_test", False),
        ("A", lambda d: d.cart_source_link.__setitem__(0, 0), "CartPose source", False),
        ("A", lambda d: setattr(d.sqp, "trust_shrink_ratio", 1.5), "trust_shrink_ratio", False),
        ("A", lambda d: setattr(d.sqp, "max_time", -1.0), "max_time", False),
        ("A", lambda d: setattr(d.osqp, "max_iter", 0), "OSQP", False),
        ("C", lambda d: setattr(d, "coll_buffer", -0.01), "buffer", False),
        ("C", lambda d: (setattr(d, "n_self_pairs", 1), d.self_pair[0].__setitem__(0, 2), d.self_pair[0].__setitem__(1, 2)),
         "self-collision", False),
        ("C", lambda d: setattr(d, "n_fixed", abi.MAX_STEPS + 1), "n_fixed", False),
    ],
)
def test_create_refuses_what_the_fused_kernel_does_not_lower(lib, config, mutate, needle, host_loop):
    d = problems.make_workload(config, 1, n_steps=6).desc
    mutate(d)
    ctx = C.c_void_p()
    # thip_create refuses the same descriptor (validation precedes its device calls)
    assert lib.thip_create(0, C.byref(d), 3, C.byref(ctx)) == -1
    rc, t = _create(lib, d)
    assert rc == -1 and not t
    msg = lib.thip_terms_last_error(None).decode()
    assert "thip_terms_create" in msg and needle in msg, msg
    if host_loop:
        assert "host loop" in msg, msg


@pytest.mark.parametrize("batch", [0, -2])
def test_create_refuses_an_empty_batch(lib, batch):
    d = problems.make_workload("A", 1, n_steps=6).desc
    rc, t = _create(lib, d, batch=batch)
    assert rc == -1 and not t
    assert "batch" in lib.thip_terms_last_error(None).decode()


def test_bad_arguments_and_null_evaluator_fail_cleanly(lib):
    d = problems.make_workload("A", 1, n_steps=6).desc
    t = C.c_void_p()
    assert lib.thip_terms_create(0, None, 1, C.byref(t)) == -1
    assert lib.thip_terms_create(0, C.byref(d), 1, None) == -1
    assert lib.thip_terms_counts(None, None, None) == -1
    assert lib.thip_terms_slots(None, None) == -1
    assert lib.thip_terms_upload(None, None, None) == -1
    assert lib.thip_terms_upload_device(None, None, None) == -1
    assert lib.thip_terms_upload_joint_targets(None, None) == -1
    assert lib.thip_terms_upload_joint_targets_device(None, None) == -1
    assert lib.thip_terms_run(None, None, None, None) == -1
    assert lib.thip_terms_run_device(None, None, None, None) == -1
    assert lib.thip_terms_last_ms(None) < 0
    lib.thip_terms_destroy(None)
