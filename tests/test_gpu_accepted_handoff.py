"""The hand-off from the accepted step to the derivative passes and the factorisation
(csrc/mpcx_ipm.hip) against the path it replaces.

Four parts move data only: the constraint scaling read from LDS (A), the accepted multipliers
handed to the stage lanes through LDS (B), the next iterate's Hessian evaluated in the
accepted-point pass (C), and the Newton assembly taking 0.0 for image entries no evaluator writes
(D).  Each has a compile-time switch that restores the previous path (``bm.HANDOFF_SWITCHES``).
Every case below solves the same agents on the shipped main build and on the main build with the
switches set, and compares ``w``, ``lam_g`` and the raw statistics records byte for byte: the
arithmetic is meant to be the same operations on the same values, so nothing weaker than equality
applies.  The builds are compiled by ``benchmarks.compile_all`` (``bm.HANDOFF_TEST_BUILDS``).
"""

import pytest
import torch

from agentlib_mpc_amd import benchmarks as bm
from agentlib_mpc_amd.runtime import native
from tests import configs
from tests.test_gpu_row_compaction import _fleets, _launch

pytestmark = pytest.mark.gpu

N_COPIES = 3


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _case_arrays(case, n=N_COPIES):
    """(backend, kernel-layout inputs of ``n`` copies of the case)."""
    prob = case.backend.problem
    return case.backend, prob.to_kernel(*prob.marshal.inputs([case.current_vars] * n, 0.0))


def _resto_fleet(which):
    """The restoration fleets of tests/test_gpu_row_compaction.py at the reference settings: one_room
    started at T0 = 285 K (restoration phases) and the fixture_mpc soft-restoration case."""
    be, a, b, _ = _fleets(which)
    return be, (b if which == "restoration_between" else a)


#: name -> (builder of (backend, arrays), structure key of bm.HANDOFF_TEST_BUILDS, what the statistics
#: of every agent must show so that the case covers what it is here for)
CASES = {
    # the hand-off crosses one stage boundary
    "one_room_n2": (lambda: _case_arrays(configs.one_room(N=2)), "one_room_n2", None),
    # M = 70: rows (and parked multipliers) on both sides of lane 64
    "one_room_n10": (lambda: _case_arrays(configs.one_room(N=10)), "one_room_n10", None),
    # a stage-0 plan and a second elimination body
    "mhe_room": (lambda: _case_arrays(configs.mhe_room()), "mhe_room", None),
    # a NARX zone: the Jacobian and the Hessian network passes share the network's output buffer
    "room_nn_n8": (lambda: _case_arrays(configs.room_nn(N=8)), "room_nn_n8", None),
    # restoration phases / a soft restoration step: iterates the accepted-point pass never saw
    "one_room_resto": (lambda: _resto_fleet("restoration_between"), "one_room",
                       lambda st: (st["n_restorations"] > 0).all() and (st["n_restoration_iters"] > 0).all()),
    "fixture_mpc_soft": (lambda: _resto_fleet("soft_restoration_first"), "fixture_mpc",
                         lambda st: (st["n_soft_restorations"] > 0).all() and (st["n_restorations"] > 0).all()),
    # inertia corrections: the re-factorisation assembles from the image again
    "one_room_switch": (lambda: _case_arrays(configs.one_room_switch()), "one_room_switch",
                        lambda st: (st["n_inertia_corrections"] > 0).all()),
    # one_room at N = 19: the scaling copy would cost a static round, so this build reads the workspace
    "one_room_n19": (lambda: _case_arrays(configs.one_room(N=19)), "one_room_n19", None),
}


def _run(make, defines, monkeypatch):
    """One launch on the main build compiled with ``defines`` (no optional builds attached)."""
    for v in native.VARIANTS:
        monkeypatch.setenv(v.env, "0")
    if defines:
        monkeypatch.setenv("MPCX_DEFINES", defines)
    else:
        monkeypatch.delenv("MPCX_DEFINES", raising=False)
    be, arrays = make()
    nat = be._native()
    nat.reserve(arrays[0].shape[0])
    return _launch(nat, be.problem.nlp.kernel_ng, arrays)


def _assert_identical(got, want, what):
    for name, x, y in zip(("w", "lam_g", "stats"), got, want):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, name, x, y)


@pytest.mark.parametrize("name", sorted(CASES))
def test_shipped_build_equals_all_switches_off(name, monkeypatch):
    make, structure, shows = CASES[name]
    assert bm.HANDOFF_ALL_OFF in bm.HANDOFF_TEST_BUILDS[structure]
    new = _run(make, None, monkeypatch)
    old = _run(make, bm.HANDOFF_ALL_OFF, monkeypatch)
    st = new[2]
    print(name, list(st["status"]), list(st["iter_count"]), list(st["n_inertia_corrections"]),
          list(st["n_restorations"]), list(st["n_soft_restorations"]))
    assert shows is None or shows(st), st
    if name != "one_room_resto":  # (that one ends as Infeasible_Problem_Detected, like the oracle)
        assert (st["status"] <= 1).all(), st["status"]
    assert (st["iter_count"] >= 2).all()  # the accepted-point pass ran
    _assert_identical(new, old, name)


@pytest.mark.parametrize("switch", bm.HANDOFF_SWITCHES)
def test_each_switch_alone_on_one_room(switch, monkeypatch):
    make = lambda: _case_arrays(configs.one_room())  # noqa: E731
    assert switch in bm.HANDOFF_TEST_BUILDS["one_room"]
    new = _run(make, None, monkeypatch)
    assert (new[2]["status"] <= 1).all()
    _assert_identical(new, _run(make, switch, monkeypatch), switch)


def test_dense_assembly_uses_the_mask(monkeypatch):
    """MPCX_NO_STATIC: every stage through ``local_assemble<G, true>`` and the dense Bunch-Kaufman."""
    make = lambda: _case_arrays(configs.one_room())  # noqa: E731
    new = _run(make, "MPCX_NO_STATIC", monkeypatch)
    assert (new[2]["n_dense_stages"] > 0).all() and (new[2]["status"] <= 1).all(), new[2]
    _assert_identical(new, _run(make, "MPCX_NO_STATIC," + bm.HANDOFF_ALL_OFF, monkeypatch), "MPCX_NO_STATIC")


def test_scaling_switch_where_the_copy_does_not_fit(monkeypatch):
    """one_room at N = 19 has no LDS copy of the scaling on its main build: the
    switch of part A changes nothing there, and the other three parts run without it."""
    make = lambda: _case_arrays(configs.one_room(N=19))  # noqa: E731
    a = _run(make, None, monkeypatch)
    b = _run(make, "MPCX_GS_HBM", monkeypatch)
    assert a[0].shape[1] == 1 + 19 * 8
    _assert_identical(a, b, "MPCX_GS_HBM at N = 19")


def test_small_fleet_build_equals_all_switches_off(monkeypatch):
    """The workspace-in-LDS build of one_room (the 256-agent leg): parts B and D act there, A and C do
    not.  Its shipped form against the same build with every switch set."""
    def run(defines):
        for v in native.VARIANTS:
            if v.key != native.SMALL_FLEET:
                monkeypatch.setenv(v.env, "0")
        monkeypatch.delenv(native._BY_KEY[native.SMALL_FLEET].env, raising=False)
        if defines:
            monkeypatch.setenv("MPCX_DEFINES", defines)
        else:
            monkeypatch.delenv("MPCX_DEFINES", raising=False)
        be, arrays = _case_arrays(configs.one_room())
        nat = be._native()
        nat.reserve(arrays[0].shape[0])
        assert nat.small_fleet_path is not None
        nat.select_build("lds")
        try:
            return _launch(nat, be.problem.nlp.kernel_ng, arrays)
        finally:
            nat.select_build(None)

    assert bm.HANDOFF_ALL_OFF in bm.HANDOFF_TEST_BUILDS_LDS["one_room"]
    new = run(None)
    assert (new[2]["status"] <= 1).all() and (new[2]["iter_count"] >= 2).all(), new[2]
    _assert_identical(new, run(bm.HANDOFF_ALL_OFF), "small-fleet build")
