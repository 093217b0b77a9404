"""The packed slack-side arrays of the interior-point kernel (csrc/mpcx_ipm.hip ``sidx_slot``).

``s``, ``sL``, ``sU``, ``vL``, ``vU`` and ``ds`` hold only the rows with a slack (lb != ub), each at
the number of such rows below it: a ballot per slot of 64 rows plus the earlier slots' counts.  What
can go wrong is the index at the slot boundaries, a set that is empty, one agent's index leaking
into another's, and a phase reading a packed entry that its own solve never wrote.  The parity
checks compare the way ``tests/test_gpu_ipm.py`` does: the oracle ``ipm.solve``, same status and
iteration count, RTOL_OBJ on the objective and RTOL_TRAJ on the solution, on every build that
exists for the structure.
"""

import numpy as np
import pytest
import torch

from tests import configs
from tests.test_gpu_ipm import (BUILDS, REFERENCE_OPTS, RTOL_OBJ, RTOL_TRAJ, _gpu_solve, _oracle, _w_of,
                                reset_builds, select_build)
from oracle import ipm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _settings(setting):
    from agentlib_mpc_amd import benchmarks as bm

    if setting == "tight":
        return bm.TIGHT, ipm.IPMOptions(tol=1e-10, max_iter=500, acceptable_iter=0)
    return bm.REFERENCE, ipm.IPMOptions(**REFERENCE_OPTS)


def _assert_matches_oracle(case, ref, res):
    for r in res:
        assert r.stats["return_status"] == ref.status, (r.stats, ref.status)
        assert r.stats["iter_count"] == ref.iterations, (r.stats["iter_count"], ref.iterations)
        np.testing.assert_allclose(r.stats["obj"], ref.f, rtol=RTOL_OBJ, atol=1e-9)
        np.testing.assert_allclose(_w_of(case, r), ref.x, rtol=RTOL_TRAJ, atol=1e-7 * max(1.0, np.abs(ref.x).max()))


def _row_bounds(case):
    p = case.oracle_inputs[0]
    return np.asarray(case.oracle.lbg(p), float), np.asarray(case.oracle.ubg(p), float)


#: one_room has 7 rows per stage, two of them inequalities (M = 7 N, 2 N packed entries).
#: N = 9: 63 rows, one slot with its last lane idle; N = 10: 70 rows, inequality rows on both sides of
#: lane 64, the second slot's base being the first slot's count; N = 19: 133 rows, three slots.
#: The oracle converges at all three, at both settings (checked before the sizes were fixed).
SLOT_HORIZONS = [9, 10, 19]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("setting", ["tight", "reference"])
@pytest.mark.parametrize("N", SLOT_HORIZONS)
def test_packed_index_at_slot_boundaries(N, setting, build):
    solver_options, opts = _settings(setting)
    case = configs.one_room(N=N, solver_options=solver_options)
    lb, ub = _row_bounds(case)
    assert len(lb) == 7 * N and int((lb != ub).sum()) == 2 * N  # the layout the horizons were chosen for
    if N == 10:
        assert (lb != ub)[:64].any() and (lb != ub)[64:].any()
    ref = _oracle(case, opts, key=("one_room_slots", N))
    assert ref.success, ref.status
    _assert_matches_oracle(case, ref, _gpu_solve(case, n_copies=3, build=build))


#: Structures all of whose rows are equalities (nothing packed: every lane's index is 0 and is
#: clamped into the array): tz_ahu over three slots (M = 144), exchange_supply inside one (M = 10).
#: No structure of tests/configs.py has 64 consecutive inequality rows (the longest run is 1), so a
#: slot without an equality row does not occur in the catalogue.
ALL_EQUALITY = ["tz_ahu", "exchange_supply"]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ALL_EQUALITY)
def test_structure_without_slack_rows(name, build):
    case = configs.CASES[name]()
    lb, ub = _row_bounds(case)
    assert np.array_equal(lb, ub)
    ref = _oracle(case, key=(name, "{}"))
    assert ref.success, ref.status
    _assert_matches_oracle(case, ref, _gpu_solve(case, n_copies=3, build=build))


def _launch(native, ng, arrays, rows=slice(None)):
    """One launch of the agents ``rows``: (w, lam_g, stats records) on the host."""
    from agentlib_mpc_amd.runtime.native import STATS_BYTES, stats_array

    p, lbw, ubw, w = (torch.as_tensor(np.ascontiguousarray(a[rows]), device="cuda") for a in arrays)
    n = p.shape[0]
    lam = torch.zeros((n, ng), dtype=torch.float64, device="cuda")
    st = torch.zeros(n * STATS_BYTES, dtype=torch.uint8, device="cuda")
    native.solve(p, lbw, ubw, w, lam_g=lam, stats=st)
    torch.cuda.synchronize()
    return w.cpu().numpy(), lam.cpu().numpy(), stats_array(st.cpu().numpy()).copy()


@pytest.mark.parametrize("build", BUILDS)
def test_fleet_of_distinct_agents_equals_one_agent_per_launch(build):
    """64 one_room agents with seeded distinct parameters (``bench.fleet_values``) in one launch and
    the same agents one per launch, on the same code object: equal array for array.  On every build:
    how many agents share a CU (and so run beside a neighbour with another packed index) differs
    between them."""
    import bench
    from agentlib_mpc_amd import benchmarks as bm
    from agentlib_mpc_amd.optimization_backends.problem import fleet_nlp_inputs

    n = 64
    be, cv = bm.one_room(solver_options=bm.REFERENCE)
    arrays = be.problem.to_kernel(*fleet_nlp_inputs(be.problem, cv, bench.fleet_values(n, 20261019)))
    native = be._native()
    native.reserve(n)
    select_build(native, build)
    try:
        w, lam, st = _launch(native, be.problem.nlp.ng_total, arrays)
        singles = [_launch(native, be.problem.nlp.ng_total, arrays, slice(i, i + 1)) for i in range(n)]
    finally:
        reset_builds(native)
    assert (st["status"] <= 1).all(), st["status"]
    assert len({int(x) for x in st["iter_count"]}) > 1  # distinct agents: not one path taken 64 times
    assert np.array_equal(w, np.concatenate([s[0] for s in singles]))
    assert np.array_equal(lam, np.concatenate([s[1] for s in singles]))
    assert np.array_equal(st, np.concatenate([s[2] for s in singles]))


#: one_room started below the supply temperature (T0 = 285 K < T_in): its temperature rows cannot be
#: met, the filter line search fails and the restoration phase runs (the oracle at the reference
#: settings: 44 iterations, 10 phases with 24 restoration iterations, Infeasible_Problem_Detected)
#: -- with the structure's 30 slack rows in every restoration phase.  No other catalogue case with
#: slack rows enters the restoration phase (RESTO_CASES and LONG_RESTO_CASES have equality rows only).
RESTO_T0 = 285.0
#: The parity check runs the first 12 iterations of it, which hold 3 restoration phases (start,
#: restoration iterations with their refinement, return, three times over): the oracle takes 6 s for
#: them and 23 s for the whole run, and it runs once for all builds.
RESTO_PREFIX = 12


@pytest.mark.parametrize("build", BUILDS)
def test_restoration_phase_with_slack_rows_matches_oracle(build):
    """The way RESTO_CASES are compared: same status, iteration count, soft steps, restoration phases
    and restoration iterations as the oracle, at the same objective and point."""
    opts = dict(REFERENCE_OPTS, max_iter=RESTO_PREFIX)
    case = configs.one_room(T0=RESTO_T0, solver_options={"ipopt": dict(opts)})
    lb, ub = _row_bounds(case)
    assert int((lb != ub).sum()) == 30
    ref = _oracle(case, ipm.IPMOptions(**opts), key=("one_room_resto", RESTO_T0))
    assert ref.n_resto == 3 and ref.resto_iterations > 0, (ref.n_resto, ref.resto_iterations)
    for r in _gpu_solve(case, n_copies=2, build=build):
        st = r.stats
        got = (st["return_status"], st["iter_count"], st["n_soft_restorations"], st["n_restorations"],
               st["n_restoration_iters"])
        print(build, got, st["obj"], (ref.status, ref.iterations, ref.n_soft_resto, ref.n_resto, ref.resto_iterations), ref.f)
        assert got == (ref.status, ref.iterations, ref.n_soft_resto, ref.n_resto, ref.resto_iterations), got
        np.testing.assert_allclose(st["obj"], ref.f, rtol=RTOL_OBJ, atol=1e-9)
        np.testing.assert_allclose(_w_of(case, r), ref.x, rtol=RTOL_TRAJ, atol=1e-7 * max(1.0, np.abs(ref.x).max()))


def _fleets(which):
    """(backend, fleet A, fleet B, what A's statistics must show) on one backend."""
    from agentlib_mpc_amd import benchmarks as bm
    from agentlib_mpc_amd.optimization_backends.problem import fleet_nlp_inputs

    n = 4
    if which == "restoration_between":
        # A: regular solves; B: the restoration fleet above, whose phases write every packed array of
        # the slab, backups included
        be, cv = bm.one_room(solver_options=bm.REFERENCE)
        inputs = lambda c, vals: be.problem.to_kernel(*fleet_nlp_inputs(be.problem, c, vals))  # noqa: E731
        a = inputs(cv, {"T": np.linspace(292.0, 300.0, n), "load": np.linspace(80.0, 220.0, n)})
        b = inputs(cv, {"T": np.full(n, RESTO_T0)})
        check = lambda sa, sb: ((sa["status"] <= 1).all() and (sa["n_restorations"] == 0).all()  # noqa: E731
                                and (sb["n_restorations"] > 0).all())
        return be, a, b, check
    # A: the fixture_mpc case of RESTO_CASES (M = 35, NW = 41; the oracle: 2 soft restoration steps, 10
    # restoration phases): the soft step is the one reader of the resident Newton step outside the
    # regular phases (soft_apply; the step is resident on every build of this structure); B: the
    # same structure's regular fleet
    be, cv = bm.fixture_mpc(solver_options=bm.REFERENCE)
    _, cv_soft = bm.fixture_mpc(solver_options=bm.REFERENCE, T_lb=245.0, T_ub=302.0, disturbance=260.0)
    inputs = lambda c, vals: be.problem.to_kernel(*fleet_nlp_inputs(be.problem, c, vals))  # noqa: E731
    a = inputs(cv_soft, {"state": np.full(n, 298.16)})
    b = inputs(cv, {"state": np.linspace(290.0, 300.0, n)})
    check = lambda sa, sb: ((sa["n_soft_restorations"] > 0).all() and (sa["n_restorations"] > 0).all()  # noqa: E731
                            and (sb["status"] <= 1).all())
    return be, a, b, check


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("which", ["restoration_between", "soft_restoration_first"])
def test_result_does_not_depend_on_what_the_workspace_held(which, build):
    """One backend, so one workspace slab: fleet A, then fleet B, then A again.  Both A results --
    ``w``, ``lam_g`` and the statistics -- are equal bit for bit."""
    be, a, b, check = _fleets(which)
    native = be._native()
    native.reserve(4)
    ng = be.problem.nlp.ng_total
    select_build(native, build)
    try:
        first = _launch(native, ng, a)
        mid = _launch(native, ng, b)
        second = _launch(native, ng, a)
    finally:
        reset_builds(native)
    assert check(first[2], mid[2]), (first[2], mid[2])
    for x, y in zip(first, second):
        assert np.array_equal(x, y)
