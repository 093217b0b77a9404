"""The CIA backend on the device: relaxed solve, rounding kernel and fixed solve of the cooler room
against tests/golden/cia_room.json (the oracle IPM on a hand-written NLP plus the numpy rounding,
tests/golden/make_cia_goldens.py), on every build of the structure.

The fixed solve is also the first parity case with a fixed stage input (lb = ub on an entry of V).
Tolerances: those of tests/test_gpu_ipm.py (same status and iteration count, RTOL_OBJ on the
objective, RTOL_TRAJ on the solution); eta within N * 1e-5 * dt, which is what a 1e-5 error of each
relaxed control can add to a running sum; B equal (the golden cases keep the next-best eta at least
1e-3 intervals away)."""

import json
import pathlib

import numpy as np
import pytest
import torch

from agentlib_mpc_amd import benchmarks as bm
from agentlib_mpc_amd.data_structures.mpc_datamodels import cia_relaxed_results_path, stats_path
from agentlib_mpc_amd.optimization_backends import create_optimization_backend
from agentlib_mpc_amd.runtime import native as nat
from tests.test_gpu_ipm import BUILDS, RTOL_OBJ, RTOL_TRAJ, reset_builds, select_build

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Model uses the deprecated objective formulation")]

CASES = json.loads((pathlib.Path(__file__).resolve().parent / "golden" / "cia_room.json").read_text())["cases"]


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _assert_solve(fleet, want, what):
    x = np.array(want["x"])
    for i in range(len(fleet)):
        st = fleet.stats[i]
        print(what, i, st["return_status"], st["iter_count"], st["obj"], "golden", want["status"], want["iterations"],
              want["f"], "max |dx|", float(np.abs(fleet.w[i] - x).max()))
        assert st["return_status"] == want["status"], (what, st, want["status"])
        assert st["iter_count"] == want["iterations"], (what, st["iter_count"], want["iterations"])
        np.testing.assert_allclose(st["obj"], want["f"], rtol=RTOL_OBJ, atol=1e-9, err_msg=what)
        np.testing.assert_allclose(fleet.w[i], x, rtol=RTOL_TRAJ, atol=1e-7 * max(1.0, np.abs(x).max()), err_msg=what)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cooler_room_matches_golden(case, build):
    """Two calls of two identical agents: the first cold, the second warm-started from the first
    call's fixed optimum with a new measured temperature (the golden's second call starts from the
    oracle's fixed optimum)."""
    be, cv = bm.one_room_cia(N=case["N"], solver_options={"ipopt": dict(case["options"])}, **case["values"])
    native = be._native()
    select_build(native, build)
    try:
        for c, call in enumerate(case["calls"]):
            cv["T"] = bm.V("T", call["T0"], 288.15, 303.15)
            res = be.solve_batch(300.0 * c, [cv, cv])
            _assert_solve(be.last_relaxed, call["relaxed"], f"call {c} relaxed")
            cia = be.last_cia
            print("eta", cia.eta, "golden", call["eta"], "b_bin", cia.b_bin[0, 0])
            assert (cia.status == nat.CIA_OK).all() and cia.ok.all()
            np.testing.assert_array_equal(cia.b_bin, np.broadcast_to(np.array(call["b_bin"]), cia.b_bin.shape))
            assert (np.abs(cia.eta - call["eta"]) <= case["N"] * 1e-5 * case["time_step"]).all()
            _assert_solve(res, call["fixed"], f"call {c} fixed")
            np.testing.assert_array_equal(res.w[:, be.binary_positions[0]], cia.b_bin[:, 0])
            np.testing.assert_array_equal(res.w[0], res.w[1])
    finally:
        reset_builds(native)


def test_fleet_in_one_batch_equals_one_agent_per_call():
    """64 rooms with measured temperatures from 294 K (never cools) to 299 K in one ``solve_batch``
    against 64 calls of one agent each, on one build: the same bits in both solves' solutions and
    stats and in the rounding -- an agent's result does not depend on its neighbours or its slot."""
    n = 64
    temps = np.linspace(294.0, 299.0, n)
    be, cv = bm.one_room_cia(N=10)
    native = be._native()
    select_build(native, "main")
    try:
        batch = [dict(cv, T=bm.V("T", float(t), 288.15, 303.15)) for t in temps]
        res = be.solve_batch(0.0, batch)
        rel, cia = be.last_relaxed, be.last_cia
        assert len({tuple(b) for b in cia.b_bin[:, 0]}) >= 3  # the spread does spread the switching patterns
        print("status", np.bincount(cia.status), "patterns", sorted({tuple(b) for b in cia.b_bin[cia.ok, 0]}))
        for i in range(n):
            be.reset_warm_start()
            one = be.solve_batch(0.0, [batch[i]])
            np.testing.assert_array_equal(one.w[0], res.w[i])
            np.testing.assert_array_equal(be.last_relaxed.w[0], rel.w[i])
            assert one.stats.array[0] == res.stats.array[i] and be.last_relaxed.stats.array[0] == rel.stats.array[i]
            assert be.last_cia.status[0] == cia.status[i]
            np.testing.assert_array_equal(be.last_cia.eta[0], cia.eta[i])
            np.testing.assert_array_equal(be.last_cia.b_bin[0], cia.b_bin[i])
    finally:
        reset_builds(native)


def test_example_config_solves_and_writes_both_files(tmp_path):
    """The reference example's backend config with ``"type": "casadi_cia"``: ``solve`` returns the
    fixed solve's results, whose bounds of the binary control are its rounded values, and both
    results files get their rows."""
    res_file = tmp_path / "results" / "mpc.csv"
    be = create_optimization_backend({
        "type": "casadi_cia",
        "model": {"type": "agentlib_mpc_amd.models.examples.CoolerRoom"},
        "discretization_options": {"collocation_order": 2, "collocation_method": "legendre",
                                   "prediction_horizon": 10, "time_step": 300},
        "solver": {"name": "ipopt"},
        "overwrite_result_file": True, "results_file": str(res_file), "save_results": True})
    _, cv = bm.one_room_cia(N=10)
    from agentlib_mpc_amd.data_structures.mpc_datamodels import MINLPVariableReference

    be.setup_optimization(MINLPVariableReference(
        states=["T"], controls=["cooling_power"], binary_controls=["cooler_on"],
        inputs=["load", "T_upper", "T_in"], parameters=["s_T", "r_cooling", "cooler_mod_limit"], outputs=[]))
    results = be.solve(0.0, cv)
    assert results.stats["success"] and be.last_relaxed[0].stats["success"]
    on = results["cooler_on"].ravel()
    assert on.shape == (10,) and set(on) <= {0.0, 1.0} and on[0] == 1.0  # 3 K above the bound: it cools
    df = results.df
    np.testing.assert_array_equal(df[("lower", "cooler_on")].dropna().to_numpy(), on)
    np.testing.assert_array_equal(df[("upper", "cooler_on")].dropna().to_numpy(), on)
    power = results["cooling_power"].ravel()
    assert (power[on == 0.0] <= 1e-6).all() and (power[on == 1.0] >= 250.0 - 1e-6).all()
    relaxed = be.last_relaxed[0]["cooler_on"].ravel()
    assert ((relaxed > 0.05) & (relaxed < 0.95)).any()  # the relaxed solve did leave something to round
    assert np.isfinite(be.last_cia.eta[0]) and 0.0 < be.last_cia.eta[0] < 300.0
    relaxed_file = cia_relaxed_results_path(res_file)
    rows = len(be.problem.layout.full_grid)
    for f in (res_file, relaxed_file):
        assert len(f.read_text().splitlines()) == 2 + rows
    assert len(stats_path(res_file).read_text().splitlines()) == 2
    assert len(stats_path(relaxed_file).read_text().splitlines()) == 2
