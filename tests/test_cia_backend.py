"""The CIA backend without a GPU: registry, config and file paths, the transcribed layout against
a hand-written NLP, the relaxed results file, and the golden file's own conditions.  The three
launches on the device: tests/test_gpu_cia_backend.py."""

import json
import pathlib

import numpy as np
import pytest
import torch

from agentlib_mpc_amd import benchmarks as bm
from agentlib_mpc_amd import symbolic as sx
from agentlib_mpc_amd.data_structures.mpc_datamodels import (
    MINLPVariableReference, VariableReference, cia_relaxed_results_path, stats_path,
)
from agentlib_mpc_amd.optimization_backends import backend_types, create_optimization_backend
from agentlib_mpc_amd.optimization_backends.cia import CIARoundingResults, MI355XCIABackend
from agentlib_mpc_amd.optimization_backends.problem import FleetResults
from agentlib_mpc_amd.runtime import native
from tests import cia_cases as cc

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "cia_room.json"

pytestmark = pytest.mark.filterwarnings("ignore:Model uses the deprecated objective formulation")


def test_registry_keys():
    for key in ("mi355x_cia", "casadi_cia"):
        assert backend_types[key].class_name == "MI355XCIABackend"
    assert "casadi_minlp" not in backend_types  # needs a mixed-integer solver: out of scope
    be = create_optimization_backend({
        "type": "casadi_cia", "model": {"type": "agentlib_mpc_amd.models.examples.CoolerRoom"},
        "discretization_options": {"collocation_order": 2, "collocation_method": "legendre"},
        "solver": {"name": "ipopt"}})
    assert isinstance(be, MI355XCIABackend)
    assert be.solver_options["max_iter"] == 100 and be.solver_options["tol"] == 1e-4  # the reference's defaults


def test_variable_reference_and_system():
    ref = MINLPVariableReference(states=["T"], controls=["cooling_power"], binary_controls=["cooler_on"])
    assert isinstance(ref, VariableReference) and "cooler_on" in ref and "cooler_on" in ref.all_variables()
    be, _ = bm.one_room_cia(N=3)
    groups = [v.name for v in be.system.variables]
    assert groups[0] == "w" and be.system.binary_controls.binary and not be.system.controls.binary
    assert be.system.binary_controls.ref_names == ("cooler_on",)


def test_relaxed_path_and_overwrite_check(tmp_path):
    res = tmp_path / "out" / "mpc.csv"
    relaxed = cia_relaxed_results_path(res)
    assert relaxed == tmp_path / "out" / "relaxed_mpc.csv"
    assert stats_path(relaxed) == tmp_path / "out" / "stats_relaxed_mpc.csv"
    res.parent.mkdir()
    files = (res, stats_path(res), relaxed, stats_path(relaxed))
    for f in files:
        f.write_text("old\n")
    cfg = {"type": "mi355x_cia", "model": {"type": "agentlib_mpc_amd.models.examples.CoolerRoom"},
           "discretization_options": {}, "results_file": str(res), "save_results": True}
    with pytest.raises(FileExistsError):
        create_optimization_backend(cfg)
    assert all(f.exists() for f in files)
    create_optimization_backend(dict(cfg, overwrite_result_file=True))
    assert not any(f.exists() for f in files)
    create_optimization_backend(dict(cfg, overwrite_result_file=True))  # nothing to remove is fine


@pytest.mark.parametrize("N", [4, 10])
def test_collocation_layout_matches_hand_written_nlp(N):
    """w, p and g of ``one_room_cia`` are the hand-written NLP's (tests/cia_cases.cooler_room): the
    same inputs, and the same functions and bounds at random points."""
    be, cv = bm.one_room_cia(N=N)
    nlp = be.problem.nlp
    prob = cc.cooler_room(N=N)
    assert (nlp.nw, nlp.ng_total, nlp.npar) == (prob.n, prob.m, prob.np_) and nlp.lift is None
    p, lbw, ubw, w0 = be.problem.marshal.inputs([cv], 0.0)
    for got, want in zip((p[0], lbw[0], ubw[0], w0[0]), cc.cooler_room_inputs(prob, N=N)):
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(be.binary_positions, cc.cooler_room_binary_positions(prob))
    np.testing.assert_array_equal(native.cia_slot_table(be.binary_positions, nlp.nw), be._slot)
    assert [nlp.w_labels[i][0] for i in be.binary_positions[0]] == ["w"] * N
    assert [nlp.w_labels[i - 1][0] for i in be.binary_positions[0]] == ["control"] * N  # w_k right after u_k
    rng = np.random.default_rng(20261021)
    for trial in range(3):
        w = w0[0] + rng.normal(size=nlp.nw) * np.maximum(1.0, np.abs(w0[0])) * 1e-2
        pp = p[0] * (1 + 0.1 * rng.normal(size=nlp.npar))
        vals = dict(zip(nlp.w_syms, w))
        vals.update(zip(nlp.p_syms, pp))
        vals.update({s: nlp.tk_values[k] for k, s in (nlp.tk_syms or {}).items()})
        f, *g = sx.evaluate([nlp.f_expr] + nlp.g_exprs, vals)
        np.testing.assert_allclose(float(f), float(prob.f(torch.as_tensor(w), torch.as_tensor(pp))), rtol=1e-12)
        np.testing.assert_allclose(np.array(g, float), prob.g(torch.as_tensor(w), torch.as_tensor(pp)).numpy(),
                                   rtol=1e-11, atol=1e-9)
        np.testing.assert_array_equal(np.array(sx.evaluate(nlp.g_lb, vals), float), prob.lbg(pp))
        np.testing.assert_array_equal(np.array(sx.evaluate(nlp.g_ub, vals), float), prob.ubg(pp))


def test_shooting_layout():
    """Multiple shooting: (u, w, z, y, x) per interval, the continuity row before the model's rows,
    the cost of an interval its stage cost times the time step."""
    be = create_optimization_backend({
        "type": "mi355x_cia", "model": {"type": "agentlib_mpc_amd.models.examples.CoolerRoom"},
        "discretization_options": {"method": "multiple_shooting", "integrator": "euler", "prediction_horizon": 3,
                                   "time_step": 300}})
    be.setup_optimization(MINLPVariableReference(
        states=["T"], controls=["cooling_power"], binary_controls=["cooler_on"],
        inputs=["load", "T_upper", "T_in"], parameters=["s_T", "r_cooling", "cooler_mod_limit"]))
    nlp = be.problem.nlp
    assert [lab[0] for lab in nlp.w_labels] == ["state"] + ["control", "w", "z", "y", "state"] * 3
    assert nlp.gap_closing == [True, False, False, False, False] * 3
    assert be.binary_positions.tolist() == [[2, 7, 12]]
    w = np.arange(1.0, nlp.nw + 1)
    p = np.array([290.0, 1000.0, 1e5, 3.0, 0.5, 250.0] + [150.0, 295.15, 290.15] * 3)
    vals = dict(zip(nlp.w_syms, w))
    vals.update(zip(nlp.p_syms, p))
    f, *g = sx.evaluate([nlp.f_expr] + nlp.g_exprs, vals)
    power, on, slack, T_out, T1 = w[1:6]
    np.testing.assert_allclose(np.array(g[:5], float),
                               [T1 - (w[0] + 300.0 * (150.0 - power) / 1e5), power - 1000.0 * on, power - 250.0 * on,
                                w[0] + slack, T_out - w[0]], rtol=1e-13)
    np.testing.assert_allclose(float(f), sum(300.0 * (0.5 * w[1 + 5 * k] + 3.0 * w[3 + 5 * k] ** 2) for k in range(3)),
                               rtol=1e-13)


def test_limits_are_checked_at_setup():
    with pytest.raises(ValueError, match="128"):
        bm.one_room_cia(N=129)


def _fake_results(be, cv, n=1, seed=0):
    """FleetResults of made-up solutions (no solve): what the writers get."""
    prob = be.problem
    p, lbw, ubw, w0, sampled = prob.marshal.inputs([cv] * n, 0.0, None, return_sampled_bounds=True)
    w = w0 + np.random.default_rng(seed).random(w0.shape)
    stats = native.StatsView(native.stats_array(np.zeros(n * native.STATS_BYTES, np.uint8)), {"t_wall_total": 0.5})
    return FleetResults(prob, prob.marshal, p, sampled[0], sampled[1], w, stats)


def test_relaxed_file_has_the_main_files_columns(tmp_path):
    res = tmp_path / "results" / "mpc.csv"
    be, cv = bm.one_room_cia(N=4, results_file=str(res), save_results=True, overwrite_result_file=True)
    for now in (0.0, 300.0):
        be.save_rel_result_df(_fake_results(be, cv, seed=1)[0], now)
        be.save_result_df(_fake_results(be, cv, seed=2)[0], now)
    relaxed = cia_relaxed_results_path(res)
    main_lines, rel_lines = res.read_text().splitlines(), relaxed.read_text().splitlines()
    assert main_lines[:2] == rel_lines[:2] and main_lines[0].startswith(",parameter")  # the two header lines
    assert len(main_lines) == len(rel_lines) == 2 + 2 * len(be.problem.layout.full_grid)
    assert [ln.split(",", 1)[0] for ln in main_lines[2:]] == [ln.split(",", 1)[0] for ln in rel_lines[2:]]
    # stats: the relaxed file has the solver's stats, the main file the objective terms before them
    rel_stats = stats_path(relaxed).read_text().splitlines()
    main_stats = stats_path(res).read_text().splitlines()
    assert len(rel_stats) == len(main_stats) == 3
    names = rel_stats[0].split(",")[1:]
    assert names[:3] == ["obj", "primal_inf", "dual_inf"] and "return_status" in names
    assert [n for n in main_stats[0].split(",")[1:] if n.startswith("stats_")] == [f"stats_{n}" for n in names]
    assert rel_stats[1].startswith('"0.0",') and rel_stats[2].startswith('"300.0",')


def test_solve_raises_on_a_rounding_failure(monkeypatch):
    be, cv = bm.one_room_cia(N=4)
    fake = _fake_results(be, cv)

    def solve_batch(now, batch_vars, agent_ids=None):
        be.last_relaxed = fake
        be.last_cia = CIARoundingResults(eta=np.array([np.nan]), b_bin=np.full((1, 1, 4), np.nan),
                                         status=np.array([status], np.int32))
        return fake
    monkeypatch.setattr(be, "solve_batch", solve_batch)
    status = native.CIA_BAD_INPUT
    with pytest.raises(ValueError, match="BAD_INPUT"):
        be.solve(0.0, cv)
    status = native.CIA_OK
    assert be.solve(0.0, cv).stats["t_wall_total"] == 0.5


def test_golden_cases_meet_their_conditions():
    """What tests/golden/make_cia_goldens.py promises about cia_room.json, and that the recorded
    rounding is what both restatements compute from the recorded relaxed controls."""
    cases = json.loads(GOLDEN.read_text())["cases"]
    assert len(cases) >= 2
    inner = 0
    for case in cases:
        assert len(case["calls"]) == 2
        for call in case["calls"]:
            assert call["relaxed"]["status"] == call["fixed"]["status"] == "Solve_Succeeded"
            assert call["eta_next_intervals"] - call["eta_intervals"] >= 1e-3
            b_rel = np.array(call["b_rel"])
            inner = max(inner, int(((b_rel > 0.05) & (b_rel < 0.95)).sum()))
            out = cc.round_batch(b_rel[None, None, :], case["time_step"])
            assert out["status"][0] == cc.OK and out["eta"][0] == call["eta"]
            np.testing.assert_array_equal(out["b_bin"][0, 0], call["b_bin"])
            b, _ = cc.modes(b_rel[None, None, :])
            eta, B = cc.dp_full(b[0])
            assert eta == call["eta_intervals"] and case["time_step"] * eta == call["eta"]
            np.testing.assert_array_equal(B[0], call["b_bin"])
            prob = cc.cooler_room(N=case["N"], ts=case["time_step"])
            pos = cc.cooler_room_binary_positions(prob)[0]
            np.testing.assert_array_equal(np.array(call["relaxed"]["x"])[pos], b_rel)
            np.testing.assert_array_equal(np.array(call["fixed"]["x"])[pos], call["b_bin"])
        # the second call starts from the first call's fixed optimum
        first, second = case["calls"]
        np.testing.assert_array_equal(second["w0"][1:], first["fixed"]["x"][1:])
        assert second["w0"][0] == second["T0"] != first["T0"]
    assert inner >= 2
