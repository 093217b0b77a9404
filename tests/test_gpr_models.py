"""GPR and linear-regression NARX models (CPU): the reference's serialized layout, the numeric
twin against recorded scikit-learn predictions, the tracer's derivative nodes, the generated
code and its host build against the oracle IPM.

Reference: ``CasadiGPR`` / ``CasadiLinReg`` (`agentlib_mpc/models/casadi_predictor.py:87-190`)
over ``SerializedGPR`` / ``SerializedLinReg`` (`models/serialized_ml_model.py:410-660`).
tests/golden/gpr_golden.json holds three models fitted by scikit-learn and ``predict`` of the
fitted estimators (scripts/make_gpr_golden.py); scikit-learn is not imported here.

The oracle converges on the three rooms of tests/gpr_cases.py (N = 8, seed 11) at tol 1e-10 in
7 / 8 / 7 iterations (gpr20_gpr20, gpr33_ann, gpr17_linreg).
"""

import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from agentlib_mpc_amd import symbolic as sx
from agentlib_mpc_amd.models import examples as ex
from agentlib_mpc_amd.models.casadi_predictor import CasadiGPR, CasadiLinReg, CasadiPredictor
from agentlib_mpc_amd.models.serialized_ml_model import SerializedGPR, SerializedLinReg, SerializedMLModel
from agentlib_mpc_amd.runtime import codegen
from oracle import cbuild, ipm
from tests import gpr_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)

with open(os.path.join(ROOT, "tests", "golden", "gpr_golden.json")) as _f:
    GOLDEN = json.load(_f)

#: scaled deviation |predict_numpy - sklearn| / sum_j |w_j| measured for the numpy twin
#: (``test_gpr_twin_matches_scikit_learn`` prints it): the bound is 8 x this, at least 16 eps
TWIN_DEVIATION = {"gpr_scalar": 1.4e-15, "gpr_ard": 2.2e-15}


def _bound(name):
    return max(8.0 * TWIN_DEVIATION[name], 16.0 * EPS)


def _terms(model: SerializedGPR, x):
    """z - T_j [n, NT, n_in], |w_j| [n, NT], s [n_in], z [n, n_in], T: from the JSON fields, direct form."""
    gp, kp, dh = model.gpr_parameters, model.kernel_parameters, model.data_handling
    X = np.asarray(gp.X_train, float)
    ls = np.broadcast_to(np.asarray(kp.length_scale, float), (X.shape[1],))
    z = (np.atleast_2d(x) - np.asarray(dh.mean)) / np.asarray(dh.std) / ls
    T = X / ls
    d = z[:, None, :] - T[None]
    aw = np.abs(dh.scale * kp.constant_value * np.asarray(gp.alpha, float).reshape(-1)) * np.exp(-0.5 * (d * d).sum(axis=2))
    return d, aw, 1.0 / (np.asarray(dh.std) * ls), z, T


@pytest.mark.parametrize("name", ["gpr_scalar", "gpr_ard"])
def test_gpr_twin_matches_scikit_learn(name):
    """Golden (a) and (b) load from the reference's layout and ``predict_numpy`` reproduces the
    recorded ``predict`` of scikit-learn.  Unit: the deviation over ``sum_j |w_j|`` (alpha has
    both signs and entries far above |y|).  Measured for the twin: 1.4e-15 (scalar length scale,
    NT = 33, 5 features) and 2.2e-15 (per-feature, NT = 20, 3 features), the expanded distance
    of the twin against the pairwise differences of scikit-learn; bound 8 x that, at least
    16 eps."""
    model = SerializedMLModel.load_serialized_model(GOLDEN[name]["model"])
    assert isinstance(model, SerializedGPR)
    again = SerializedMLModel.load_serialized_model_from_string(model.model_dump_json())
    pred = CasadiPredictor.from_serialized_model(model)
    assert isinstance(pred, CasadiGPR)
    x, y = np.asarray(GOLDEN[name]["x"]), np.asarray(GOLDEN[name]["y"])
    got = pred.predict_numpy(x)
    assert got.shape == (len(x), 1)
    np.testing.assert_array_equal(CasadiGPR(again).predict_numpy(x), got)
    dev = float((np.abs(got[:, 0] - y) / _terms(model, x)[1].sum(axis=1)).max())
    print(f"{name}: scaled deviation {dev:.3g}, recorded {TWIN_DEVIATION[name]:.3g}, bound {_bound(name):.3g}")
    assert dev <= _bound(name)


def test_linreg_matches_scikit_learn():
    model = SerializedMLModel.load_serialized_model(GOLDEN["linreg"]["model"])
    assert isinstance(model, SerializedLinReg)
    pred = CasadiPredictor.from_serialized_model(model)
    assert isinstance(pred, CasadiLinReg) and (pred.n_out, pred.n_in) == (2, 4)
    x, y = np.asarray(GOLDEN["linreg"]["x"]), np.asarray(GOLDEN["linreg"]["y"])
    coef, icpt = np.asarray(model.parameters.coef), np.asarray(model.parameters.intercept)
    scale = np.abs(icpt) + np.abs(x[:, None, :] * coef[None]).sum(axis=2)
    assert np.all(np.abs(pred.predict_numpy(x) - y) <= 4.0 * EPS * scale)
    syms = [sx.sym(f"lr{i}") for i in range(4)]
    out = pred.predict(syms)
    assert not sx.network_sites(out)          # expanded into the graph, no network node
    got = np.array([sx.evaluate(out, dict(zip(syms, row))) for row in x], float)
    assert np.all(np.abs(got - y) <= 4.0 * EPS * scale)
    # zero coefficients are skipped
    sparse = gc.synthetic_linreg(gc.CCA, 5)
    e = CasadiLinReg(sparse).predict([sx.sym(f"lz{i}") for i in range(8)])[0]
    assert {s.name for s in sx.free_symbols([e])} == {f"lz{i}" for i in range(8) if i != 1}


@pytest.mark.parametrize("name", ["gpr_scalar", "gpr_ard"])
def test_tracer_nodes_match_autograd(name):
    """Value, gradient and Hessian nodes of a ``CasadiGPR`` output against torch autograd of the
    direct-difference forward of tests/gpr_cases.py.  The tracer evaluates the moment form
    (``z_i S0 - S1_i`` ...), whose rounding error is proportional to the sums of its terms in
    absolute value, ``|s_i| sum_j |w_j| (|z_i| + |T_ji|)`` and
    ``|s_i s_k| sum_j |w_j| ((|z_i| + |T_ji|)(|z_k| + |T_jk|) + delta_ik)``: the deviation over
    these sums stays within the bound of the value."""
    model = SerializedMLModel.load_serialized_model(GOLDEN[name]["model"])
    pred = CasadiGPR(model)
    syms = [sx.sym(f"{name}{i}") for i in range(pred.n_in)]
    out = pred.predict(syms)[0]
    assert out.op.startswith("annv")
    grad = [sx.diff(out, s) for s in syms]
    hess = [sx.diff(g, s) for g in grad for s in syms]
    fwd = gc.torch_forward(model)
    for row in np.asarray(GOLDEN[name]["x"])[:4]:
        vals = np.array(sx.evaluate([out] + grad + hess, dict(zip(syms, row))), float)
        xt = torch.tensor(row, dtype=torch.float64, requires_grad=True)
        f = lambda x: fwd(x[None])[0, 0]
        tv = float(f(xt))
        tg = torch.autograd.functional.jacobian(f, xt).numpy()
        th = torch.autograd.functional.hessian(f, xt).numpy()
        d, aw, s, z, T = _terms(model, row)
        m = np.abs(z[0])[None, :] + np.abs(T)                       # [NT, n_in]
        sg = np.abs(s) * (aw[0][:, None] * m).sum(axis=0)
        sh = np.abs(s[:, None] * s[None, :]) * (np.einsum("j,ji,jk->ik", aw[0], m, m) + np.eye(len(s)) * aw[0].sum())
        assert abs(vals[0] - tv) <= _bound(name) * aw[0].sum()
        assert np.all(np.abs(vals[1:1 + pred.n_in] - tg) <= _bound(name) * sg)
        assert np.all(np.abs(vals[1 + pred.n_in:].reshape(th.shape) - th) <= _bound(name) * sh)


def test_same_model_is_interned_once():
    model = SerializedMLModel.load_serialized_model(GOLDEN["gpr_ard"]["model"])
    a, b = CasadiGPR(model)._networks(), CasadiGPR(model.model_copy(deep=True))._networks()
    assert a == b and len(a) == 1
    assert isinstance(sx.network(a[0]), sx.RBFNetwork) and sx.network(a[0]).n_in == 3
    other = CasadiGPR(SerializedMLModel.load_serialized_model(GOLDEN["gpr_scalar"]["model"]))._networks()
    assert other != a


def _edited(name, edit):
    data = json.loads(json.dumps(GOLDEN[name]["model"]))
    edit(data)
    return data


@pytest.mark.parametrize("name,edit,match", [
    ("gpr_ard", lambda d: d["gpr_parameters"].update(alpha=[[a, a] for a in d["gpr_parameters"]["alpha"]]), "alpha"),
    ("gpr_ard", lambda d: d["gpr_parameters"].update(alpha=d["gpr_parameters"]["alpha"][:-1]), "alpha"),
    ("gpr_ard", lambda d: d["gpr_parameters"].update(X_train=[r[:-1] for r in d["gpr_parameters"]["X_train"]]), "X_train"),
    ("gpr_ard", lambda d: d["input"]["u1"].update(lag=2), "n_features_in"),
    ("gpr_ard", lambda d: d["data_handling"].update(mean=None), "Mean and std are not valid"),
    ("gpr_ard", lambda d: d["data_handling"].update(std=None), "Mean and std are not valid"),
    ("gpr_ard", lambda d: d["kernel_parameters"].update(length_scale=[1.0, 2.0]), "length_scale"),
    ("linreg", lambda d: d["parameters"].update(coef=d["parameters"]["coef"][0]), "coef"),
    ("linreg", lambda d: d["parameters"].update(coef=[r[:-1] for r in d["parameters"]["coef"]]), "coef"),
])
def test_validation_errors_name_the_field(name, edit, match):
    with pytest.raises(ValueError, match=match):
        SerializedMLModel.load_serialized_model(_edited(name, edit))


def test_keras_ann_and_unfitted_estimators_still_raise():
    with pytest.raises(NotImplementedError):
        SerializedMLModel.load_serialized_model({"model_type": "KerasANN", "dt": 1, "model_path": "m.keras"})

    class Unfitted:
        pass

    feats = GOLDEN["gpr_ard"]["model"]
    for cls in (SerializedGPR, SerializedLinReg):
        try:
            with pytest.raises(ValueError, match="unfitted"):
                cls.serialize(Unfitted(), dt=1, input=feats["input"], output=feats["output"])
        except ImportError:   # scikit-learn is optional: the import inside serialize comes first
            pass


def test_lagged_gpr_inputs_keep_the_column_order():
    """The T_CCA_0 model takes T_v with lags 0..2 and mDot with lags 0..1: the room's stage
    function evaluates the GPR on those columns in ``column_order`` (checked through the tracer
    against the model's own numeric twin at random lagged values)."""
    model = gc.synthetic_gpr(gc.CCA, 3, 9, per_feature=True)
    room = ex.RoomCCA(ml_model_sources=[gc.synthetic_gpr(gc.AIR, 2, 9), model], dt=1800)
    nxt = room.predict_step()["T_CCA_0"]
    cols = ["T_air", "T_v", "T_v_1", "T_v_2", "d", "mDot", "mDot_1", "T_CCA_0"]
    free = {s.name: s for s in sx.free_symbols([nxt])}
    assert set(free) == set(cols)
    rng = np.random.default_rng(4)
    row = np.array([296.0, 295.0, 294.0, 293.0, 120.0, 0.1, 0.08, 295.5]) + rng.normal(size=8) * 0.3
    got = float(sx.evaluate([nxt], {free[c]: v for c, v in zip(cols, row)})[0])
    want = row[7] + CasadiGPR(model).predict_numpy(row)[0, 0]
    assert abs(got - want) <= 4 * EPS * abs(want)


# ---------------------------------------------------------------------------
# generated code
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rooms():
    mp = pytest.MonkeyPatch()
    try:
        yield {name: gc.room(gc.models_of(name), 8, mp) for name in gc.CASE_NAMES}
    finally:
        mp.undo()


def test_network_section_dispatches_per_kind(rooms):
    calls = {}
    for name, case in rooms.items():
        src = case.backend.problem.gen.source
        rbf = re.findall(r"mpcx_net::eval_rbf<(\d+), (\d+), (\d+), (\w+), (\d+), (\d+)>", src)
        ann = re.findall(r"mpcx_net::eval<(\d+), (\d+), (\d+), (\d+), (\w+), (\d+), (\d+)>", src)
        calls[name] = (len(rbf), len(ann))
        assert "#define MPCX_NET_MFMA 1" in src
        for R, nin, nt, wv, nd1, nd2 in rbf:
            assert int(R) % 8 == 0 and int(nt) in (17, 20, 33)
        # the pair operand of an RBF network is two index reads, not a product table
        assert re.search(r"__constant__ int ANN\d+_P2hess\[\d+\]", src)
        assert ("_PWhess" in src) == bool(ann)
        # the kernel's stage functions read the entries instead of looping over the points
        body = src[src.index("gen_stage_fg_m("):src.index("// <<< device only")]
        assert not re.search(r"for \(int j = 0; j < (17|20|33); \+\+j\)", body)
    # (fg, gj, hess) per network; the mixed stage calls both evaluators, LinReg has no kernel
    assert calls == {"gpr20_gpr20": (6, 0), "gpr33_ann": (3, 3), "gpr17_linreg": (3, 0)}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_gpr_room_compiles_for_gfx950(rooms, tmp_path):
    gen = rooms["gpr33_ann"].backend.problem.gen
    src = tmp_path / "m.hip"
    src.write_text(gen.source)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "m.s"
    subprocess.run([hipcc, "--cuda-device-only", "-S", "--offload-arch=gfx950", "-O3", "-std=c++17",
                    f"-I{ROOT}/include", f"-I{ROOT}/agentlib-mpc_amd/csrc", str(src), "-o", str(out)],
                   check=True, capture_output=True)
    assert out.read_text().count("v_mfma_f64_16x16x4") >= 6


def test_training_points_above_the_cap_raise():
    from agentlib_mpc_amd import benchmarks as bm

    cap = codegen.RBF_MAX_POINTS
    big = gc.synthetic_gpr(gc.AIR, 1, cap + 1)
    with pytest.raises(ValueError, match=str(cap)):
        bm.room_nn(anns=[big, ex.room_cca_anns()[1]], N=2)


@pytest.mark.parametrize("name", gc.CASE_NAMES)
def test_host_build_of_gpr_room_takes_the_oracle_path(name, rooms):
    """The generated stage functions compiled for the host (`oracle/c/gen_model.cpp`, the
    per-lane loop over the training points) against the numpy oracle over the independent NLP
    (tests/gpr_cases.py): same status, iteration count, objective and solution.  Both run to
    tol 1e-10; the solutions then agree far inside 1e-7 relative."""
    case = rooms[name]
    prob = case.backend.problem
    mi = prob.mpc_inputs(case.current_vars, 0.0)
    mi.update(prob.initial_guess(mi))
    ref_in = prob.nlp_inputs(mi)
    p, lbw, ubw, w0 = prob.to_kernel(*[a[None] for a in ref_in])
    w, st, ok = cbuild.solve_generated_fleet(prob.gen, p, lbw, ubw, w0, threads=1, tol=1e-10, max_iter=500,
                                             acceptable_iter=0)
    op, olb, oub, ow = case.oracle_inputs
    ref = ipm.solve(case.oracle.functions(op), ow, olb, oub, case.oracle.lbg(op), case.oracle.ubg(op),
                    ipm.IPMOptions(tol=1e-10, max_iter=500, acceptable_iter=0))
    assert ref.success and ref.status == "Solve_Succeeded" and st[0]["status"] == 0
    assert st[0]["iter"] == ref.iterations
    np.testing.assert_allclose(st[0]["obj"], ref.f, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(prob.from_kernel(w[0], ref_in[1]), ref.x, rtol=1e-7, atol=1e-7)
