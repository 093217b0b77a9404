"""Writes tests/golden/gpr_golden.json: three fitted scikit-learn models in the reference's
serialized layout (`agentlib_mpc/models/serialized_ml_model.py`) and ``predict`` of the fitted
estimator at 16 seeded points each, with ``data_handling.scale`` applied as the reference does.

    python scripts/make_gpr_golden.py

Seeded; needs scikit-learn (recorded in the file), which the tests do not.
  gpr_scalar   ConstantKernel * RBF + WhiteKernel, scalar length scale, normalised inputs,
               scale 2.5, 33 training points, 5 features (one input with lag 2)
  gpr_ard      the same with one length scale per feature, 20 training points, 3 features
  linreg       LinearRegression with two targets, 4 features
"""

import json
import os
import sys

import numpy as np
import sklearn
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
from sklearn.linear_model import LinearRegression

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "agentlib-mpc_amd")]

from agentlib_mpc_amd.data_structures.ml_model_datatypes import Feature, OutputFeature  # noqa: E402
from agentlib_mpc_amd.models.serialized_ml_model import SerializedGPR, SerializedLinReg  # noqa: E402

N_POINTS = 16


def _features(lags, outputs):
    inp = {n: Feature(name=n, lag=l) for n, l in lags.items()}
    out = {n: OutputFeature(name=n, lag=1, output_type="absolute", recursive=True) for n in outputs}
    return inp, out


def gpr(seed, nt, lags, ard, scale):
    rng = np.random.default_rng(seed)
    inp, out = _features(lags, ["y"])
    nf = sum(lags.values()) + 1
    centre, spread = rng.uniform(-5.0, 300.0, nf), rng.uniform(0.5, 40.0, nf)
    X = centre + spread * rng.normal(size=(nt, nf))
    mean, std = X.mean(axis=0), X.std(axis=0)
    Xn = (X - mean) / std
    y = np.sin(Xn @ rng.normal(size=nf)) + 0.3 * Xn[:, 0] * Xn[:, -1] + 0.01 * rng.normal(size=nt)
    kernel = ConstantKernel() * RBF(length_scale=np.ones(nf) if ard else 1.0) + WhiteKernel(noise_level=1e-3)
    model = GaussianProcessRegressor(kernel=kernel, random_state=seed).fit(Xn, y / scale)
    model.data_handling = {"normalize": True, "scale": scale, "mean": mean, "std": std}
    ser = SerializedGPR.serialize(model, dt=900, input=inp, output=out)
    xs = centre + spread * rng.normal(size=(N_POINTS, nf))
    ys = model.predict((xs - mean) / std) * scale
    return {"model": json.loads(ser.model_dump_json()), "x": xs.tolist(), "y": ys.tolist()}


def linreg(seed):
    rng = np.random.default_rng(seed)
    inp, out = _features({"u0": 2}, ["y0", "y1"])
    X = rng.normal(size=(40, 4)) * np.array([3.0, 3.0, 10.0, 0.5]) + np.array([290.0, 290.0, 0.0, 1.0])
    Y = X @ rng.normal(size=(4, 2)) + np.array([1.5, -20.0]) + 0.05 * rng.normal(size=(40, 2))
    model = LinearRegression().fit(X, Y)
    ser = SerializedLinReg.serialize(model, dt=900, input=inp, output=out)
    xs = rng.normal(size=(N_POINTS, 4)) * np.array([3.0, 3.0, 10.0, 0.5]) + np.array([290.0, 290.0, 0.0, 1.0])
    return {"model": json.loads(ser.model_dump_json()), "x": xs.tolist(), "y": model.predict(xs).tolist()}


if __name__ == "__main__":
    golden = {"sklearn": sklearn.__version__,
              "gpr_scalar": gpr(1, 33, {"u0": 1, "u1": 2, "u2": 1}, False, 2.5),
              "gpr_ard": gpr(2, 20, {"u0": 1, "u1": 1}, True, 0.5),
              "linreg": linreg(3)}
    path = os.path.join(ROOT, "tests", "golden", "gpr_golden.json")
    with open(path, "w") as f:
        json.dump(golden, f)
    print(path, os.path.getsize(path), "bytes")
