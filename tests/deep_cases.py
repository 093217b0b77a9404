"""Two-hidden-layer NARX networks for the tests: seeded ``SerializedANN``s with the layout of
``tests/configs.py::topology_ann`` plus a second hidden layer, and the NARX room built on two
of them, once through the product backend and once through the oracle's restatement
(`oracle/nlps.py::room_nn`, networks evaluated by torch with autograd derivatives).
"""

from __future__ import annotations

import numpy as np

from agentlib_mpc_amd import benchmarks as bm
from oracle import nlps
from tests.configs import Case, _ACT_AT_ZERO


def deep_layers(n_in: int, seed: int, hidden, activations, n_out: int = 1, mean=None, var=None, out_act="linear"):
    """``BatchNormalization -> Dense(h, act) ... -> Dense(n_out, out_act)`` layer specs with seeded
    weights; the output bias centres the output at zero pre-activations."""
    rng = np.random.default_rng(seed)
    mean = np.zeros(n_in) if mean is None else mean
    var = np.ones(n_in) if var is None else var
    layers = [{"class_name": "BatchNormalization", "config": {"axis": -1, "epsilon": 0.001},
               "weights": [np.ones(n_in), np.zeros(n_in), mean, var]}]
    fan = n_in
    for h, act in zip(hidden, activations):
        layers.append({"class_name": "Dense", "config": {"units": h, "activation": act},
                       "weights": [rng.normal(0.0, 1.0 / np.sqrt(fan), (fan, h)), rng.normal(0.0, 0.1, h)]})
        fan = h
    W = rng.normal(0.0, 0.6 / np.sqrt(fan), (fan, n_out))
    b = -_ACT_AT_ZERO.get(activations[-1], 0.0) * W.sum(axis=0)
    layers.append({"class_name": "Dense", "config": {"units": n_out, "activation": out_act}, "weights": [W, b]})
    return layers


def serialized(layers, n_out: int = 1):
    """``SerializedANN`` of layer specs on plain features ``x0 ..`` (lag 1) and outputs ``y0 ..``."""
    from agentlib_mpc_amd.data_structures.ml_model_datatypes import Feature, OutputFeature
    from agentlib_mpc_amd.models.serialized_ml_model import SerializedANN

    n_in = next(l["weights"][0].shape[0] for l in layers if l["class_name"] == "Dense")
    inputs = {f"x{i}": Feature(name=f"x{i}", lag=1) for i in range(n_in)}
    outputs = {f"y{o}": OutputFeature(name=f"y{o}", lag=1, output_type="absolute", recursive=False)
               for o in range(n_out)}
    return SerializedANN.from_layers(layers, dt=1.0, input=inputs, output=outputs)


def deep_ann(features: dict, seed: int, hidden, activations, dt: float = 1800.0):
    """A seeded network on the lagged features of the three-zone example (statistics of
    ``models/examples.py::_FEATURE_SCALE`` in the BatchNormalization layer)."""
    from agentlib_mpc_amd.data_structures.ml_model_datatypes import Feature, OutputFeature, column_order
    from agentlib_mpc_amd.models import examples as ex
    from agentlib_mpc_amd.models.serialized_ml_model import SerializedANN

    inputs = {n: Feature(name=n, lag=l) for n, l in features["inputs"].items()}
    oname, olag = features["output"]
    outputs = {oname: OutputFeature(name=oname, lag=olag, output_type="difference", recursive=True)}
    cols = column_order(inputs, outputs)
    base = [c.rsplit("_", 1)[0] if c not in ex._FEATURE_SCALE else c for c in cols]
    mean = np.array([ex._FEATURE_SCALE[b][0] for b in base])
    var = np.array([ex._FEATURE_SCALE[b][1] ** 2 for b in base])
    layers = deep_layers(len(cols), seed, hidden, activations, mean=mean, var=var)
    return SerializedANN.from_layers(layers, dt=dt, input=inputs, output=outputs)


def room_nn_deep(h1, h2, act1, act2, N=8, seed=7, **kw) -> Case:
    """``room_nn`` with two seeded networks ``Dense(h1, act1) -> Dense(h2, act2) -> Dense(1)``."""
    from agentlib_mpc_amd.models import examples as ex

    anns = [deep_ann(ex.T_AIR_FEATURES, seed, (h1, h2), (act1, act2)),
            deep_ann(ex.T_CCA_FEATURES, seed + 1, (h1, h2), (act1, act2))]
    be, cv = bm.room_nn(anns=anns, N=N, **kw)
    air, cca = (nlps.ann_layers_from_serialized(a.layer_specs()) for a in anns)
    assert [l[0] for l in air] == [l[0] for l in cca] == ["bn", act1, act2, "linear"]
    prob = nlps.room_nn(air, cca, N=N)
    return Case(be, cv, prob, nlps.room_nn_inputs(prob, N=N, **kw))
