"""Two-hidden-layer NARX networks as opaque network nodes (CPU checks): the fp64 host twin
``symbolic.DeepNetwork`` against mpmath and against the expanded graph, the loader's routing,
the generated source of the deep room, and the per-lane loop form compiled for the host against
the torch-autograd oracle.  The wave pass ``mpcx_net::eval2`` runs alone in
tests/test_deep_eval.py and inside the solver in tests/test_gpu_deep_ann.py.

Reference: the trainer's ``layers: list[(units, activation)]``
(`agentlib_mpc/modules/ml_model_training/ml_model_trainer.py:592-626`) evaluated layer by layer
(`agentlib_mpc/models/casadi_predictor.py:306-336`).
"""

import re

import mpmath as mp
import numpy as np
import pytest

from agentlib_mpc_amd import symbolic as sx
from agentlib_mpc_amd.models.casadi_predictor import CasadiANN
from oracle import cbuild
from tests import configs, deep_cases as dc, deep_eval_harness as dh
from tests.net_eval_harness import scaled_error
from tests.test_gpu_ipm import RTOL_OBJ, RTOL_TRAJ, _oracle

ACTS = sx._ACTS
WIDTHS = (1, 15, 16, 17, 33, 64)
#: (act1, act2, H1, H2): every activation in either position, every width on either layer
TWIN_CASES = [(ACTS[i], ACTS[(i + 1 + i // 3) % 6], WIDTHS[i], WIDTHS[(i + 2) % 6]) for i in range(6)] + \
             [(ACTS[(i + 3) % 6], ACTS[i], WIDTHS[(i + 4) % 6], WIDTHS[i]) for i in range(6)]


def test_twin_cases_cover_activations_and_widths():
    assert {c[0] for c in TWIN_CASES} == {c[1] for c in TWIN_CASES} == set(ACTS)
    assert {c[2] for c in TWIN_CASES} == {c[3] for c in TWIN_CASES} == set(WIDTHS)
    assert any(a1 != a2 for a1, a2, _, _ in TWIN_CASES)


@pytest.mark.parametrize("act1,act2,h1,h2", TWIN_CASES)
def test_deep_network_evaluate_matches_mpmath(act1, act2, h1, h2):
    """Value, gradient and full Hessian of ``DeepNetwork.evaluate`` against the defining formulas
    at 60 digits.  Bound: 64 eps of the element's scale (the nested sums with absolute values of
    all factors): every output is a sum of at most 64 x 64 products of fp64-rounded factors, whose
    rounding errors add up like a random walk, and exp / tanh / log are within an ulp."""
    n_in, R = 3, 4
    rng = np.random.default_rng(1000 * h1 + h2)
    W1 = rng.normal(0.0, 1.0 / np.sqrt(n_in), (n_in, h1))
    b1 = rng.normal(0.0, 0.5, h1)
    W2 = rng.normal(0.0, 1.0 / np.sqrt(h1), (h1, h2))
    b2 = rng.normal(0.0, 0.5, h2)
    if act1 in ("exponential", "softplus", "linear"):   # keep the second pre-activation moderate
        W2 *= 0.5
    w3, b3 = rng.normal(0.0, 1.0, h2), float(rng.normal())
    X = rng.uniform(-1.5, 1.5, (R, n_in))
    every = [(a, b) for a in range(n_in) for b in range(a + 1)]
    v, g, h = sx.DeepNetwork(W1, b1, W2, b2, w3, b3, act1, act2).evaluate(X)
    assert v.shape == (R,) and g.shape == (R, n_in) and h.shape == (R, n_in, n_in)
    np.testing.assert_allclose(h, h.transpose(0, 2, 1), rtol=0, atol=64 * dh.EPS * np.abs(h).max())
    with mp.workdps(dh.DPS):
        V, G, Hh, _ = dh.reference_of(act1, act2, X, W1, b1, W2, b2, w3, b3, list(range(n_in)), every)
        errs = (scaled_error(v, V), scaled_error(g, G),
                scaled_error(np.stack([h[:, a, b] for a, b in every], axis=1), Hh))
    print(act1, act2, h1, h2, errs)
    assert max(errs) <= 64 * dh.EPS, errs


def _deep_ann(hidden=(20, 12), acts=("tanh", "sigmoid"), seed=3, n_out=1, **kw):
    layers = dc.deep_layers(5, seed, hidden, acts, n_out=n_out, mean=np.linspace(-1.0, 1.0, 5),
                            var=np.linspace(0.5, 2.0, 5), **kw)
    return dc.serialized(layers, n_out), layers


@pytest.mark.parametrize("acts", [("tanh", "sigmoid"), ("softplus", "gaussian"), ("exponential", "linear")])
def test_deep_node_derivatives_match_expanded_graph(acts):
    """The opaque node (value, gradient, Hessian via the network derivative rules) == the
    layer-by-layer expanded graph differentiated by the generic AD."""
    net = CasadiANN(_deep_ann(acts=acts)[0])
    xs = [sx.sym(f"x{i}") for i in range(net.n_in)]
    opaque = net.predict(xs)[0]
    assert opaque.op.startswith("annv") and isinstance(sx.network(sx.ann_parse(opaque.op)[1]), sx.DeepNetwork)
    expanded = xs
    for spec in net.layers:
        expanded = CasadiANN._layer_sym(spec, expanded)
    expanded = expanded[0]
    sel = [0, 2, 4]
    outs = []
    for e in (opaque, expanded):
        g = [sx.diff(e, xs[i]) for i in sel]
        h = [sx.diff(gi, xs[j]) for gi in g for j in sel]
        outs.append([e] + g + h)
    vals = dict(zip(xs, np.array([0.3, -0.7, 1.1, 0.2, -1.4])))
    a = np.array(sx.evaluate(outs[0], vals), float)
    b = np.array(sx.evaluate(outs[1], vals), float)
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------------
# loader routing
# ---------------------------------------------------------------------------

def _sites(ann):
    net = CasadiANN(ann)
    xs = [sx.sym(f"x{i}") for i in range(net.n_in)]
    outs = net.predict(xs)
    return net, xs, outs, sx.network_sites(outs)


def test_two_hidden_layers_become_network_sites():
    ann, _ = _deep_ann()
    net, _, outs, sites = _sites(ann)
    assert len(outs) == 1 and len(sites) == 1
    (nid, _), = sites
    d = sx.network(nid)
    assert isinstance(d, sx.DeepNetwork) and (d.n_in, d.H1, d.H2, d.act1, d.act2) == (5, 20, 12, "tanh", "sigmoid")
    x = np.random.default_rng(0).normal(size=(7, 5))
    np.testing.assert_allclose(d.evaluate(x)[0], net.predict_numpy(x)[:, 0], rtol=1e-12, atol=1e-14)
    # identical weights intern to one id
    again = _sites(dc.serialized(_deep_ann()[1]))[3]
    assert [nid for nid, _ in again] == [nid]


def test_two_outputs_share_only_the_hidden_weights():
    ann, layers = _deep_ann(n_out=2)
    net, _, outs, sites = _sites(ann)
    ids = [nid for nid, _ in sites]
    assert len(outs) == 2 and len(set(ids)) == 2
    a, b = (sx.network(i) for i in ids)
    for name in ("W1", "b1", "W2", "b2"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
    W3, b3 = layers[-1]["weights"]
    np.testing.assert_array_equal(np.stack([a.w3, b.w3], axis=1), W3)
    assert (a.b3, b.b3) == tuple(b3) and not np.array_equal(a.w3, b.w3)
    x = np.random.default_rng(1).normal(size=(3, 5))
    np.testing.assert_allclose(np.stack([a.evaluate(x)[0], b.evaluate(x)[0]], axis=1), net.predict_numpy(x),
                               rtol=1e-12, atol=1e-14)


def _between_bn():
    layers = dc.deep_layers(5, 3, (8, 6), ("tanh", "tanh"))
    layers.insert(2, {"class_name": "BatchNormalization", "config": {"axis": -1, "epsilon": 0.001},
                      "weights": [np.ones(8), np.zeros(8), np.full(8, 0.1), np.full(8, 1.5)]})
    return layers


@pytest.mark.parametrize("layers", [
    pytest.param(lambda: dc.deep_layers(5, 3, (8, 6, 4), ("tanh", "tanh", "tanh")), id="three_hidden_layers"),
    pytest.param(lambda: dc.deep_layers(5, 3, (8, 6), ("tanh", "relu")), id="relu"),
    pytest.param(lambda: dc.deep_layers(5, 3, (8, sx.DEEP_MAX_WIDTH + 1), ("tanh", "tanh")), id="width_65"),
    pytest.param(lambda: dc.deep_layers(5, 3, (sx.DEEP_MAX_WIDTH + 1, 8), ("tanh", "tanh")), id="width_65_first"),
    pytest.param(lambda: dc.deep_layers(5, 3, (8, 6), ("tanh", "tanh"), out_act="sigmoid"), id="sigmoid_output"),
    pytest.param(_between_bn, id="normalisation_between_dense"),
])
def test_topologies_outside_the_scope_keep_expanding(layers):
    """No network site, no error, and ``predict`` still equals ``predict_numpy``."""
    net, xs, outs, sites = _sites(dc.serialized(layers()))
    assert not sites and len(outs) == 1
    x = np.random.default_rng(2).normal(size=5)
    got = sx.evaluate(outs, dict(zip(xs, x)))
    np.testing.assert_allclose(np.array(got, float).ravel(), net.predict_numpy(x).ravel(), rtol=1e-12, atol=1e-14)


def test_width_at_the_cap_is_a_node():
    w = sx.DEEP_MAX_WIDTH
    assert w == 64
    _, _, _, sites = _sites(dc.serialized(dc.deep_layers(5, 3, (w, w), ("tanh", "tanh"))))
    assert len(sites) == 1


# ---------------------------------------------------------------------------
# generated source
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def room16():
    return dc.room_nn_deep(16, 16, "tanh", "tanh", N=8)


def test_deep_room_source_calls_eval2(room16):
    """N = 8 room with two 16/16 tanh networks: six ``eval2`` calls carrying both widths and both
    activation codes, no ``eval`` call, the pair tables of either Hessian term, and a source within
    2x of the 16-unit one-layer structure's (the expanded form measured 27x)."""
    src = room16.backend.problem.gen.source
    calls = re.findall(r"mpcx_net::eval2<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\w+), (\d+), (\d+)>", src)
    assert len(calls) == 6 and len(re.findall(r"mpcx_net::eval2<", src)) == 6   # 2 networks x (fg, gj, hess)
    assert "mpcx_net::eval<" not in src and "mpcx_net::eval_rbf<" not in src
    n = int(re.search(r"#define MPCX_N (\d+)", src).group(1))
    for R, nin, h1, h2, a1, a2, wv, nd1, nd2 in calls:
        assert int(R) > 0 and int(R) % n == 0
        assert (int(h1), int(h2)) == (16, 16) and int(a1) == int(a2) == sx.ACT_CODE["tanh"]
    assert sorted(int(c[1]) for c in calls) == [8, 8, 8, 9, 9, 9]
    w2 = re.findall(r"__constant__ double ANN(\d+)_W2\[(\d+)\] =", src)
    assert len(w2) == 2 and all(int(size) == 16 * 16 for _, size in w2)
    n_in = {nid: int(size) // 16 for nid, size in re.findall(r"__constant__ double ANN(\d+)_W1T\[(\d+)\] =", src)}
    # either Hessian term has its table, over the same pairs
    pw = dict(re.findall(r"__constant__ double ANN(\d+)_PWhess\[(\d+)\]", src))
    p2 = {nid: body for nid, body in re.findall(r"__constant__ int ANN(\d+)_P2hess\[\d+\] = \{([^}]*)\}", src)}
    assert pw and set(pw) == set(p2)
    for nid, body in p2.items():
        idx = [int(v) for v in body.split(",")]
        pairs = list(zip(idx[::2], idx[1::2]))
        assert pairs == sorted(set(pairs)) and all(0 <= b <= a < n_in[nid] for a, b in pairs)
        assert int(pw[nid]) == len(pairs) * 16
        assert any(int(c[8]) == len(pairs) for c in calls)
    one = configs.room_nn_topology(16, "tanh", N=8).backend.problem.gen.source
    print(f"deep 16/16 source {len(src)} B, one-layer 16 source {len(one)} B")
    assert len(src) <= 2 * len(one)
    # the stage functions of the kernel read the network entries instead of looping
    body = src[src.index("gen_stage_fg_m("):src.index("// <<< device only")]
    assert "for (int j = 0; j < 16; ++j)" not in body


def test_flop_count_prices_both_layers():
    net = sx.DeepNetwork(np.ones((3, 5)), np.zeros(5), np.ones((5, 4)), np.zeros(4), np.ones(4), 0.0, "tanh", "tanh")
    nid = sx.register_network(net)
    xs = [sx.sym(f"f{i}") for i in range(3)]
    y = sx.ann_call(nid, xs)
    fv = sx.flop_count([y])
    assert fv >= 2 * 3 * 5 + 2 * 5 * 4 + 2 * 4           # the three products of the forward pass
    g = sx.diff(y, xs[0])
    h = sx.diff(g, xs[1])
    assert sx.flop_count([y, g]) >= fv + 2 * 5 * 4         # u = W2 c1
    assert sx.flop_count([y, g, h]) >= sx.flop_count([y, g]) + 2 * 5 * 4   # a Jacobian column


# ---------------------------------------------------------------------------
# host loop form
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("h1,h2,act1,act2", [(20, 12, "tanh", "tanh"), (16, 33, "sigmoid", "softplus")])
def test_host_build_of_deep_room_reaches_the_oracle_optimum(h1, h2, act1, act2):
    """The generated stage functions compiled for the host (`oracle/c/gen_model.cpp`; the network
    entries by the per-lane loops of ``symbolic.DeepNetwork.emit_lane``) solve the N = 8 deep room to
    the optimum of the oracle IPM over the independent NLP, whose networks torch evaluates with
    autograd derivatives (`oracle/nlps.py::_ann_torch`).  Tolerances of tests/test_gpu_ipm.py.  The
    oracle converges at tol 1e-10 for the seed of ``deep_cases.room_nn_deep`` in 8 / 8 iterations
    (the host build in 9 / 7)."""
    case = dc.room_nn_deep(h1, h2, act1, act2, N=8)
    ref = _oracle(case, key=("room_nn_deep", h1, h2, act1, act2, 8))
    assert ref.success and ref.status == "Solve_Succeeded", ref.status
    prob = case.backend.problem
    mi = prob.mpc_inputs(case.current_vars, 0.0)
    mi.update(prob.initial_guess(mi))
    ref_in = prob.nlp_inputs(mi)
    p, lbw, ubw, w0 = prob.to_kernel(*[a[None] for a in ref_in])
    w, st, ok = cbuild.solve_generated_fleet(prob.gen, p, lbw, ubw, w0, threads=1, tol=1e-10, max_iter=500,
                                             acceptable_iter=0)
    print(f"oracle {ref.iterations} iterations, host build {st[0]['iter']}")
    assert st[0]["status"] == 0 and st[0]["iter"] > 0
    np.testing.assert_allclose(st[0]["obj"], ref.f, rtol=RTOL_OBJ, atol=1e-9)
    x = prob.from_kernel(w[0], ref_in[1])
    np.testing.assert_allclose(x, ref.x, rtol=RTOL_TRAJ, atol=1e-7 * max(1.0, np.abs(ref.x).max()))
