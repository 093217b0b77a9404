"""``mpcx_net::eval2`` (csrc/mpcx_net_mfma.h, two hidden layers) against a high-precision
reference, one kernel per row of ``deep_eval_harness.CONFIGS``: partial and full tiles of rows,
k-steps and hidden units of either layer, derivatives and pairs, every activation code in either
position, ``WV = false``, a Hessian without gradient, pairs of inputs the gradient list lacks.

Reference: mpmath at 60 digits on the defining formulas of a Dense -> Dense -> Dense(linear)
model (`agentlib_mpc/models/casadi_predictor.py:306-336` applied per layer).  Tolerance: the
scaled error ``max |err| / S`` (``S``: the nested sums with absolute values of all factors) of
the kernel stays within 8 x that of the plain fp64 numpy evaluation of the same formulas
(``symbolic.DeepNetwork.evaluate``; recorded in tests/golden/deep_eval_fp64_error.json,
regenerate with ``python -m tests.deep_eval_harness``), and never below a floor of 4 eps: the
bound of tests/test_net_eval.py.
"""

import os
import shutil

import numpy as np
import pytest

from tests import eval_harness_core as core
from tests import deep_eval_harness as dh

NAMES = [c.name for c in dh.CONFIGS]
FP64_ERROR, _bound = core.golden("deep_eval")


def test_config_tables_hit_the_edges():
    assert set(FP64_ERROR) == set(NAMES)
    assert {c.act1 for c in dh.CONFIGS} == {c.act2 for c in dh.CONFIGS} == set(dh.ACTS)
    assert any(c.act1 != c.act2 for c in dh.CONFIGS)
    edges = {(c.R, c.NIN, c.H1, c.H2) for c in dh.CONFIGS}
    assert {(1, 1, 1, 1), (15, 3, 15, 17), (17, 5, 17, 15), (16, 4, 16, 16), (33, 9, 32, 32), (20, 18, 33, 20),
            (24, 6, 64, 64)} <= edges
    assert any(c.ND1 == 0 and c.ND2 > 0 for c in dh.CONFIGS)
    assert any(not c.WV and c.ND2 == 0 for c in dh.CONFIGS)
    assert any(c.ND1 > 16 and c.ND2 > 16 for c in dh.CONFIGS)
    assert any(c.ND1 and c.ND2 and not {i for p in c.pairs() for i in p} & set(c.d1()) for c in dh.CONFIGS)
    for c in dh.CONFIGS:
        d1, pairs = c.d1(), c.pairs()
        assert len(d1) == c.ND1 and d1 == sorted(set(d1)) and all(0 <= i < c.NIN for i in d1)
        if 0 < c.ND1 < c.NIN and c.d1_fixed is None:
            assert d1[0] > 0 and d1[-1] == c.NIN - 1
        assert len(pairs) == c.ND2 == len(set(pairs)) and all(0 <= b <= a < c.NIN for a, b in pairs)
        assert pairs == sorted(pairs)
        if c.ND2:
            assert (c.NIN - 1, c.NIN - 1) in pairs
            assert c.NIN == 1 or any(a != b for a, b in pairs)
        kinds = {k for k, on in (("V", c.WV), ("G", c.ND1), ("H", c.ND2)) if on}
        assert set(FP64_ERROR[c.name]) == kinds


@pytest.mark.parametrize("name", [c.name for c in dh.CONFIGS if not c.exact])
def test_input_sets_are_in_range(name):
    """Largest |pre-activation| of either layer: 3 on the moderate set, 20 on the saturated one
    (saturates sigmoid, tanh and softplus; exp(a) and exp(-a^2) stay normal fp64 numbers), the
    bias alone / 3 on the zero set."""
    amax = dh.reference(name).amax
    np.testing.assert_allclose(amax[0], (3.0, 3.0), rtol=1e-12)
    np.testing.assert_allclose(amax[1], (20.0, 20.0), rtol=1e-12)
    assert amax[2][0] == float(np.abs(dh.inputs(name).b1[2]).max())
    np.testing.assert_allclose(amax[2][1], 3.0, rtol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_deep_network_evaluate_matches_reference(name):
    """The plain fp64 evaluation (the host twin and the unit of the tolerance) against mpmath on
    the harness inputs."""
    err = dh.errors_of(name, lambda s: dh.numpy_outputs(name, s))
    print(f"{name}: fp64 scaled error {err}, recorded {FP64_ERROR[name]}")
    assert set(err) == set(FP64_ERROR[name])
    for kind, e in err.items():
        assert e <= _bound(name, kind), (kind, e, FP64_ERROR[name][kind])


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_harness_source_compiles_for_gfx950():
    src = dh.generate_source()
    for c in dh.CONFIGS:
        assert ("mpcx_net::eval2<R, NIN, H1, H2, ACT1, ACT2, WV, ND1, ND2>" in src
                and f"deep_eval_kernel<{c.R}, {c.NIN}, {c.H1}, {c.H2}, {dh.ACTS.index(c.act1)}, "
                    f"{dh.ACTS.index(c.act2)}, {'true' if c.WV else 'false'}, {c.ND1}, {c.ND2}>" in src)
    lib = dh.build()
    assert lib.exists() and lib.stat().st_size > 0


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

harness = core.harness_fixture(dh)


def run_config(lib, name):
    """Launch one config on its three input sets -> (Xback [NB, NX + GUARD], Oback [NB, NO + GUARD])."""
    c, inp = dh.BY_NAME[name], dh.inputs(name)
    assert inp.W1T.size == dh.NB * c.H1 * c.NIN
    assert inp.W2.size == dh.NB * c.H1 * c.H2 and inp.b1.size == dh.NB * c.H1
    assert inp.b2.size == inp.w3.size == dh.NB * c.H2 and inp.b3.size == dh.NB
    assert inp.PW.size == dh.NB * c.ND2 * c.H1 and inp.P2.size == 2 * c.ND2
    return core.launch(lib, c, dh.NB, inp.X, [inp.W1T, inp.b1, inp.W2, inp.b2, inp.w3, inp.b3,
                                              inp.d1 if c.ND1 else None, inp.PW if c.ND2 else None,
                                              inp.P2 if c.ND2 else None])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_eval2_matches_reference(name, harness):
    c, inp = dh.BY_NAME[name], dh.inputs(name)
    xb, ob = run_config(harness, name)
    outs = core.assert_guards_and_nans(c, inp.X, xb, ob)
    err = dh.errors_of(name, lambda s: core.produced(c, outs[s]))
    print(f"{name}: kernel scaled error {err}, fp64 {FP64_ERROR[name]}")
    assert set(err) == set(FP64_ERROR[name])
    for kind, e in err.items():
        assert e <= _bound(name, kind), (kind, e, FP64_ERROR[name][kind])
    if c.exact:
        # integers, linear / linear: every intermediate sum is exact in fp64, so is the result;
        # the gradient is W1 W2 w3 in every row and the Hessian exactly zero
        for s in range(dh.NB):
            a2 = (inp.X[s] @ inp.W1[s] + inp.b1[s]) @ inp.W2[s] + inp.b2[s]
            v, g, h, _ = outs[s]
            assert np.array_equal(v, a2 @ inp.w3[s] + inp.b3[s])
            assert np.array_equal(g, np.broadcast_to((inp.W1[s] @ inp.W2[s] @ inp.w3[s])[inp.d1], g.shape))
            assert np.array_equal(h, np.zeros_like(h))
