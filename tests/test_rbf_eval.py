"""``mpcx_net::eval_rbf`` (csrc/mpcx_net_mfma.h) against a high-precision reference, one kernel
per row of ``rbf_eval_harness.CONFIGS``: partial and full tiles of rows, k-steps, training
points, derivatives and pairs, a Hessian without gradient, ``WV = false``, derivative subsets
that do not start at input 0, seven streamed tiles, one-hot coefficients on the first and the
last training point.

Reference: mpmath at 60 digits on the direct-difference formulas of the GPR mean
(`agentlib_mpc/models/casadi_predictor.py:126-174`, per-feature length scale).  Tolerance: the
scaled error ``max |err| / S`` (``S``: the sum with absolute values of all factors) of the
kernel stays within 8 x that of the plain fp64 numpy evaluation of the kernel's algebra
(``symbolic.RBFNetwork.evaluate``; recorded in tests/golden/rbf_eval_fp64_error.json,
regenerate with ``python -m tests.rbf_eval_harness``), and never below a floor of 4 eps.  The
fourth input set (every weight underflows) is only asserted finite and below 1e-290.
"""

import os
import shutil

import numpy as np
import pytest

from tests import eval_harness_core as core
from tests import rbf_eval_harness as rh

NAMES = [c.name for c in rh.CONFIGS]
FP64_ERROR, _bound = core.golden("rbf_eval")


def test_config_table_hits_the_edges():
    assert set(FP64_ERROR) == set(NAMES)
    table = {(c.R, c.NIN, c.NT, c.WV, c.ND1, c.ND2, c.onehot) for c in rh.CONFIGS}
    assert table == {(1, 1, 1, True, 1, 1, False), (15, 3, 15, True, 0, 6, False), (16, 4, 16, False, 4, 0, False),
                     (17, 5, 17, True, 5, 15, False), (17, 5, 17, True, 3, 2, True), (33, 9, 33, True, 4, 6, False),
                     (20, 18, 48, True, 17, 21, False), (24, 6, 100, True, 6, 21, False)}
    for c in rh.CONFIGS:
        d1, pairs = c.d1(), c.pairs()
        assert len(d1) == c.ND1 and d1 == sorted(set(d1)) and all(0 <= i < c.NIN for i in d1)
        if 0 < c.ND1 < c.NIN:
            assert d1[0] > 0 and d1[-1] == c.NIN - 1
        assert len(pairs) == c.ND2 == len(set(pairs)) and all(0 <= b <= a < c.NIN for a, b in pairs)
        if c.ND1 == 0 and c.ND2:   # the S1 union: pair inputs outside the (empty) gradient list
            assert {i for p in pairs for i in p} - set(d1)
        kinds = {k for k, on in (("V", c.WV), ("G", c.ND1), ("H", c.ND2)) if on}
        assert set(FP64_ERROR[c.name]) == kinds


@pytest.mark.parametrize("name", NAMES)
def test_input_sets_are_where_they_should_be(name):
    c, inp = rh.BY_NAME[name], rh.inputs(name)
    e = [rh.exponents(inp, s) for s in range(rh.NB)]
    assert e[0].max(axis=1).min() > -10.0                   # inside: a training point nearby
    assert np.array_equal(e[1].max(axis=1), np.zeros(c.R))  # on a training point, exactly
    assert -60.0 <= e[2].min() <= -40.0                     # far
    assert e[3].max() < -1000.0                             # every exp underflows (exp(-745) = 0)
    if c.onehot:
        hot = [np.flatnonzero(inp.a[s]).tolist() for s in range(rh.NB)]
        assert hot == [[0], [c.NT - 1], [0], [c.NT - 1]]
    else:
        assert np.all(inp.a != 0.0)


@pytest.mark.parametrize("name", NAMES)
def test_rbf_network_evaluate_matches_reference(name):
    """The plain fp64 evaluation (the host side and the unit of the tolerance) against mpmath."""
    err = rh.errors_of(name, lambda s: rh.numpy_outputs(name, s))
    print(f"{name}: fp64 scaled error {err}, recorded {FP64_ERROR[name]}")
    assert set(err) == set(FP64_ERROR[name])
    for kind, e in err.items():
        assert e <= _bound(name, kind), (kind, e, FP64_ERROR[name][kind])
    for got in rh.numpy_outputs(name, 3):
        assert got is None or (np.isfinite(got).all() and np.abs(got).max() < rh.UNDERFLOW_BOUND)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_harness_source_compiles_for_gfx950():
    src = rh.generate_source()
    for c in rh.CONFIGS:
        assert ("mpcx_net::eval_rbf<R, NIN, NT, WV, ND1, ND2>" in src
                and f"rbf_eval_kernel<{c.R}, {c.NIN}, {c.NT}, {'true' if c.WV else 'false'}, "
                    f"{c.ND1}, {c.ND2}>" in src)
    lib = rh.build()
    assert lib.exists() and lib.stat().st_size > 0


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

harness = core.harness_fixture(rh)


def run_config(lib, name):
    """Launch one config on its four input sets -> (Xback [NB, NX + GUARD], Oback [NB, NO + GUARD])."""
    c, inp = rh.BY_NAME[name], rh.inputs(name)
    assert inp.T.size == rh.NB * c.NT * c.NIN
    assert inp.TT.size == inp.a.size == rh.NB * c.NT and inp.s.size == inp.t.size == rh.NB * c.NIN
    assert inp.P2.size == 2 * c.ND2
    return core.launch(lib, c, rh.NB, inp.X, [inp.T, inp.TT, inp.a, inp.s, inp.t, inp.d1 if c.ND1 else None,
                                              inp.P2 if c.ND2 else None])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_eval_rbf_matches_reference(name, harness):
    c, inp = rh.BY_NAME[name], rh.inputs(name)
    xb, ob = run_config(harness, name)
    outs = core.assert_guards_and_nans(c, inp.X, xb, ob)
    # every weight underflows: finite, and nothing above 1e-290
    for part in outs[3][:3]:
        assert np.all(np.abs(part[np.isfinite(part)]) < rh.UNDERFLOW_BOUND), part
    err = rh.errors_of(name, lambda s: core.produced(c, outs[s]))
    ratio = {k: e / FP64_ERROR[name][k] for k, e in err.items()}
    print(f"{name}: kernel scaled error {err}, fp64 {FP64_ERROR[name]}, kernel/fp64 {ratio}")
    assert set(err) == set(FP64_ERROR[name])
    for kind, e in err.items():
        assert e <= _bound(name, kind), (kind, e, FP64_ERROR[name][kind])
