"""``mpcx_net::eval`` (csrc/mpcx_net_mfma.h) against a high-precision reference, one kernel per
row of ``net_eval_harness.CONFIGS``: partial and full tiles of rows, k-steps, hidden units,
derivatives and pairs, every activation code, ``WV = false``, derivative subsets that do not
start at input 0.

Reference: mpmath at 60 digits on the defining formulas of the serialized ANN
(`agentlib_mpc/models/casadi_predictor.py:306-336`).  Tolerance: the scaled error
``max |err| / S`` (``S``: the sum with absolute values of all factors) of the kernel stays
within 8 x that of the plain fp64 numpy evaluation of the same formulas
(``symbolic.Network.evaluate``; recorded in tests/golden/net_eval_fp64_error.json, regenerate
with ``python -m tests.net_eval_harness``), and never below a floor of 4 eps: the MFMA sums in
another order over at most 18 inputs / 48 hidden units, and the device exp / tanh are accurate
to a few ulp.
"""

import os
import shutil

import numpy as np
import pytest

from tests import eval_harness_core as core
from tests import net_eval_harness as nh

NAMES = [c.name for c in nh.CONFIGS]
FP64_ERROR, _bound = core.golden("net_eval")


def test_config_tables_hit_the_edges():
    assert set(FP64_ERROR) == set(NAMES)
    assert {c.act for c in nh.CONFIGS} == set(nh.ACTS)
    for c in nh.CONFIGS:
        d1, pairs = c.d1(), c.pairs()
        assert len(d1) == c.ND1 and d1 == sorted(set(d1)) and all(0 <= i < c.NIN for i in d1)
        if 0 < c.ND1 < c.NIN:
            assert d1[0] > 0 and d1[-1] == c.NIN - 1
        assert len(pairs) == c.ND2 == len(set(pairs)) and all(0 <= b <= a < c.NIN for a, b in pairs)
        if c.ND2:
            assert (c.NIN - 1, c.NIN - 1) in pairs
            assert c.NIN == 1 or any(a != b for a, b in pairs)
        kinds = {k for k, on in (("V", c.WV), ("G", c.ND1), ("H", c.ND2)) if on}
        assert set(FP64_ERROR[c.name]) == kinds


@pytest.mark.parametrize("name", [c.name for c in nh.CONFIGS if not c.exact])
def test_saturated_set_is_in_range(name):
    """Largest |pre-activation| of the saturated set in [15, 25] (saturates sigmoid, tanh and
    softplus; exp(a) and exp(-a^2) stay normal fp64 numbers).  The bit-exact row has three
    integer sets instead."""
    amax = nh.reference(name).amax
    assert 15.0 <= amax[1] <= 25.0, amax
    assert amax[0] < 15.0 and amax[2] == float(np.abs(nh.inputs(name).b1[2]).max())


@pytest.mark.parametrize("name", NAMES)
def test_network_evaluate_matches_reference(name):
    """The plain fp64 evaluation (the host side of the fleet and the unit of the tolerance)
    against mpmath, on the harness inputs: all six activations."""
    err = nh.errors_of(name, lambda s: nh.numpy_outputs(name, s))
    print(f"{name}: fp64 scaled error {err}, recorded {FP64_ERROR[name]}")
    assert set(err) == set(FP64_ERROR[name])
    for kind, e in err.items():
        assert e <= _bound(name, kind), (kind, e, FP64_ERROR[name][kind])


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_harness_source_compiles_for_gfx950():
    src = nh.generate_source()
    for c in nh.CONFIGS:
        assert ("mpcx_net::eval<R, NIN, H, ACT, WV, ND1, ND2>" in src
                and f"net_eval_kernel<{c.R}, {c.NIN}, {c.H}, {nh.ACTS.index(c.act)}, "
                    f"{'true' if c.WV else 'false'}, {c.ND1}, {c.ND2}>" in src)
    lib = nh.build()
    assert lib.exists() and lib.stat().st_size > 0


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

harness = core.harness_fixture(nh)


def run_config(lib, name):
    """Launch one config on its three input sets -> (Xback [NB, NX + GUARD], Oback [NB, NO + GUARD])."""
    c, inp = nh.BY_NAME[name], nh.inputs(name)
    assert inp.W1T.size == nh.NB * c.H * c.NIN
    assert inp.b1.size == inp.w2.size == nh.NB * c.H and inp.b2.size == nh.NB
    assert inp.PW.size == nh.NB * c.ND2 * c.H
    return core.launch(lib, c, nh.NB, inp.X, [inp.W1T, inp.b1, inp.w2, inp.b2, inp.d1 if c.ND1 else None,
                                              inp.PW if c.ND2 else None])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_eval_matches_reference(name, harness):
    c, inp = nh.BY_NAME[name], nh.inputs(name)
    xb, ob = run_config(harness, name)
    outs = core.assert_guards_and_nans(c, inp.X, xb, ob)
    err = nh.errors_of(name, lambda s: core.produced(c, outs[s]))
    print(f"{name}: kernel scaled error {err}, fp64 {FP64_ERROR[name]}")
    assert set(err) == set(FP64_ERROR[name])
    for kind, e in err.items():
        assert e <= _bound(name, kind), (kind, e, FP64_ERROR[name][kind])
    if c.exact:
        # integers: every intermediate sum is exact in fp64, so is the result
        for s in range(nh.NB):
            a = inp.X[s] @ inp.W1[s] + inp.b1[s]
            v, g, h, _ = outs[s]
            assert np.array_equal(v, a @ inp.w2[s] + inp.b2[s])
            assert np.array_equal(g, np.broadcast_to(inp.W1[s][inp.d1] @ inp.w2[s], g.shape))
            assert np.array_equal(h, np.zeros_like(h))
