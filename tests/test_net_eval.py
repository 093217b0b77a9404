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

import json
import os
import shutil

import numpy as np
import pytest

from tests import net_eval_harness as nh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c.name for c in nh.CONFIGS]
FACTOR = 8.0
FLOOR = 4.0 * nh.EPS

with open(os.path.join(ROOT, "tests", "golden", "net_eval_fp64_error.json")) as _f:
    FP64_ERROR = json.load(_f)


def _bound(name, kind):
    return max(FACTOR * FP64_ERROR[name][kind], FLOOR)


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

@pytest.fixture(scope="module")
def harness():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return nh.load(nh.build())


def run_config(lib, name):
    """Launch one config on its three input sets -> (Xback [NB, NX + GUARD], Oback [NB, NO + GUARD])."""
    import torch

    c, inp = nh.BY_NAME[name], nh.inputs(name)
    dev = torch.device("cuda:0")
    up = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    X, W1T, B1, W2, b2 = up(inp.X), up(inp.W1T), up(inp.b1), up(inp.w2), up(inp.b2)
    assert X.numel() == nh.NB * c.nx and W1T.numel() == nh.NB * c.H * c.NIN
    assert B1.numel() == W2.numel() == nh.NB * c.H and b2.numel() == nh.NB
    D1 = up(inp.d1, torch.int32) if c.ND1 else None
    PW = up(inp.PW) if c.ND2 else None
    assert PW is None or PW.numel() == nh.NB * c.ND2 * c.H
    Xb = torch.zeros(nh.NB, c.nx + nh.GUARD, dtype=torch.float64, device=dev)
    Ob = torch.zeros(nh.NB, c.nout + nh.GUARD, dtype=torch.float64, device=dev)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    torch.cuda.synchronize()
    rc = getattr(lib, f"launch_{name}")(ptr(X), ptr(W1T), ptr(B1), ptr(W2), ptr(b2), ptr(D1), ptr(PW),
                                        ptr(Xb), ptr(Ob), nh.NB)
    torch.cuda.synchronize()
    assert rc == 0
    return Xb.cpu().numpy(), Ob.cpu().numpy()


def split_outputs(c, ob):
    """One set's LDS output array -> V [R], G [R, ND1], Hd [R, ND2], guard."""
    R = c.R
    v, g, h = ob[:R], ob[R:R + R * c.ND1], ob[R + R * c.ND1:c.nout]
    return v, g.reshape(R, c.ND1), h.reshape(R, c.ND2), ob[c.nout:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_eval_matches_reference(name, harness):
    c, inp = nh.BY_NAME[name], nh.inputs(name)
    xb, ob = run_config(harness, name)
    outs = [split_outputs(c, ob[s]) for s in range(nh.NB)]
    for s in range(nh.NB):
        v, g, h, guard = outs[s]
        # the guards of both LDS arrays and the LDS input are untouched
        assert np.array_equal(guard, np.full(nh.GUARD, nh.SENTINEL)), (s, guard)
        assert np.array_equal(xb[s, c.nx:], np.full(nh.GUARD, nh.SENTINEL)), (s, xb[s, c.nx:])
        assert np.array_equal(xb[s, :c.nx].view(np.int64), inp.X[s].ravel().view(np.int64))
        # what the config does not produce stays NaN (an empty G or Hd block has no room of its
        # own: a stray write there lands in the next block or the guard), the rest is written
        assert np.isnan(v).all() if not c.WV else np.isfinite(v).all()
        assert np.isfinite(g).all() and np.isfinite(h).all()
    err = nh.errors_of(name, lambda s: (outs[s][0] if c.WV else None, outs[s][1] if c.ND1 else None,
                                        outs[s][2] if c.ND2 else None))
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
