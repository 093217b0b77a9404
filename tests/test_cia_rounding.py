"""The rounding step of the CIA backend on the CPU: the numpy restatements of tests/cia_cases.py
against exhaustive enumeration, and the argument checks of ``mpcx_cia_round`` and its Python
wrapper, which answer before any GPU call.  The kernel itself: tests/test_gpu_cia_rounding.py."""

import ctypes

import numpy as np
import pytest

from agentlib_mpc_amd.runtime import native
from tests import cia_cases as cc

#: (n_bin, N, kind, agents): nc = 2 / 3 / 4 at N <= 10 / 8 / 6 -- enumeration is nc^N
SMALL = [(1, 10, "random", 6), (1, 10, "ties", 8), (1, 7, "ties", 6), (1, 1, "random", 3), (1, 2, "ties", 4),
         (2, 9, "random", 4), (2, 10, "ties", 4),
         (3, 8, "random", 6), (3, 7, "ties", 6), (3, 3, "random", 3),
         (4, 6, "random", 6), (4, 6, "ties", 6), (4, 5, "random", 3)]


@pytest.mark.parametrize("n_bin,N,kind,agents", SMALL)
def test_restatements_match_enumeration(n_bin, N, kind, agents):
    """eta of the banded recursion, of the full recursion and of all nc^N assignments are the same
    double; B is one mode per interval, attains eta, and both recursions pick the same B (the tie
    rules are part of the statement)."""
    rng = np.random.default_rng(1000 * n_bin + 10 * N + len(kind))
    b_rel = cc.random_controls(rng, agents, n_bin, N, kind)
    out = cc.round_batch(b_rel, dt=1.0)
    b, bad = cc.modes(b_rel)
    assert not bad.any() and (out["status"] == cc.OK).all()
    for a in range(agents):
        eta_all = cc.enumerate_eta(b[a])[0]
        eta_dp, B_dp = cc.dp_full(b[a])
        assert out["eta"][a] == eta_dp == eta_all
        B = out["b_bin"][a]
        full = np.vstack([B, 1.0 - B]) if n_bin == 1 else B
        assert set(np.unique(full)) <= {0.0, 1.0} and (full.sum(axis=0) == 1.0).all()
        assert cc.deviation(b[a], full) == eta_all
        np.testing.assert_array_equal(full, B_dp)
        assert out["eta"][a] <= out["eta_sur"][a]


def test_quarter_grid_inputs_do_tie():
    """The tie-heavy inputs are what they claim: several assignments attain the optimum, so the
    tie rules decide B."""
    rng = np.random.default_rng(5)
    b, _ = cc.modes(cc.random_controls(rng, 6, 1, 8, "ties"))
    tied = 0
    for a in range(6):
        S = cc.running_sums(b[a])
        eta = cc.enumerate_eta(b[a])[0]
        n = 0
        for bits in range(2 ** 8):
            B0 = np.array([(bits >> i) & 1 for i in range(8)], dtype=np.float64)
            n += float(np.max(np.abs(S - np.cumsum(np.vstack([B0, 1 - B0]), axis=1)))) == eta
        tied += n > 1
    assert tied >= 3


@pytest.mark.parametrize("n_bin,N", [(1, 10), (2, 7), (3, 8), (4, 6)])
def test_integral_input_is_returned(n_bin, N):
    b_rel = cc.random_controls(np.random.default_rng(n_bin), 5, n_bin, N, "integral")
    out = cc.round_batch(b_rel, dt=300.0)
    assert (out["status"] == cc.OK).all() and (out["eta"] == 0.0).all()
    np.testing.assert_array_equal(out["b_bin"], b_rel)


def test_dt_is_applied_last():
    b_rel = cc.random_controls(np.random.default_rng(3), 4, 3, 8)
    one, many = cc.round_batch(b_rel, 1.0), cc.round_batch(b_rel, 300.0)
    np.testing.assert_array_equal(many["eta"], 300.0 * one["eta"])
    np.testing.assert_array_equal(many["b_bin"], one["b_bin"])


def test_clip_edges():
    """(-1e-5, 0) counts as 0 and (1, 1 + 1e-5) as 1; anything further out, a NaN, an infinity or a
    column that does not sum to 1 is BAD_INPUT with NaN results, agent by agent."""
    N = 6
    base = np.array([0.3, 0.0, 1.0, 0.6, 1.0, 0.0])
    rows = {"inside": base,
            "clipped": np.array([0.3, -0.9e-5, 1.0 + 0.9e-5, 0.6, 1.0, 0.0]),
            "above": np.array([0.3, 0.0, 1.0 + 2e-5, 0.6, 1.0, 0.0]),
            "below": np.array([0.3, -2e-5, 1.0, 0.6, 1.0, 0.0]),
            "nan": np.array([0.3, np.nan, 1.0, 0.6, 1.0, 0.0]),
            "inf": np.array([0.3, 0.0, np.inf, 0.6, 1.0, 0.0])}
    out = cc.round_batch(np.stack(list(rows.values()))[:, None, :], dt=2.0)
    assert out["status"].tolist() == [cc.OK, cc.OK, cc.BAD_INPUT, cc.BAD_INPUT, cc.BAD_INPUT, cc.BAD_INPUT]
    assert out["eta"][1] == out["eta"][0] and np.isfinite(out["eta"][0])
    np.testing.assert_array_equal(out["b_bin"][1], out["b_bin"][0])
    assert np.isnan(out["eta"][2:]).all() and np.isnan(out["b_bin"][2:]).all()
    assert out["b_bin"][0].shape == (1, N)
    # two controls: the columns must sum to 1 within 1e-6
    two = np.stack([np.vstack([base, 1.0 - base]), np.vstack([base, 1.0 - base])])
    two[1, 1, 3] += 3e-6
    two[0, 1, 3] += 0.5e-6
    assert cc.round_batch(two, dt=1.0)["status"].tolist() == [cc.OK, cc.BAD_INPUT]


def _call(lib, n_agents=1, nw=16, n_bin=2, N=4, dt=1.0, null=()):
    """mpcx_cia_round with host buffers of the right size: every case here must be refused before
    the launch, so nothing ever reads them."""
    f = lambda name, arr: None if name in null else ctypes.c_void_p(arr.ctypes.data)  # noqa: E731
    rowsz = max(nw, 1) * max(n_agents, 1)
    d = {n: np.zeros(rowsz) for n in ("w", "lbw", "ubw", "lbw_fix", "ubw_fix")}
    d["slot"] = np.full(max(nw, 1), -1, dtype=np.int32)
    d["b_bin"] = np.zeros(max(n_agents, 1) * 4 * 128)
    d["eta"] = np.zeros(max(n_agents, 1))
    d["status"] = np.zeros(max(n_agents, 1), dtype=np.int32)
    return lib.mpcx_cia_round(n_agents, nw, n_bin, N, dt, f("slot", d["slot"]), f("w", d["w"]), f("lbw", d["lbw"]),
                              f("ubw", d["ubw"]), f("lbw_fix", d["lbw_fix"]), f("ubw_fix", d["ubw_fix"]),
                              f("b_bin", d["b_bin"]), f("eta", d["eta"]), f("status", d["status"]), None, None)


def test_entry_point_checks_its_arguments():
    lib = native.load_library()
    assert native.CIA_MAX_MODES == cc.MAX_MODES and native.CIA_MAX_INTERVALS == cc.MAX_INTERVALS
    assert native.CIA_MAX_STATES == cc.MAX_STATES
    assert (native.CIA_OK, native.CIA_BAD_INPUT, native.CIA_BAND_OVERFLOW) == (cc.OK, cc.BAD_INPUT, cc.BAND_OVERFLOW)
    header = (native.INCLUDE / "mpcx.h").read_text()
    for name, value in (("MAX_MODES", 4), ("MAX_INTERVALS", 128), ("MAX_STATES", 64), ("OK", 0), ("BAD_INPUT", 1),
                        ("BAND_OVERFLOW", 2)):
        assert f"#define MPCX_CIA_{name} {value}\n" in header
    for kw in (dict(n_agents=-1), dict(nw=0), dict(n_bin=0), dict(n_bin=5, nw=64), dict(N=0), dict(N=129, nw=1024),
               dict(n_bin=4, N=5, nw=19), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")), dict(dt=float("inf")),
               *[dict(null=(n,)) for n in ("slot", "w", "lbw", "ubw", "lbw_fix", "ubw_fix", "eta", "status")]):
        assert _call(lib, **kw) == native.ERR_ARG, kw
    # nothing to do is not an error, and b_bin is optional (no agents: no launch)
    assert _call(lib, n_agents=0) == 0
    assert _call(lib, n_agents=0, null=("b_bin",)) == 0
    assert _call(lib, n_agents=0, n_bin=4, N=128, nw=512) == 0


def test_wrapper_raises_before_any_device_call():
    """Host tensors, wrong shapes and limits are Python errors: the wrapper never reaches HIP."""
    import torch

    w = torch.zeros((2, 16), dtype=torch.float64)
    slot = torch.from_numpy(native.cia_slot_table([[0, 1, 2, 3]], 16))
    for kw, match in ((dict(n_bin=5), "n_bin"), (dict(n_bin=0), "n_bin"), (dict(n_intervals=129), "n_intervals"),
                      (dict(n_intervals=0), "n_intervals"), (dict(dt=0.0), "dt"), (dict(dt=float("nan")), "dt"),
                      (dict(n_bin=4, n_intervals=5), "smaller"), (dict(), "device tensor")):
        args = dict(n_bin=1, n_intervals=4, dt=1.0)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            native.cia_round(w, w, w, slot, **args)
    with pytest.raises(ValueError, match="n_agents, nw"):
        native.cia_round(torch.zeros(16, dtype=torch.float64), w, w, slot, 1, 4, 1.0)


def test_slot_table():
    table = native.cia_slot_table([[7, 2, 9], [0, 4, 1]], 10)
    assert table.dtype == np.int32 and table.tolist() == [3, 5, 1, -1, 4, -1, -1, 0, -1, 2]
    for bad in ([[0, 10]], [[-1, 2]], [[3, 3]], [], [1, 2]):
        with pytest.raises(ValueError):
            native.cia_slot_table(bad, 10)
