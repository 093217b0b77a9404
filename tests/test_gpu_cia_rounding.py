"""``mpcx_cia_round`` on the device against the numpy restatement (tests/cia_cases.round_batch),
bit for bit: eta, B, the fixed bound rows and the status.

What can go wrong in the kernel is the state index at a level's window (the digits of a lane, the
window's shift between two levels), the walk back through the predecessor bytes, one agent's
LDS share leaking into another wave's, the last workgroup's idle waves, and a row written for an
agent that has none.  Hence every mode count, horizons of one interval and of the limit, agent
counts that are no multiple of the waves per workgroup, inputs that tie, and a guard row behind
every output."""

import numpy as np
import pytest
import torch

from agentlib_mpc_amd.runtime import native
from tests import cia_cases as cc

pytestmark = pytest.mark.gpu

#: (n_bin, N, agents): nc = 2 at N = 1, 2, 3, 10, 128, nc = 3 at 8, 33, nc = 4 at 6, 33 (and both at
#: the limit of 128); 1, 4, 5 and 257 agents
SHAPES = [(1, 1, 5), (1, 2, 4), (1, 3, 5), (1, 10, 1), (1, 10, 257), (1, 128, 5), (2, 10, 5),
          (3, 8, 1), (3, 8, 257), (3, 33, 5), (3, 128, 4), (4, 6, 4), (4, 6, 257), (4, 33, 5), (4, 128, 5)]
SENTINEL = -12345.0


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _batch(n_bin, N, agents, seed):
    """Host arrays of a batch with one spare row behind the agents: relaxed controls of every kind
    (random, tie-heavy, integral) scattered over rows of nw entries whose other entries are
    arbitrary, and for four agents or more one unusable agent and one switched off in the middle."""
    rng = np.random.default_rng(seed)
    nw = n_bin * N + 7
    pos = cc.scattered_positions(rng, n_bin, N, nw)
    b_rel = np.empty((agents, n_bin, N))
    for q, kind in enumerate(("random", "ties", "integral")):
        sel = np.arange(agents) % 3 == q
        b_rel[sel] = cc.random_controls(rng, int(sel.sum()), n_bin, N, kind)
    active = None
    if agents >= 4:
        b_rel[agents // 2, n_bin - 1, N // 2] = 1.0 + 2e-5 if agents % 2 else np.nan
        active = np.ones(agents, dtype=np.int32)
        active[agents // 2 - 1] = 0
    w = rng.normal(size=(agents + 1, nw)) * 3.0
    w[:agents, pos.reshape(-1)] = b_rel.reshape(agents, -1)
    lbw = rng.normal(size=(agents + 1, nw)) - 2.0
    ubw = lbw + rng.random((agents + 1, nw))
    return pos, nw, b_rel, active, w, lbw, ubw


def _expected(pos, b_rel, active, lbw, ubw, dt, agents):
    ref = cc.round_batch(b_rel, dt)
    ne = pos.size
    lf = np.full_like(lbw, SENTINEL)
    uf = np.full_like(ubw, SENTINEL)
    lf[:agents], uf[:agents] = lbw[:agents], ubw[:agents]
    okay = ref["status"] == cc.OK
    flat = ref["b_bin"].reshape(agents, ne)
    for a in np.flatnonzero(okay):
        lf[a, pos.reshape(-1)] = flat[a]
        uf[a, pos.reshape(-1)] = flat[a]
    bb = np.full((agents + 1, ne), SENTINEL)
    bb[:agents] = flat
    eta = np.r_[ref["eta"], SENTINEL]
    status = np.r_[ref["status"], -7].astype(np.int32)
    if active is not None:
        off = active == 0
        lf[:agents][off], uf[:agents][off], bb[:agents][off] = SENTINEL, SENTINEL, SENTINEL
        eta[:agents][off], status[:agents][off] = SENTINEL, -7
    return ref, lf, uf, bb, eta, status


def _run(pos, nw, n_bin, N, agents, active, w, lbw, ubw, dt, stream=None):
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    wd, ld, ud = up(w), up(lbw), up(ubw)
    slot = up(native.cia_slot_table(pos, nw))
    full = native.CIARounding(torch.full_like(ld, SENTINEL), torch.full_like(ud, SENTINEL),
                              torch.full((agents + 1, n_bin * N), SENTINEL, dtype=torch.float64, device=dev),
                              torch.full((agents + 1,), SENTINEL, dtype=torch.float64, device=dev),
                              torch.full((agents + 1,), -7, dtype=torch.int32, device=dev))
    out = native.CIARounding(*(t[:agents] for t in full))
    torch.cuda.synchronize()  # the uploads ran on the default stream
    native.cia_round(wd[:agents], ld[:agents], ud[:agents], slot, n_bin, N, dt, out=out,
                     active=None if active is None else up(active), stream=stream)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in full]


@pytest.mark.parametrize("n_bin,N,agents", SHAPES)
def test_kernel_matches_restatement_bit_for_bit(n_bin, N, agents):
    dt = 300.0
    pos, nw, b_rel, active, w, lbw, ubw = _batch(n_bin, N, agents, seed=97 * n_bin + 13 * N + agents)
    ref, *want = _expected(pos, b_rel, active, lbw, ubw, dt, agents)
    got = _run(pos, nw, n_bin, N, agents, active, w, lbw, ubw, dt)
    for name, g, x in zip(("lbw_fix", "ubw_fix", "b_bin", "eta", "status"), got, want):
        np.testing.assert_array_equal(g, x, err_msg=name)  # NaN equals NaN here; the spare row is in both
    # the batch is what it is meant to be
    if agents >= 4:
        assert ref["status"][agents // 2] == cc.BAD_INPUT and got[4][agents // 2 - 1] == -7
        assert (np.delete(ref["status"], agents // 2) == cc.OK).all()
    else:
        assert (ref["status"] == cc.OK).all()
    on = np.ones(agents, bool) if active is None else active != 0
    integral = (np.arange(agents) % 3 == 2) & on & (ref["status"] == cc.OK)
    assert (got[3][:agents][integral] == 0.0).all()


def test_launch_is_stream_ordered_and_reuses_its_buffers():
    """On a stream of the caller's, into buffers of an earlier call: the same bits as on the default
    stream."""
    n_bin, N, agents, dt = 3, 8, 5, 60.0
    pos, nw, b_rel, active, w, lbw, ubw = _batch(n_bin, N, agents, seed=11)
    base = _run(pos, nw, n_bin, N, agents, active, w, lbw, ubw, dt)
    side = torch.cuda.Stream()
    other = _run(pos, nw, n_bin, N, agents, active, w, lbw, ubw, dt, stream=side.cuda_stream)
    for g, x in zip(other, base):
        np.testing.assert_array_equal(g, x)
