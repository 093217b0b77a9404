"""GPU parity of the NARX room with networks other than the 32-unit sigmoid one: hidden widths
that are no multiple of the 16-unit MFMA tile and the tanh / softplus activations, on every
kernel build, against the oracle IPM (whose networks are evaluated by torch with autograd
derivatives, `oracle/nlps.py::_ann_torch`: no code shared with csrc/mpcx_net_mfma.h).

Same assertions and tolerances as ``test_gpu_ipm.py::test_gpu_matches_oracle``.  The oracle
converges at tol 1e-10 for the seed of ``configs.room_nn_topology`` in 8 / 7 / 21 iterations.
"""

import numpy as np
import pytest

from tests import configs
from tests.test_gpu_ipm import BUILDS, RTOL_OBJ, RTOL_TRAJ, _cuda, _gpu_solve, _oracle, _w_of  # noqa: F401

pytestmark = pytest.mark.gpu

TOPOLOGIES = [(20, "tanh"), (33, "sigmoid"), (16, "softplus")]
N = 8


@pytest.mark.parametrize("hidden,activation", TOPOLOGIES)
@pytest.mark.parametrize("build", BUILDS)
def test_gpu_net_topology_matches_oracle(hidden, activation, build):
    case = configs.room_nn_topology(hidden, activation, N=N)
    ref = _oracle(case, key=("room_nn_topology", hidden, activation, N))
    assert ref.success, ref.status
    res = _gpu_solve(case, n_copies=3, build=build)
    nlp = case.backend.problem.nlp
    for r in res:
        assert r.stats["success"], r.stats
        assert r.stats["iter_count"] > 0
        np.testing.assert_allclose(r.stats["obj"], ref.f, rtol=RTOL_OBJ, atol=1e-9)
        for gname, lay in nlp.var_groups.items():   # every variable group on its grid
            if not lay.dim:
                continue
            got = case.backend.problem.outputs(_w_of(case, r))[gname]
            want = ref.x[lay.index]
            first = sorted({t: j for j, t in reversed(list(enumerate(lay.grid)))}.values())
            np.testing.assert_allclose(got[:, first], want[:, first], rtol=RTOL_TRAJ,
                                       atol=1e-7 * max(1.0, np.abs(want).max()))
