"""GPU parity of the NARX room with two-hidden-layer networks (``mpcx_net::eval2`` inside the
solver): widths that are no multiple of the 16-unit MFMA tile on either layer, equal and mixed
activations, on every kernel build, against the oracle IPM (whose networks are evaluated by
torch with autograd derivatives, `oracle/nlps.py::_ann_torch`: no code shared with
csrc/mpcx_net_mfma.h).

Same assertions and tolerances as ``test_gpu_net_topologies.py``.  The oracle converges at tol
1e-10 for the seed of ``deep_cases.room_nn_deep`` in 8 / 8 iterations.
"""

import numpy as np
import pytest

from tests import deep_cases as dc
from tests.test_gpu_ipm import BUILDS, RTOL_OBJ, RTOL_TRAJ, _cuda, _gpu_solve, _oracle, _w_of  # noqa: F401

pytestmark = pytest.mark.gpu

TOPOLOGIES = [(20, 12, "tanh", "tanh"), (16, 33, "sigmoid", "softplus")]
N = 8


@pytest.mark.parametrize("h1,h2,act1,act2", TOPOLOGIES)
@pytest.mark.parametrize("build", BUILDS)
def test_gpu_deep_ann_matches_oracle(h1, h2, act1, act2, build):
    case = dc.room_nn_deep(h1, h2, act1, act2, N=N)
    assert "mpcx_net::eval2<" in case.backend.problem.gen.source
    ref = _oracle(case, key=("room_nn_deep", h1, h2, act1, act2, N))
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
