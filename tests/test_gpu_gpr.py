"""GPU parity of the NARX room with GPR and linear-regression models on every kernel build,
against the oracle IPM over the independent NLP of tests/gpr_cases.py (torch forwards in
direct-difference form with autograd derivatives: no code shared with csrc/mpcx_net_mfma.h).

Cases (N = 8, three copies): two GPRs of 20 training points with a scalar length scale; a GPR
of 33 points with per-feature length scales beside the shipped 32-unit sigmoid ANN, where
``eval`` and ``eval_rbf`` run in one stage; a GPR of 17 points beside a linear regression.
17, 20 and 33 are the smallest sizes that cross an edge of the 16-point tile.

Same assertions and tolerances as ``test_gpu_net_topologies.py::test_gpu_net_topology_matches_oracle``.
The oracle converges at tol 1e-10 in 7 / 8 / 7 iterations.
"""

import numpy as np
import pytest

from tests import gpr_cases as gc
from tests.test_gpu_ipm import BUILDS, RTOL_OBJ, RTOL_TRAJ, _cuda, _gpu_solve, _oracle, _w_of  # noqa: F401

pytestmark = pytest.mark.gpu

N = 8


@pytest.fixture(scope="module")
def rooms():
    mp = pytest.MonkeyPatch()
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = gc.room(gc.models_of(name), N, mp)
        return cache[name]
    try:
        yield get
    finally:
        mp.undo()


@pytest.mark.parametrize("name", gc.CASE_NAMES)
@pytest.mark.parametrize("build", BUILDS)
def test_gpu_gpr_room_matches_oracle(name, build, rooms):
    case = rooms(name)
    ref = _oracle(case, key=("room_gpr", name, N))
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
