"""GPU parity runs that provably take the IPM kernel's fallback paths.

The shipped builds eliminate every stage of these structures statically and never enter the
block chain (tests/test_gpu_ipm.py asserts ``n_block_chain == 0``), so their parity cases do not
execute ``interior_bk`` / ``trailing_backsolve`` (the dense stage path), ``seq_factor`` /
``seq_solve`` with ``bk_factor<NB, LDB>`` (the block chain), nor the chain pivots' LDL^T +
inverse pair and the serial recurrence.  Diagnostic builds of the main code object
(``MPCX_DEFINES``, as ``test_gpu_filter_matches_oracle`` builds its filter variants) force each
path; the counters show that it ran.  Tolerances: those of ``test_gpu_matches_oracle``.
"""

import numpy as np
import pytest
import torch

from agentlib_mpc_amd.runtime import native
from tests import configs
from tests.ipm_linalg_harness import nmu_of
from tests.test_gpu_ipm import RTOL_OBJ, _gpu_solve, _oracle, assert_matches_oracle

pytestmark = pytest.mark.gpu

CASES = ["one_room", "rng_room_mpc", "mhe_room"]
#: the chain flags on structures whose chain they change: blocks (NX > 1) for the LDL^T pair, the
#: scalar chain (NX = 1, no bordered rows, one DPP row: the scan is the shipped path) for the recurrence
CHAIN_VARIANTS = {"MPCX_CHAIN_BK": ["rng_room_mpc", "mhe_room"], "MPCX_CHAIN_SERIAL": ["one_room", "cubic_room"]}


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _solve_main(name, monkeypatch, define=None):
    """Three copies of the case on the main build compiled with ``define`` (no optional builds)."""
    for v in native.VARIANTS:
        monkeypatch.setenv(v.env, "0")
    if define is not None:
        monkeypatch.setenv("MPCX_DEFINES", define)
    else:
        monkeypatch.delenv("MPCX_DEFINES", raising=False)
    case = configs.CASES[name]()
    return case, _gpu_solve(case, n_copies=3, build="main")


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("define,counter", [("MPCX_NO_STATIC", "n_dense_stages"),
                                            ("MPCX_FORCE_BLOCK_CHAIN", "n_block_chain")])
def test_forced_fallback_matches_oracle(define, counter, name, monkeypatch):
    """Dense Bunch-Kaufman for every stage / the sequential block chain for every factorisation."""
    case, res = _solve_main(name, monkeypatch, define)
    ref = _oracle(case, key=(name, "{}"))
    assert ref.success, ref.status
    assert_matches_oracle(case, name, {}, ref, res)
    for r in res:
        assert r.stats[counter] > 0, r.stats
    print(define, name, [(r.stats["iter_count"], r.stats[counter]) for r in res])


@pytest.mark.parametrize("define,name", [(d, n) for d, names in CHAIN_VARIANTS.items() for n in names])
def test_chain_variant_matches_the_shipped_chain(define, name, monkeypatch):
    """The chain pivots through ``bk_factor`` + ``bk_inverse`` instead of the sweep (block chains),
    and the serial recurrence instead of the scan (scalar chains, where alone the flag acts): the
    same path as the unflagged build."""
    d = configs.CASES[name]().backend.problem.gen
    if define == "MPCX_CHAIN_SERIAL":   # acts inside ``if constexpr (NX == 1 && NMU == 0)`` only
        assert d.dims["NX"] == 1 and nmu_of(d) == 0 and d.dims["N"] <= 16
    else:
        assert d.dims["NX"] > 1
    _, base = _solve_main(name, monkeypatch)
    _, res = _solve_main(name, monkeypatch, define)
    for r, b in zip(res, base):
        assert b.stats["success"], b.stats
        assert (r.stats["return_status"], r.stats["iter_count"]) == (b.stats["return_status"], b.stats["iter_count"]), \
            (r.stats, b.stats)
        np.testing.assert_allclose(r.stats["obj"], b.stats["obj"], rtol=RTOL_OBJ, atol=1e-9)
