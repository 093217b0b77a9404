"""The NARX networks are evaluated on the FP64 matrix cores (CPU checks of the generated
code; the numerics are checked on the GPU by tests/test_net_eval.py, which runs
``mpcx_net::eval`` alone, and by the room_nn / C5 parity cases in tests/test_gpu_ipm.py,
tests/test_gpu_net_topologies.py and tests/test_gpu_admm.py).

Reference: the serialized ANN evaluated by CasADi inside IPOPT
(`agentlib_mpc/models/casadi_predictor.py:306-336`); here one batched
``[stages x call sites, inputs] x [inputs, hidden]`` product per wavefront and network
(csrc/mpcx_net_mfma.h).
"""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from agentlib_mpc_amd import benchmarks as bm
from agentlib_mpc_amd import symbolic as sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen(N=None):
    be, _ = bm.room_nn() if N is None else bm.room_nn(N=N)
    return be.problem.gen


def test_network_section_is_generated():
    src = _gen().source
    assert "#define MPCX_NET_MFMA 1" in src
    # every network is evaluated over all stages x call sites in one call per evaluation kind
    calls = re.findall(r"mpcx_net::eval<(\d+), (\d+), (\d+), (\d+), (\w+), (\d+), (\d+)>", src)
    assert len(calls) == 6   # 2 networks x (fg, gj, hess)
    n = int(re.search(r"#define MPCX_N (\d+)", src).group(1))
    for R, nin, H, act, wv, nd1, nd2 in calls:
        assert int(R) % n == 0 and int(H) == 32 and int(act) == sx.ACT_CODE["sigmoid"]
    # the stage functions of the kernel read the network entries instead of looping
    body = src[src.index("gen_stage_fg_m("):src.index("// <<< device only")]
    assert "for (int j = 0; j < 32; ++j)" not in body


def test_second_derivative_tables_are_pair_products():
    src = _gen().source
    m = re.search(r"__constant__ double ANN0_PWhess\[(\d+)\] = \{([^}]*)\}", src)
    d1 = re.search(r"__constant__ int ANN0_D1gj\[\d+\] = \{([^}]*)\}", src)
    assert m and d1
    rows = np.array([float(v) for v in m.group(2).split(",")]).reshape(-1, 32)

    def pair_products(w1):   # every row is W1[a] * W1[b] for some input pair (a >= b)
        return all(any(np.array_equal(r, w1[a] * w1[b]) for a in range(len(w1)) for b in range(a + 1))
                   for r in rows)

    assert any(pair_products(sx.network(i).W1) for i in range(len(sx._NETWORKS)))


def test_network_section_follows_the_topology():
    """A 20-unit tanh pair of networks (tests/configs.py::room_nn_topology): the template
    arguments carry the width and the activation code, the derivative tables stay sorted."""
    from tests import configs

    src = configs.room_nn_topology(20, "tanh", N=8).backend.problem.gen.source
    calls = re.findall(r"mpcx_net::eval<(\d+), (\d+), (\d+), (\d+), (\w+), (\d+), (\d+)>", src)
    n = int(re.search(r"#define MPCX_N (\d+)", src).group(1))
    assert len(calls) == 6   # 2 networks x (fg, gj, hess)
    for R, nin, H, act, wv, nd1, nd2 in calls:
        # n: the (super-)stages of the kernel, 8: the horizon
        assert int(R) > 0 and int(R) % n == 0 and int(R) % 8 == 0
        assert int(H) == 20 and int(act) == sx.ACT_CODE["tanh"]
    assert sorted(int(c[1]) for c in calls) == [8, 8, 8, 9, 9, 9]
    n_in = {}   # network id -> inputs, from the W1T table ([H][n_in])
    for nid, size in re.findall(r"__constant__ double ANN(\d+)_W1T\[(\d+)\] =", src):
        n_in[nid] = int(size) // 20
    tables = re.findall(r"__constant__ int ANN(\d+)_D1(\w+)\[(\d+)\] = \{([^}]*)\}", src)
    assert tables
    for nid, kind, size, body in tables:
        d1 = [int(v) for v in body.split(",")]
        assert len(d1) == int(size) and d1 == sorted(set(d1)), (nid, kind, d1)
        assert 0 <= d1[0] and d1[-1] < n_in[nid], (nid, kind, d1, n_in[nid])
        # the call of this kind and network has as many derivative columns
        assert any(int(c[5]) == len(d1) and int(c[1]) == n_in[nid] for c in calls)


def test_every_table_a_kind_names_is_declared():
    """For one network of each kind, with a gradient and a pair: every ``ANN<id>_<NAME>`` in the
    wave call and in the lane loop is a table of ``tables()`` or, with the evaluation kind
    appended, one of ``wave_tables()`` (``D1<kind>`` is the generator's own)."""
    rng = np.random.default_rng(3)
    nets = [sx.Network(rng.normal(size=(3, 5)), rng.normal(size=5), rng.normal(size=5), 0.25, "tanh"),
            sx.RBFNetwork(rng.normal(size=(6, 3)), rng.normal(size=6), rng.uniform(0.5, 2.0, 3), rng.normal(size=3)),
            sx.DeepNetwork(rng.normal(size=(3, 5)), rng.normal(size=5), rng.normal(size=(5, 4)), rng.normal(size=4),
                           rng.normal(size=4), -0.5, "sigmoid", "softplus")]
    d1, d2 = [0, 2], [(1, 0), (2, 2)]
    for net in nets:
        declared = {s for s, _ in net.tables()}
        wave = declared | {"D1hess"} | {s + "hess" for s, _ in net.wave_tables(d2)}
        call = net.wave_call("ANN7", "hess", 8, True, len(d1), len(d2), ["X", "O", "O + 8", "O + 24"])
        lane = "\n".join(net.emit_lane("ANN7", ["x0", "x1", "x2"], True, d1, d2, "q"))
        assert call.startswith(f"mpcx_net::{net.wave_fn}<8, 3, ") and call.endswith(", lane);")
        used_call, used_lane = set(re.findall(r"ANN7_(\w+)", call)), set(re.findall(r"ANN7_(\w+)", lane))
        assert used_call and used_call <= wave, (type(net).__name__, used_call - wave)
        assert used_lane and used_lane <= declared, (type(net).__name__, used_lane - declared)
        assert set(net.wave_pair_args) == {s for s, _ in net.wave_tables(d2)}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_code_object_issues_fp64_mfma(tmp_path):
    gen = _gen()
    src = tmp_path / "m.hip"
    src.write_text(gen.source)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "m.s"
    subprocess.run([hipcc, "--cuda-device-only", "-S", "--offload-arch=gfx950", "-O3", "-std=c++17",
                    f"-I{ROOT}/include", f"-I{ROOT}/agentlib-mpc_amd/csrc", str(src), "-o", str(out)],
                   check=True, capture_output=True)
    asm = out.read_text()
    assert asm.count("v_mfma_f64_16x16x4") >= 6
