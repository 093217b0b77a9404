"""Unit harness for ``mpcx_net::eval2`` (csrc/mpcx_net_mfma.h, two hidden layers): the config
table, the HIP source generated from it, its build, the seeded inputs and the high-precision
reference.

The kernel wrapper, launcher and build are those of tests/eval_harness_core.py (one set of
tables per input set).

The reference evaluates the defining formulas in mpmath at 60 digits,

    a1 = W1^T x + b1, a2 = W2^T act1(a1) + b2, v = b3 + sum_j w3_j act2(a2_j),
    u_k = sum_j W2_kj w3_j act2'(a2_j),  g_i = sum_k W1_ik act1'(a1_k) u_k,
    J_ji = sum_k W2_kj act1'(a1_k) W1_ik,
    h_(a,b) = sum_k W1_ak W1_bk act1''(a1_k) u_k + sum_j w3_j act2''(a2_j) J_ja J_jb,

and for every element its scale ``S``: the same nested sums with every factor replaced by its
absolute value (a cancellation-free bound for act'').
"""

from __future__ import annotations

import dataclasses
import functools
from typing import List, Optional, Tuple

import mpmath as mp
import numpy as np

from tests import eval_harness_core as core
from tests.eval_harness_core import ACTS, DPS, EPS, GUARD, SENTINEL, _m, scaled_error  # noqa: F401
from tests.net_eval_harness import NB, _act_terms

#: largest |pre-activation| of either layer per input set (moderate, saturated, zero inputs): the
#: first layer's by scaling the inputs and its bias, the second layer's by scaling W2 and b2 of
#: that set (an unbounded act1 would otherwise push exp(a2) out of range)
TARGETS = ((3.0, 3.0), (20.0, 20.0), (None, 3.0))


@dataclasses.dataclass(frozen=True)
class Config(core.ConfigBase):
    R: int
    NIN: int
    H1: int
    H2: int
    act1: str
    act2: str
    WV: bool
    ND1: int
    ND2: int
    edge: str
    exact: bool = False                       # small-integer weights and inputs: every sum is exact in fp64
    d1_fixed: Optional[Tuple[int, ...]] = None
    pairs_fixed: Optional[Tuple[Tuple[int, int], ...]] = None

    @property
    def name(self) -> str:
        return (f"r{self.R}_i{self.NIN}_h{self.H1}_{self.H2}_{self.act1}_{self.act2}_"
                f"{'v' if self.WV else 'nov'}_g{self.ND1}_p{self.ND2}")

    def d1(self) -> List[int]:
        return list(self.d1_fixed) if self.d1_fixed is not None else super().d1()

    def pairs(self) -> List[Tuple[int, int]]:
        return [tuple(p) for p in self.pairs_fixed] if self.pairs_fixed is not None else super().pairs()


#: the instantiations, each chosen for the edge named (the single source of the generated
#: kernels and of the pytest parametrisation); every activation stands in either position
CONFIGS = [
    Config(1, 1, 1, 1, "exponential", "gaussian", True, 1, 1, "minimum of everything"),
    Config(15, 3, 15, 17, "softplus", "gaussian", True, 3, 6, "one below a tile (rows, layer 1), one above (layer 2)"),
    Config(17, 5, 17, 15, "tanh", "exponential", True, 5, 15, "one above a tile (rows, layer 1), one below (layer 2)"),
    Config(16, 4, 16, 16, "gaussian", "sigmoid", False, 4, 0, "exact tiles; no value output; no Hessian"),
    Config(17, 5, 17, 15, "linear", "linear", True, 3, 2, "bit-exact layout check", exact=True),
    Config(33, 9, 32, 32, "sigmoid", "sigmoid", True, 4, 6,
           "product-like; 3 row tiles; D1 a strict subset without input 0"),
    Config(12, 4, 20, 12, "exponential", "softplus", True, 0, 5, "Hessian without gradient"),
    Config(10, 6, 12, 20, "linear", "tanh", True, 2, 4, "pairs of inputs absent from D1; second Hessian term alone",
           d1_fixed=(1, 3), pairs_fixed=((2, 0), (4, 2), (5, 4), (5, 5))),
    Config(20, 18, 33, 20, "exponential", "gaussian", True, 17, 21, "ND1 > 16, ND2 > 16, 3 hidden-1 tiles, 5 k-steps"),
    Config(24, 6, 64, 64, "tanh", "softplus", True, 6, 21, "both widths at the cap; every pair of 6 inputs"),
]
BY_NAME = {c.name: c for c in CONFIGS}
assert len(BY_NAME) == len(CONFIGS) <= 16


# ---------------------------------------------------------------------------
# the HIP source and its build
# ---------------------------------------------------------------------------

KERNEL = core.Kernel(
    "deep_eval", "eval2",
    (("int", "R"), ("int", "NIN"), ("int", "H1"), ("int", "H2"), ("int", "ACT1"), ("int", "ACT2"), ("bool", "WV"),
     ("int", "ND1"), ("int", "ND2")),
    (("double", "W1T"), ("double", "B1"), ("double", "W2"), ("double", "B2"), ("double", "W3"), ("double", "b3"),
     ("int", "D1"), ("double", "PW"), ("int", "P2")),
    "W1T + set * (H1 * NIN), B1 + set * H1, W2 + set * (H1 * H2), B2 + set * H2, W3 + set * H2, b3[set], D1, "
    "ND2 > 0 ? PW + set * (ND2 * H1) : nullptr, P2")


def generate_source(configs=CONFIGS) -> str:
    return KERNEL.source(configs)


def build(include_dir=None, configs=CONFIGS):
    """Compile the harness (``eval_harness_core.build_source``)."""
    return KERNEL.build(configs, include_dir)


def load(lib_path):
    return core.load(lib_path, CONFIGS, KERNEL.nargs)


# ---------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------

@dataclasses.dataclass
class Inputs:
    X: np.ndarray      # [NB, R, NIN]
    W1: np.ndarray     # [NB, NIN, H1]
    b1: np.ndarray     # [NB, H1]
    W2: np.ndarray     # [NB, H1, H2], the layout of ANN<id>_W2
    b2: np.ndarray     # [NB, H2]
    w3: np.ndarray     # [NB, H2]
    b3: np.ndarray     # [NB]
    d1: List[int]
    pairs: List[Tuple[int, int]]

    @property
    def W1T(self) -> np.ndarray:   # [NB, H1, NIN], the layout of ANN<id>_W1T
        return np.ascontiguousarray(self.W1.transpose(0, 2, 1))

    @property
    def PW(self) -> np.ndarray:    # [NB, ND2, H1], as runtime/codegen.py builds ANN<id>_PW<kind>
        out = np.zeros((self.X.shape[0], len(self.pairs), self.W1.shape[2]))
        for p, (a, b) in enumerate(self.pairs):
            out[:, p, :] = self.W1[:, a, :] * self.W1[:, b, :]
        return out

    @property
    def P2(self) -> np.ndarray:    # [ND2, 2], as ANN<id>_P2<kind>
        return np.asarray(self.pairs, dtype=np.int32).reshape(-1, 2)


def _act_np(act: str, a: np.ndarray) -> np.ndarray:
    from agentlib_mpc_amd import symbolic as sx

    return sx.act_derivs(act, a)[0]


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> Inputs:
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    if c.exact:   # three sets of small integers (|.| <= 8), the last with X = 0
        shp = lambda *s: rng.integers(-8, 9, (NB, *s)).astype(float)
        X = shp(c.R, c.NIN)
        X[2] = 0.0
        return Inputs(X, shp(c.NIN, c.H1), shp(c.H1), shp(c.H1, c.H2), shp(c.H2), shp(c.H2), shp(), c.d1(), c.pairs())
    X = rng.uniform(-2.0, 2.0, (c.R, c.NIN))
    W1 = rng.normal(0.0, 1.0 / np.sqrt(c.NIN), (c.NIN, c.H1))
    b1 = rng.normal(0.0, 0.5, c.H1)
    W2 = rng.normal(0.0, 1.0 / np.sqrt(c.H1), (c.H1, c.H2))
    b2 = rng.normal(0.0, 0.5, c.H2)
    w3 = rng.normal(0.0, 1.0, c.H2)
    b3 = float(rng.normal(0.0, 1.0))
    Xs, b1s, W2s, b2s = [], [], [], []
    for t1, t2 in TARGETS:
        s = 0.0 if t1 is None else t1 / float(np.abs(X @ W1 + b1).max())
        xs, bs = s * X, (b1 if t1 is None else s * b1)
        s2 = t2 / float(np.abs(_act_np(c.act1, xs @ W1 + bs) @ W2 + b2).max())
        Xs.append(xs), b1s.append(bs), W2s.append(s2 * W2), b2s.append(s2 * b2)
    return Inputs(np.stack(Xs), np.stack([W1] * NB), np.stack(b1s), np.stack(W2s), np.stack(b2s),
                  np.stack([w3] * NB), np.full(NB, b3), c.d1(), c.pairs())


# ---------------------------------------------------------------------------
# the reference (mpmath)
# ---------------------------------------------------------------------------

@dataclasses.dataclass
class Reference:
    """Per input set: value/scale pairs as object arrays of mpf, and the largest |a1|, |a2|."""
    V: list
    G: list
    H: list
    amax: List[Tuple[float, float]]


def reference_of(act1, act2, X, W1, b1, W2, b2, w3, b3, d1, pairs):
    """((V, S_V), (G, S_G) | None, (H, S_H) | None, (max |a1|, max |a2|)) of one input set, in
    mpmath (call inside ``mp.workdps``); G over the inputs ``d1``, H over ``pairs``."""
    absf = np.frompyfunc(abs, 1, 1)
    X, W1, b1, W2, b2, w3, b3 = _m(X), _m(W1), _m(b1), _m(W2), _m(b2), _m(w3), mp.mpf(float(b3))
    A1 = X.dot(W1) + b1
    s0, s1, s2, S2 = np.frompyfunc(lambda a: _act_terms(act1, a), 1, 4)(A1)
    A2 = s0.dot(W2) + b2
    t0, t1, t2, T2 = np.frompyfunc(lambda a: _act_terms(act2, a), 1, 4)(A2)
    aw3, aW1, aW2 = absf(w3), absf(W1), absf(W2)
    amax = (float(max(absf(A1).ravel())), float(max(absf(A2).ravel())))
    V = ((t0 * w3).sum(axis=1) + b3, (absf(t0) * aw3).sum(axis=1) + abs(b3))
    u, au = (t1 * w3).dot(W2.T), (absf(t1) * aw3).dot(aW2.T)                  # [R, H1]
    G = Hh = None
    if len(d1):
        G = ((s1 * u).dot(W1[d1, :].T), (absf(s1) * au).dot(aW1[d1, :].T))
    if len(pairs):
        Pd = np.stack([W1[a] * W1[b] for a, b in pairs]).T                    # [H1, ND2], exact products
        cols = sorted({i for p in pairs for i in p})
        J = {i: (s1 * W1[i]).dot(W2) for i in cols}                           # [R, H2]
        aJ = {i: (absf(s1) * aW1[i]).dot(aW2) for i in cols}
        second = np.stack([(t2 * w3 * J[a] * J[b]).sum(axis=1) for a, b in pairs], axis=1)
        asecond = np.stack([(T2 * aw3 * aJ[a] * aJ[b]).sum(axis=1) for a, b in pairs], axis=1)
        Hh = ((s2 * u).dot(Pd) + second, (S2 * au).dot(absf(Pd)) + asecond)
    return V, G, Hh, amax


@functools.lru_cache(maxsize=None)
def reference(name: str) -> Reference:
    c, inp = BY_NAME[name], inputs(name)
    out = Reference([], [], [], [])
    with mp.workdps(DPS):
        for s in range(NB):
            V, G, Hh, amax = reference_of(c.act1, c.act2, inp.X[s], inp.W1[s], inp.b1[s], inp.W2[s], inp.b2[s],
                                          inp.w3[s], inp.b3[s], inp.d1, inp.pairs)
            out.V.append(V), out.G.append(G), out.H.append(Hh), out.amax.append(amax)
    return out


def numpy_outputs(name: str, s: int):
    """(V, G[:, d1], H[:, pairs]) of ``symbolic.DeepNetwork.evaluate`` (plain fp64) on input set s."""
    from agentlib_mpc_amd import symbolic as sx

    c, inp = BY_NAME[name], inputs(name)
    v, g, h = sx.DeepNetwork(inp.W1[s], inp.b1[s], inp.W2[s], inp.b2[s], inp.w3[s], float(inp.b3[s]),
                             c.act1, c.act2).evaluate(inp.X[s])
    G = g[:, inp.d1] if c.ND1 else None
    Hh = np.stack([h[:, a, b] for a, b in inp.pairs], axis=1) if c.ND2 else None
    return (v if c.WV else None), G, Hh


def errors_of(name: str, outputs) -> dict:
    """{"V" | "G" | "H": scaled error, max over the input sets}; ``outputs(s) -> (V, G, H)``."""
    return core.errors_of(reference(name), outputs, range(NB))


if __name__ == "__main__":   # prints the content of tests/golden/deep_eval_fp64_error.json
    import sys

    core.print_fp64_errors(sys.modules[__name__])
