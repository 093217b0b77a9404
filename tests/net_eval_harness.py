"""Unit harness for ``mpcx_net::eval`` (csrc/mpcx_net_mfma.h): the config table, the HIP
source generated from it, its build, the seeded inputs and the high-precision reference.

The kernel wrapper, launcher and build are those of tests/eval_harness_core.py.

The reference evaluates the defining formulas
``v = b2 + sum_j w2_j act(a_j)``, ``g_i = sum_j w2_j act'(a_j) W1_ij``,
``h_(i,k) = sum_j w2_j act''(a_j) W1_ij W1_kj`` in mpmath at 60 digits, with act, act' and
act'' written here from their definitions, and for every element its scale ``S``: the same sum
with every factor replaced by its absolute value (a cancellation-free bound for act'').
"""

from __future__ import annotations

import dataclasses
import functools
from typing import List, Tuple

import mpmath as mp
import numpy as np

from tests import eval_harness_core as core
from tests.eval_harness_core import ACTS, DPS, EPS, GUARD, SENTINEL, _m, build_source, scaled_error  # noqa: F401

NB = 3           # input sets per config: moderate, saturated, zero


@dataclasses.dataclass(frozen=True)
class Config(core.ConfigBase):
    R: int
    NIN: int
    H: int
    act: str
    WV: bool
    ND1: int
    ND2: int
    edge: str
    exact: bool = False   # small-integer weights and inputs: every sum is exact in fp64

    @property
    def name(self) -> str:
        return (f"r{self.R}_i{self.NIN}_h{self.H}_{self.act}_{'v' if self.WV else 'nov'}"
                f"_g{self.ND1}_p{self.ND2}")


#: the instantiations, each chosen for the edge named (the single source of the generated
#: kernels and of the pytest parametrisation)
CONFIGS = [
    Config(1, 1, 1, "sigmoid", True, 1, 1, "minimum of everything"),
    Config(15, 3, 15, "softplus", True, 0, 6, "one below each tile; Hessian without gradient"),
    Config(16, 4, 16, "linear", False, 4, 0, "exact tiles; no value output; no Hessian"),
    Config(17, 5, 17, "tanh", True, 5, 15, "one above each tile; full pair set"),
    Config(17, 5, 17, "linear", True, 3, 2, "bit-exact layout check", exact=True),
    Config(12, 9, 32, "sigmoid", True, 0, 0, "the product's fg kind"),
    Config(33, 9, 32, "sigmoid", True, 4, 6, "product-like; 3 row tiles; D1 a strict subset without input 0"),
    Config(20, 18, 33, "exponential", True, 17, 21, "ND1 > 16, ND2 > 16, 3 hidden tiles, 5 k-steps"),
    Config(48, 8, 48, "gaussian", True, 8, 17, "3 full hidden tiles, 3 full row tiles"),
    Config(24, 6, 20, "tanh", True, 6, 21, "every pair (a >= b) of 6 inputs"),
]
BY_NAME = {c.name: c for c in CONFIGS}
assert len(BY_NAME) == len(CONFIGS) <= 16


# ---------------------------------------------------------------------------
# the HIP source and its build
# ---------------------------------------------------------------------------

KERNEL = core.Kernel(
    "net_eval", "eval",
    (("int", "R"), ("int", "NIN"), ("int", "H"), ("int", "ACT"), ("bool", "WV"), ("int", "ND1"), ("int", "ND2")),
    (("double", "W1T"), ("double", "B1"), ("double", "W2"), ("double", "b2"), ("int", "D1"), ("double", "PW")),
    "W1T + set * (H * NIN), B1 + set * H, W2 + set * H, b2[set], D1, ND2 > 0 ? PW + set * (ND2 * H) : nullptr")


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
    W1: np.ndarray     # [NB, NIN, H]
    b1: np.ndarray     # [NB, H]
    w2: np.ndarray     # [NB, H]
    b2: np.ndarray     # [NB]
    d1: List[int]
    pairs: List[Tuple[int, int]]

    @property
    def W1T(self) -> np.ndarray:   # [NB, H, NIN], the layout of ANN<id>_W1T
        return np.ascontiguousarray(self.W1.transpose(0, 2, 1))

    @property
    def PW(self) -> np.ndarray:    # [NB, ND2, H], as runtime/codegen.py builds ANN<id>_PW<kind>
        out = np.zeros((self.X.shape[0], len(self.pairs), self.W1.shape[2]))
        for p, (a, b) in enumerate(self.pairs):
            out[:, p, :] = self.W1[:, a, :] * self.W1[:, b, :]
        return out


SATURATED_TARGET = 20.0   # largest |pre-activation| of the saturated set, inside [15, 25]


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> Inputs:
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    if c.exact:   # three sets of small integers (|.| <= 8), the last with X = 0
        shp = lambda *s: rng.integers(-8, 9, (NB, *s)).astype(float)
        X = shp(c.R, c.NIN)
        X[2] = 0.0
        return Inputs(X, shp(c.NIN, c.H), shp(c.H), shp(c.H), shp(), c.d1(), c.pairs())
    X = rng.uniform(-2.0, 2.0, (c.R, c.NIN))
    W1 = rng.normal(0.0, 1.0 / np.sqrt(c.NIN), (c.NIN, c.H))
    b1 = rng.normal(0.0, 0.5, c.H)
    w2 = rng.normal(0.0, 1.0, c.H)
    b2 = float(rng.normal(0.0, 1.0))
    # saturated: the whole pre-activation (inputs and bias) of the moderate set scaled
    s = SATURATED_TARGET / float(np.abs(X @ W1 + b1).max())
    return Inputs(np.stack([X, s * X, np.zeros_like(X)]), np.stack([W1] * NB), np.stack([b1, s * b1, b1]),
                  np.stack([w2] * NB), np.full(NB, b2), c.d1(), c.pairs())


# ---------------------------------------------------------------------------
# the reference (mpmath)
# ---------------------------------------------------------------------------

def _act_terms(act: str, a):
    """act(a), act'(a), act''(a) and a cancellation-free bound of |act''(a)|, from the
    definitions: sigmoid 1/(1+e^-a), tanh, identity, softplus log(1+e^a), e^a, e^(-a^2)."""
    if act == "sigmoid":
        e = mp.exp(-a)
        return 1 / (1 + e), e / (1 + e) ** 2, e * (e - 1) / (1 + e) ** 3, e * (e + 1) / (1 + e) ** 3
    if act == "tanh":
        t, q = mp.tanh(a), mp.sech(a) ** 2
        return t, q, -2 * t * q, 2 * abs(t) * q
    if act == "linear":
        return a, mp.mpf(1), mp.mpf(0), mp.mpf(0)
    if act == "softplus":
        e = mp.exp(-a)
        return mp.log(1 + mp.exp(a)), 1 / (1 + e), e / (1 + e) ** 2, e / (1 + e) ** 2
    if act == "exponential":
        e = mp.exp(a)
        return e, e, e, e
    assert act == "gaussian"
    g = mp.exp(-a * a)
    return g, -2 * a * g, (4 * a * a - 2) * g, (4 * a * a + 2) * g


@dataclasses.dataclass
class Reference:
    """Per input set: value/scale pairs as object arrays of mpf, and the largest |a|."""
    V: list
    G: list
    H: list
    amax: List[float]


@functools.lru_cache(maxsize=None)
def reference(name: str) -> Reference:
    c, inp = BY_NAME[name], inputs(name)
    out = Reference([], [], [], [])
    absf = np.frompyfunc(abs, 1, 1)
    with mp.workdps(DPS):
        terms = np.frompyfunc(lambda a: _act_terms(c.act, a), 1, 4)
        for s in range(NB):
            X, W1, b1, w2, b2 = _m(inp.X[s]), _m(inp.W1[s]), _m(inp.b1[s]), _m(inp.w2[s]), mp.mpf(float(inp.b2[s]))
            A = X.dot(W1) + b1
            s0, s1, s2, B2 = terms(A)
            aw2 = absf(w2)
            out.amax.append(float(max(absf(A).ravel())))
            out.V.append(((s0 * w2).sum(axis=1) + b2, (absf(s0) * aw2).sum(axis=1) + abs(b2)))
            if c.ND1:
                Wd = W1[inp.d1, :].T                                # [H, ND1]
                out.G.append(((s1 * w2).dot(Wd), (absf(s1) * aw2).dot(absf(Wd))))
            else:
                out.G.append(None)
            if c.ND2:
                Pd = np.stack([W1[a] * W1[b] for a, b in inp.pairs]).T   # [H, ND2], exact products
                out.H.append(((s2 * w2).dot(Pd), (B2 * aw2).dot(absf(Pd))))
            else:
                out.H.append(None)
    return out


def numpy_outputs(name: str, s: int):
    """(V, G[:, d1], H[:, pairs]) of ``symbolic.Network.evaluate`` (plain fp64) on input set s."""
    from agentlib_mpc_amd import symbolic as sx

    c, inp = BY_NAME[name], inputs(name)
    v, g, h = sx.Network(inp.W1[s], inp.b1[s], inp.w2[s], float(inp.b2[s]), c.act).evaluate(inp.X[s])
    G = g[:, inp.d1] if c.ND1 else None
    Hh = np.stack([h[:, a, b] for a, b in inp.pairs], axis=1) if c.ND2 else None
    return (v if c.WV else None), G, Hh


def errors_of(name: str, outputs) -> dict:
    """{"V" | "G" | "H": scaled error, max over the input sets}; ``outputs(s) -> (V, G, H)``."""
    return core.errors_of(reference(name), outputs, range(NB))


if __name__ == "__main__":   # prints the content of tests/golden/net_eval_fp64_error.json
    import sys

    core.print_fp64_errors(sys.modules[__name__])
