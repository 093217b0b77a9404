"""Unit harness for ``mpcx_net::eval_rbf`` (csrc/mpcx_net_mfma.h): the config table, the HIP
source generated from it, its build, the seeded inputs and the high-precision reference.

The kernel wrapper, launcher and build are those of tests/eval_harness_core.py; the tables
(``T``, ``TT``, ``A``, ``S``, ``SH``, one of each per input set) stay in global memory.

The reference evaluates the direct-difference formulas, ``z = s o x + t``, ``d_j = z - T_j``,

    w_j = a_j exp(-1/2 |d_j|^2),  v = sum_j w_j,  g_i = -s_i sum_j w_j d_ji,
    h_(i,k) = s_i s_k sum_j w_j (d_ji d_jk - delta_ik)

in mpmath at 60 digits, and for every element its scale ``S``: the same sum with every factor
replaced by its absolute value (``|d_ji d_jk| + delta_ik`` for the Hessian).

Input sets per config: 0 inside the training cloud; 1 every row exactly on a training point
(``s = 1``, ``t = 0`` and ``X`` a copy of rows of ``T``, so ``z = T_j`` whatever the
rounding of ``s x + t``: that term's gradient contribution vanishes); 2 far, the smallest
exponent ``-1/2 |d_j|^2`` over rows and points at -50; 3 so far that every weight underflows.
On a training point the direct-difference sums lose their dominant term, while the moment form
``z_i S0 - S1_i`` of the kernel and of ``RBFNetwork.evaluate`` keeps that term's rounding
noise: the fp64 unit of set 1 is therefore far above eps where the other weights are small
(18 inputs: 1e-10), and the kernel is held to 8 x that unit like everywhere else.
"""

from __future__ import annotations

import dataclasses
import functools
from typing import List, Tuple

import mpmath as mp
import numpy as np

from tests import eval_harness_core as core
from tests.eval_harness_core import DPS, EPS, GUARD, SENTINEL, _m, scaled_error  # noqa: F401

NB = 4                 # input sets per config: inside, on a training point, far, underflow
CHECKED = (0, 1, 2)    # the sets compared with the reference (3: finite and below 1e-290)
FAR_EXPONENT = -50.0   # smallest exponent of the far set, inside [-60, -40]
UNDERFLOW_BOUND = 1e-290


@dataclasses.dataclass(frozen=True)
class Config(core.ConfigBase):
    R: int
    NIN: int
    NT: int
    WV: bool
    ND1: int
    ND2: int
    edge: str
    onehot: bool = False   # a = one unit entry: point 0 in sets 0 and 2, point NT - 1 in sets 1 and 3

    @property
    def name(self) -> str:
        return (f"r{self.R}_i{self.NIN}_t{self.NT}_{'v' if self.WV else 'nov'}_g{self.ND1}_p{self.ND2}"
                f"{'_onehot' if self.onehot else ''}")

    @property
    def subset_seed(self) -> int:
        # d1() and pairs() were drawn under the name of the one-layer config of the same shape
        return core.name_seed(f"r{self.R}_i{self.NIN}_h{self.NT}_linear_{'v' if self.WV else 'nov'}"
                              f"_g{self.ND1}_p{self.ND2}")


#: the instantiations, each chosen for the edge named (the single source of the generated
#: kernels and of the pytest parametrisation)
CONFIGS = [
    Config(1, 1, 1, True, 1, 1, "minimum of everything"),
    Config(15, 3, 15, True, 0, 6, "one below each tile; Hessian without gradient (S1 of the pairs is still needed)"),
    Config(16, 4, 16, False, 4, 0, "exact tiles; no value output; no Hessian"),
    Config(17, 5, 17, True, 5, 15, "one above each tile; full pair set"),
    Config(17, 5, 17, True, 3, 2, "layout check for the first and the last training point", onehot=True),
    Config(33, 9, 33, True, 4, 6, "product-like; 3 row tiles; D1 a strict subset without input 0"),
    Config(20, 18, 48, True, 17, 21, "ND1 > 16, ND2 > 16, 5 k-steps"),
    Config(24, 6, 100, True, 6, 21, "seven streamed tiles, the last partial; every pair of 6 inputs"),
]
BY_NAME = {c.name: c for c in CONFIGS}
assert len(BY_NAME) == len(CONFIGS)


# ---------------------------------------------------------------------------
# the HIP source and its build
# ---------------------------------------------------------------------------

KERNEL = core.Kernel(
    "rbf_eval", "eval_rbf",
    (("int", "R"), ("int", "NIN"), ("int", "NT"), ("bool", "WV"), ("int", "ND1"), ("int", "ND2")),
    (("double", "T"), ("double", "TT"), ("double", "A"), ("double", "S"), ("double", "SH"), ("int", "D1"),
     ("int", "P2")),
    "T + set * (NT * NIN), TT + set * NT, A + set * NT, S + set * NIN, SH + set * NIN, D1, P2")


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
    T: np.ndarray      # [NB, NT, NIN]
    a: np.ndarray      # [NB, NT]
    s: np.ndarray      # [NB, NIN]
    t: np.ndarray      # [NB, NIN]
    d1: List[int]
    pairs: List[Tuple[int, int]]

    @property
    def TT(self) -> np.ndarray:   # [NB, NT], as symbolic.RBFNetwork builds ANN<id>_TT
        return -0.5 * np.sum(self.T * self.T, axis=2)

    @property
    def P2(self) -> np.ndarray:   # [ND2, 2], as runtime/codegen.py builds ANN<id>_P2<kind>
        return np.asarray(self.pairs, dtype=np.int32).reshape(-1, 2)


def exponents(inp: Inputs, s: int) -> np.ndarray:
    """-1/2 |z - T_j|^2 of set s, [R, NT] (fp64, direct differences)."""
    z = inp.X[s] * inp.s[s] + inp.t[s]
    d = z[:, None, :] - inp.T[s][None, :, :]
    return -0.5 * np.sum(d * d, axis=2)


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> Inputs:
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    T = rng.normal(0.0, 1.0, (c.NT, c.NIN))
    a = rng.normal(0.0, 1.0, c.NT)
    s = rng.uniform(0.3, 3.0, c.NIN)
    t = rng.normal(0.0, 1.0, c.NIN)
    # one-hot: no row on the hot point of set 1 (NT - 1).  There every direct-difference term of
    # an off-diagonal Hessian entry is exactly 0, so S = 0, while the moment form of the kernel
    # and of RBFNetwork.evaluate (four rounded terms that cancel) cannot return an exact 0.
    rows = np.arange(c.R) % (c.NT - 1 if c.onehot else c.NT)
    u = rng.normal(size=(c.R, c.NIN))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    z_in = T[rng.integers(0, c.NT, c.R)] + rng.normal(0.0, 0.5, (c.R, c.NIN))

    def smallest(lam):   # smallest exponent with every row moved lam along its direction
        d = (lam * u)[:, None, :] - T[None, :, :]
        return float((-0.5 * np.sum(d * d, axis=2)).min())

    lo, hi = 0.0, 100.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if smallest(mid) > FAR_EXPONENT else (lo, mid)
    X = np.stack([(z_in - t) / s, T[rows], (hi * u - t) / s, (100.0 * u - t) / s])
    S = np.stack([s, np.ones(c.NIN), s, s])
    SH = np.stack([t, np.zeros(c.NIN), t, t])
    A = np.stack([a] * NB)
    if c.onehot:
        A = np.zeros((NB, c.NT))
        A[[0, 2], 0] = 1.5
        A[[1, 3], c.NT - 1] = -2.5
    return Inputs(X, np.stack([T] * NB), A, S, SH, c.d1(), c.pairs())


# ---------------------------------------------------------------------------
# the reference (mpmath)
# ---------------------------------------------------------------------------

@dataclasses.dataclass
class Reference:
    """Per checked input set: value/scale pairs as object arrays of mpf."""
    V: list
    G: list
    H: list


@functools.lru_cache(maxsize=None)
def reference(name: str) -> Reference:
    c, inp = BY_NAME[name], inputs(name)
    out = Reference([], [], [])
    absf = np.frompyfunc(abs, 1, 1)
    mexp = np.frompyfunc(mp.exp, 1, 1)
    with mp.workdps(DPS):
        for k in CHECKED:
            X, T, a, s, t = _m(inp.X[k]), _m(inp.T[k]), _m(inp.a[k]), _m(inp.s[k]), _m(inp.t[k])
            z = X * s + t
            d = z[:, None, :] - T[None, :, :]                      # [R, NT, NIN]
            e = mexp((d * d).sum(axis=2) * mp.mpf(-0.5))           # [R, NT]
            w, aw = e * a, e * absf(a)
            out.V.append((w.sum(axis=1), aw.sum(axis=1)))
            if c.ND1:
                dd = d[:, :, inp.d1]                                # [R, NT, ND1]
                sd = s[inp.d1]
                out.G.append((-(w[:, :, None] * dd).sum(axis=1) * sd, (aw[:, :, None] * absf(dd)).sum(axis=1) * absf(sd)))
            else:
                out.G.append(None)
            if c.ND2:
                hv, hs = [], []
                for (i, j) in inp.pairs:
                    dij = d[:, :, i] * d[:, :, j]
                    delta = 1 if i == j else 0
                    hv.append((w * (dij - delta)).sum(axis=1) * (s[i] * s[j]))
                    hs.append((aw * (absf(dij) + delta)).sum(axis=1) * abs(s[i] * s[j]))
                out.H.append((np.stack(hv, axis=1), np.stack(hs, axis=1)))
            else:
                out.H.append(None)
    return out


def numpy_outputs(name: str, s: int):
    """(V, G[:, d1], H[:, pairs]) of ``symbolic.RBFNetwork.evaluate`` (plain fp64) on input set s."""
    from agentlib_mpc_amd import symbolic as sx

    c, inp = BY_NAME[name], inputs(name)
    v, g, h = sx.RBFNetwork(inp.T[s], inp.a[s], inp.s[s], inp.t[s]).evaluate(inp.X[s])
    G = g[:, inp.d1] if c.ND1 else None
    Hh = np.stack([h[:, a, b] for a, b in inp.pairs], axis=1) if c.ND2 else None
    return (v if c.WV else None), G, Hh


def errors_of(name: str, outputs) -> dict:
    """{"V" | "G" | "H": scaled error, max over the checked input sets}; ``outputs(s) -> (V, G, H)``."""
    return core.errors_of(reference(name), outputs, CHECKED)


if __name__ == "__main__":   # prints the content of tests/golden/rbf_eval_fp64_error.json
    import sys

    core.print_fp64_errors(sys.modules[__name__])
