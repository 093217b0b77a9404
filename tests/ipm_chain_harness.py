"""Device unit harness of the IPM kernel's state chain (csrc/mpcx_ipm.hip: ``chain_factor`` +
``chain_solve``, ``chain_factor_tw`` + ``chain_solve_tw``) and of its filter lists
(``filter_insert``, ``spill_prune``, ``spill_shift``, ``spill_dominates``), support code of
tests/test_ipm_chain.py and tests/test_ipm_filter.py.  Built on tests/ipm_linalg_harness.py (its
launcher, ``_compile``, ``scaled_error``, ``bound``, ``mp_solve``, ``Module``).

Wrapper kernels are appended to a structure's generated model source inside ``namespace
mpcx_kernel``, one code object per structure and horizon; one wavefront per workgroup, one
problem per workgroup.

The chain wrapper fills the whole ``LdsRest`` part of ``gL`` with a byte pattern, stages ``S``,
``fixm`` and ``zx`` from global memory, fills ``Dinv``, ``xs``, ``C``, ``CW``, ``CY`` with NaN and
poisons ``cperm`` / ``cpiv``, calls the factor and the solve of the one-sided (``which`` 0) or of
the twisted order (``which`` 1) and copies all of ``LdsRest`` back: every byte outside the seven
output fields must come back as it went in.  What the restatement never reads (the x part of stage
0 in ``zx``, stage 0's S00 and S10) holds NaN, so a read of it shows in the outputs.

Chains: tests/test_chain_twisted.py ``make_chain`` (blocks) in the kernel's layout; scalar chains
from (a_j, s_j) with b_j = s_j^2.  Classes of block chains: ``random``; ``fixed`` (fixed states; a
fixed state strands multiplier rows of its boundary -- always singular in the first boundary where
NMU = NX -- so every boundary's multiplier block holds -delta I, the inertia correction's delta_c
term that the kernel itself adds to every multiplier row when a chain is singular; with it the
states' block of a pivot's inverse, which the forward recurrence multiplies the couplings with and
which is exactly zero where NMU = NX and the multiplier block is zero, is not zero);
``scaled`` and ``extreme``: a random
chain T0 under the congruence D T0 D, D a power of two per state (exact in fp64), so that the state
diagonals are multiplied by 4^e (1e-6 .. 1e6; 1e+-18 in the patterns all large, all small, and
large or small from one boundary to the next.  Mixing 1e+-18 state by state inside a boundary makes
the entries of one pivot block span 1e36, more than 1 / eps^2: the fp64 restatement's own error is
then ~1e-8 and differs by up to 8.1 times between its two orders on one and the same chain
(one_room_du, N = 5), so no implementation can be held to FACTOR times one of them).
The chains mixed from boundary to boundary hold -delta I on every multiplier block as the fixed
class does: where NMU = NX and the multiplier block is zero, the states' block of a pivot's inverse
is exactly zero, the fp64 result is its rounding residue, and a step from a large boundary to a
small one multiplies that residue by the ratio of the two scalings -- a scaled error of 1e-10 ...
8e-9 on those chains alone, next to 1e-16 on all others, that says nothing about the routine (two
correct implementations differ by more than FACTOR in it).  With delta every block of every pivot's
inverse is a number with a relative error, and the class is held to a unit of 1e-16 ... 1e-15.
A chain whose state diagonals alone are scaled has eigenvalues of the order of the diagonals next
to those of the multiplier rows' Schur complement, their reciprocals: it cannot be separated at any
cap.  The congruence keeps the inertia (Sylvester), so the separation condition and the eigenvalue
inertia are taken from T0, the solution from the scaled chain itself.  ``zero``: one chain block
and its couplings exactly zero.  Every block chain is ``make_chain``'s with ``CONTINUITY`` times
the identity added to the coupling of the multipliers mu_j with their own states x_{j+1} (a
continuity row x_{j+1} - f(x_j, u_j) = 0 has that identity): ``make_chain``'s purely random
coupling leaves more than half of the chains of 15 boundaries closer to singular than SEPARATION,
and single pivots with inverses of 1e3 ... 1e4, on which the fp64 restatement's own error is a
matter of luck (1e-16 on one chain, 1e-13 on the next): no unit for a factor of 8.

Reference: mpmath at ``DPS`` digits -- the solution from a solve of the assembled matrix, the pivot
inverses from the pivot recurrences of either order, the inertia from the eigenvalues of the
assembled matrix (every chain of a non-zero class is separated: min |ev| >= SEPARATION max |ev|).
The unit of the tolerance is the scaled error of the fp64 host restatement (``twisted``,
``one_sided``, ``serial_restart``) on the same chains, tests/golden/ipm_chain_fp64_error.json
(regenerate: ``python -m tests.ipm_chain_harness``).

After a counted zero pivot the callers discard the solve (tests/ipm_linalg_harness.py), so the
zero classes pin the inertia and ``Dinv`` only; the ``MPCX_CHAIN_BK`` build's ``bk_inverse``
divides by the zero pivot, so there the inertia is pinned where the zero block is the last one.
"""

from __future__ import annotations

import dataclasses
import functools
import json
import math
import os
import pathlib
from typing import Dict, List, Optional, Sequence, Tuple

import mpmath as mp
import numpy as np

from agentlib_mpc_amd import benchmarks as bm
from agentlib_mpc_amd.runtime import native
from tests import configs
from tests.eval_harness_core import DPS, ROOT, name_seed, upload
from tests.ipm_linalg_harness import (IPOISON, SEPARATION, Module, _compile, _mp_rows, _to_obj, bound,  # noqa: F401
                                      mp_solve, nmu_of, scaled_error)
from tests.test_chain_scan import accepted, scan
from tests.test_chain_sweep import ZERO_PIVOT
from tests.test_chain_twisted import block, full_matrix, make_chain, one_sided, twisted

FILL = 0xA5               # the byte pattern of LdsRest (as a double: finite)
SLAB_SENTINEL = -3.0e88   # the workspace slab of the filter wrapper
SMALL = 20                # N * NC up to this: NCHAIN chains per class, else NCHAIN_LARGE
NCHAIN = 16
NCHAIN_LARGE = 4
MAX_DRAWS = 400
DELTA_C = 0.5             # the fixed class, the mixed extreme chains: -delta I on every boundary's multiplier block
CONTINUITY = 6.0          # added to the multiplier rows' coupling with their own states
MARGIN = 100.0            # scalar chains: distance (as a factor) from the thresholds of the scan's ok rule

BLOCK_CLASSES = ("random", "fixed", "scaled", "extreme", "zero")
SCALAR_CLASSES = ("dominant", "indefinite", "near_singular", "overflow", "fixed", "zero")
ORDERS = ("one_sided", "twisted")


@dataclasses.dataclass(frozen=True)
class ChainConfig:
    case: str
    N: int
    defines: Tuple[str, ...] = ()
    asserts: str = "true"

    @property
    def name(self) -> str:
        return f"{self.case}_N{self.N}" + ("_" + "_".join(d.lower().replace("mpcx_", "").replace("=", "") for d in self.defines)
                                           if self.defines else "")


_SCALAR = "NX == 1 && NMU == 0 && !CHAIN_TW"
_DU = "NX == 2 && NMU == 2 && NC == 4"
_MHE = "NX == 3 && NMU == 3 && NC == 6 && 2 * NC * NC > WAVE && CHAIN_TW"
CHAIN_CONFIGS = (
    *(ChainConfig("one_room", n, asserts=_SCALAR) for n in (1, 2, 4, 15, 16, 17)),
    *(ChainConfig("one_room_du", n, asserts=_DU + " && CHAIN_TW") for n in (1, 2, 3, 4, 5, 15)),
    *(ChainConfig("one_room_du", n, ("MPCX_CHAIN_BK",), _DU + " && !CHAIN_TW") for n in (2, 5)),
    *(ChainConfig("mhe_room", n, asserts=_MHE) for n in (2, 15)),
)
CHAIN_BY_NAME = {c.name: c for c in CHAIN_CONFIGS}

#: the filter builds: the shipped parts, the two of tests/test_gpu_ipm.py and one without a spill list
FILTER_BUILDS = {
    "shipped": (),
    "spill": tuple(bm.FILTER_TEST_BUILDS["spill"][0].split(",")),
    "capped": tuple(bm.FILTER_TEST_BUILDS["capped"][0].split(",")),
    "nospill": ("MPCX_MAXF=8", "MPCX_FSPILL=0"),
}
FILTER_PARTS = {"shipped": (48, 976), "spill": (8, 1016), "capped": (8, 4), "nospill": (8, 0)}
FILTER_CASE = "one_room"


@functools.lru_cache(maxsize=None)
def gen_of(case: str, N: Optional[int]):
    return configs.CASES[case](**({} if N is None else {"N": N})).backend.problem.gen


@dataclasses.dataclass(frozen=True)
class CDims:
    N: int
    NX: int
    NMU: int
    LX1: int

    @property
    def NC(self) -> int:
        return self.NX + self.NMU

    @property
    def SOFF(self) -> int:
        return self.NX * self.NX + self.NC * self.NC + self.NC * self.NX

    @property
    def scalar(self) -> bool:
        return self.NX == 1 and self.NMU == 0

    @property
    def CMID(self) -> int:
        return self.N // 2


@functools.lru_cache(maxsize=None)
def cdims(c: ChainConfig) -> CDims:
    g = gen_of(c.case, c.N)
    d = g.dims
    assert d["N"] == c.N
    return CDims(N=c.N, NX=d["NX"], NMU=nmu_of(g), LX1=d["NV"] + d["NG"] + d["NX"])


def nchain(d: CDims, cls: str = "") -> int:
    return NCHAIN if d.N * d.NC <= SMALL else NCHAIN_LARGE


def orders_of(c: ChainConfig) -> Tuple[str, ...]:
    if cdims(c).scalar:
        return ("serial",)
    return ("one_sided",) if c.defines else ORDERS


# ---------------------------------------------------------------------------
# the chains
# ---------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True, eq=False)
class Chain:
    cls: str
    S11: tuple
    S00: tuple
    S10: tuple
    fix: dict                     # boundary -> set of fixed states
    rhs: tuple                    # per boundary, fp64: what the kernel's rhs(j, r) evaluates to
    zx: np.ndarray                # [N * (NX + NC)] the split right-hand side, NaN where never read
    inertia: Optional[Tuple[int, int, int]]   # from the eigenvalues; zero classes: of the rest plus the zeros
    zero: Tuple[int, ...] = ()    # zero class: the zero blocks / lanes
    path: str = ""                # scalar chains: "scan" or "serial", what the class is meant to take


def _separated(T: np.ndarray) -> bool:
    if T.size == 0:
        return True
    ev = np.linalg.eigvalsh(T / np.abs(T).max()) if np.abs(T).max() > 0 else np.zeros(1)
    return bool(np.abs(ev).min() >= SEPARATION * np.abs(ev).max() and np.abs(ev).max() > 0)


def _ev_inertia(T: np.ndarray) -> Tuple[int, int]:
    if T.size == 0:
        return 0, 0
    ev = np.linalg.eigvalsh(T / np.abs(T).max())
    return int((ev > 0).sum()), int((ev < 0).sum())


def _split_rhs(rng, d: CDims, fix) -> Tuple[tuple, np.ndarray]:
    """zx with every entry of the right-hand side split over the two places the kernel adds up;
    fixed entries sum to exactly 0; the x part of stage 0 (never read) NaN."""
    N, NX, NC, XO = d.N, d.NX, d.NC, d.NMU
    ZS = NX + NC
    zx = rng.normal(size=N * ZS)
    zx[:NX] = np.nan
    rhs = []
    for j in range(N):
        r = np.zeros(NC)
        for q in range(NC):
            two = j + 1 < N and q >= XO
            if q >= XO and (q - XO) in fix[j]:
                if two:
                    zx[j * ZS + NX + q] = -zx[(j + 1) * ZS + (q - XO)]
                else:
                    zx[j * ZS + NX + q] = 0.0
            r[q] = zx[j * ZS + NX + q] + (zx[(j + 1) * ZS + (q - XO)] if two else 0.0)
        rhs.append(r)
    return tuple(rhs), zx


def _congruence(S11, S00, S10, e: np.ndarray, d: CDims):
    """D T D with D = 2^e[j, i] on state i of boundary j, exact in fp64."""
    NMU = d.NMU
    f = np.ldexp(1.0, e)
    for j in range(d.N):
        S11[j][NMU:, :] *= f[j][:, None]
        S11[j][:, NMU:] *= f[j][None, :]
        if j + 1 < d.N:
            S00[j + 1] *= f[j][:, None] * f[j][None, :]
        if j > 0:
            S10[j][NMU:, :] *= f[j][:, None]
            S10[j] *= f[j - 1][None, :]


def _draw_block(cls: str, m: int, d: CDims, rng):
    """-> (S11, S00, S10, fix, T0 whose eigenvalues decide separation and inertia, zero blocks)."""
    N, NX, NMU, NC = d.N, d.NX, d.NMU, d.NC
    fixed = []
    if cls == "fixed":
        where = (0, d.CMID, N - 1, (m // 4) % N)[m % 4]
        fixed = [(where, i) for i in range(NX)] if m % 4 == 3 else [(where, int(rng.integers(NX)))]
    S11, S00, S10, fix = make_chain(rng, N, NX, NMU, fixed)
    for a in S11:   # the continuity rows' own identity (mu_j against x_{j+1}); see the module docstring
        k = min(NMU, NX)
        a[:k, NMU:NMU + k] += CONTINUITY * np.eye(k)
        a[NMU:NMU + k, :k] += CONTINUITY * np.eye(k)
    if cls == "fixed" or (cls == "extreme" and m % 3 == 2):
        for a in S11:
            a[:NMU, :NMU] = -DELTA_C * np.eye(NMU)
    zero = ()
    if cls == "zero":
        z = (0, d.CMID, N - 1)[m % 3]
        S11[z][:] = 0.0
        if z + 1 < N:
            S00[z + 1][:] = 0.0
            S10[z + 1][:] = 0.0
        if z > 0:
            S10[z][:] = 0.0
        zero = (z,)
    T0 = full_matrix(S11, S00, S10, fix, NX, NMU)
    if zero:
        keep = [i for i in range(N * NC) if i // NC != zero[0]]
        T0 = T0[np.ix_(keep, keep)]
    if cls in ("scaled", "extreme"):
        if cls == "scaled":     # 4^e in 1e-6 .. 1e6
            e = rng.integers(-10, 11, (N, NX))
        else:                   # 4^e ~ 1e+-18: all large, all small, mixed from boundary to boundary
            e = (np.full((N, NX), 30), np.full((N, NX), -30), np.repeat(rng.choice([-30, 30], (N, 1)), NX, axis=1))[m % 3]
        _congruence(S11, S00, S10, e, d)
    return S11, S00, S10, fix, T0, zero


@functools.lru_cache(maxsize=None)
def block_chains(c: ChainConfig):
    """-> (chains class-major, {class: (kept, rejected)})."""
    d = cdims(c)
    out, counts = [], {}
    for cls in BLOCK_CLASSES:
        rng = np.random.default_rng(name_seed(f"ipm_chain {c.case} {c.N} {cls}"))
        kept = rejected = 0
        m = 0
        while kept < nchain(d, cls):
            assert kept + rejected < MAX_DRAWS, (c.name, cls)
            S11, S00, S10, fix, T0, zero = _draw_block(cls, m, d, rng)
            if not _separated(T0):
                rejected += 1
                continue
            pos, neg = _ev_inertia(T0)
            rhs, zx = _split_rhs(rng, d, fix)
            out.append(Chain(cls, tuple(S11), tuple(S00), tuple(S10), fix, rhs, zx,
                             (pos, neg, d.NC * len(zero)), zero))
            kept += 1
            m += 1
        counts[cls] = (kept, rejected)
    return tuple(out), counts


# ---- scalar chains ---------------------------------------------------------------------------

def serial_restart(a, b):
    """The serial recurrence of ``chain_factor`` with its zero-pivot rule (tests/test_chain_scan.py
    ``serial`` without a zero pivot): -> (1 / d_j, 0 at a zero pivot; (pos, neg, zero))."""
    r, dprev = np.zeros(len(a)), 0.0
    pos = neg = nz = 0
    for j in range(len(a)):
        dj = a[j] - b[j] * dprev
        if abs(dj) <= ZERO_PIVOT:
            nz += 1
            dprev = 0.0
        else:
            pos, neg = pos + (dj > 0), neg + (dj < 0)
            dprev = 1.0 / dj
        r[j] = dprev
    return r, (int(pos), int(neg), int(nz))


def scalar_ab(ch: Chain):
    """The (a_j, b_j) the kernel gathers from a scalar chain (a fixed lane: 1, 0)."""
    N = len(ch.S11)
    a = np.array([1.0 if ch.fix[j] else float(block(ch.S11, ch.S00, ch.fix, j, 1, 0)[0, 0]) for j in range(N)])
    b = np.array([0.0 if (j == 0 or ch.fix[j]) else float(ch.S10[j][0, 0]) ** 2 for j in range(N)])
    return a, b


def scan_margin(a, b):
    """How the scan's result stands against the kernel's ok rule: (accepted, factor by which the
    nearest test is met or, when rejected, by which the worst one is missed)."""
    n = len(a)
    if n > 16:
        return False, math.inf          # no scan above one DPP row
    with np.errstate(all="ignore"):
        dq = scan(a, b)
        ok = accepted(a, b, dq)
        r = 1.0 / dq
        rprev = np.concatenate([[0.0], r[:-1]])
        num, den = np.abs(dq - (a - b * rprev)), 1e-12 * (np.abs(a) + np.abs(b * rprev))
        resid = np.where(num <= den, np.where(num > 0, num / np.where(den > 0, den, 1.0), 0.0),
                         np.where(den > 0, num / np.where(den > 0, den, 1.0), math.inf))
        resid = np.where(np.isnan(num) | np.isnan(den), math.inf, resid)
        mag = np.minimum(np.abs(dq) / (1e-8 * np.fmax(np.abs(a), 1e-300)), np.abs(dq) / ZERO_PIVOT)
    if not np.isfinite(dq).all():
        return False, math.inf
    if ok:
        return True, float(min(1.0 / max(resid.max(), 1e-300), mag.min()))
    return False, float(max(resid.max(), 1.0 / max(mag.min(), 1e-300)))


def _scalar_chain(cls, a, s, fixed_lanes, d: CDims, rng, zero=(), path=""):
    """The kernel's layout of a scalar chain: a_j = S11(j) + S00(j + 1) (halves: exact), S10(j) = s_j."""
    N = d.N
    S11 = [np.array([[a[j] * (0.5 if j + 1 < N else 1.0)]]) for j in range(N)]
    S00 = [None] + [np.array([[a[j - 1] * 0.5]]) for j in range(1, N)]
    S10 = [None] + [np.array([[s[j]]]) for j in range(1, N)]
    fix = {j: set() for j in range(N)}
    for j in fixed_lanes:
        fix[j].add(0)
        S11[j][0, 0] = 7.0           # a fixed lane's own entries are not read
        if j + 1 < N:
            S10[j + 1][0, 0] = 0.0
        if j > 0:
            S10[j][0, 0] = 0.0
    rhs, zx = _split_rhs(rng, d, fix)
    return Chain(cls, tuple(S11), tuple(S00), tuple(S10), fix, rhs, zx, None, tuple(zero), path)


def _draw_scalar(cls: str, m: int, d: CDims, rng) -> Chain:
    n = d.N
    fixed, zero, path = (), (), "scan" if n <= 16 else "serial"
    if cls in ("dominant", "indefinite", "overflow", "fixed"):
        scale = 10.0 ** rng.uniform(-2.5, 2.5, n)
        s = np.concatenate([[0.0], np.sqrt(rng.uniform(0.0, 1.0, n - 1) * scale[1:] * scale[:-1])])
        a = scale * rng.uniform(1.05, 3.0, n) + np.concatenate([s[1:], [0.0]]) + s
        if cls == "indefinite" or (cls in ("overflow", "fixed") and m % 2 == 1):
            flip = rng.uniform(size=n) < 0.4
            flip[rng.integers(n)] = True
            a[flip] *= -1.0
        if cls == "overflow" and m % 2 == 0:
            # restoration penalties: products of 16 entries of 1e20 overflow without the rescaling, the scan stands
            a, s = a * 1e20, s * 1e20
        elif cls == "overflow":
            # entries of 1e150: a_2 b_1 overflows inside one product whatever the rescaling, from three
            # lanes on the scan's result is not finite and the recurrence runs
            a, s = a * 1e150, s * 1e150
            path = "serial" if n >= 3 else path
        if cls == "fixed":
            fixed = sorted({(0, n // 2, n - 1)[m % 3], int(rng.integers(n))} if m % 2 else {(0, n // 2, n - 1)[m % 3]})
    elif cls == "near_singular" and n <= 2:
        # no leading minor but the matrix itself (n = 2: a small last pivot is a singular matrix)
        return dataclasses.replace(_draw_scalar("indefinite", m, d, rng), cls=cls)
    elif cls == "near_singular":
        # every third leading minor nearly singular: its pivot is ~1e-11 (even members; the scan's ok
        # rule asks for 1e-8) or ~1e-7 (odd members; the scan's next pivot then misses the recurrence
        # check) of its diagonal, the next pivot is its large reciprocal and the one after is ordinary
        # again, so the matrix itself stays well conditioned.  tests/test_chain_scan.py builds every
        # pivot small: such a matrix is singular to working precision, outside the inertia set, and
        # neither the recurrence nor the scan has an accurate answer to be held to
        path = "serial"
        a = rng.uniform(1.0, 3.0, n)
        s = np.concatenate([[0.0], rng.uniform(0.3, 1.0, n - 1)])
        dj = a[0] = a[0] * rng.choice([-1.0, 1.0])
        for j in range(1, n):
            if j % 3 == 1 and j + 1 < n:
                a[j] = math.copysign(a[j], dj)        # b_j = s_j^2 > 0 cancels a_j only with the sign of d_{j-1}
                lo = (-11.5, -7.0)[m % 2 if n >= 15 else 0]     # (a short scan's error stays inside the check)
                # odd members: above the 1e-8 rule, rejected by the recurrence check alone
                target = a[j] * 10.0 ** rng.uniform(lo, lo + (1.0 if lo < -10 else 0.5)) * rng.choice([-1.0, 1.0])
                s[j] = math.sqrt((a[j] - target) * dj)
            else:
                a[j] *= rng.choice([-1.0, 1.0])
            dj = a[j] - s[j] * s[j] / dj
    else:                         # zero: exact zero pivots from powers of two
        path = "serial"
        z = (0, n - 1, n // 2)[m % 3]
        if m % 4 == 3:            # every pivot below the absolute threshold ZERO_PIVOT: entries of 1e-150
            a = rng.uniform(1.0, 3.0, n) * 1e-150 * rng.choice([-1.0, 1.0], n)
            s = np.concatenate([[0.0], rng.uniform(0.1, 1.0, n - 1) * 1e-150])
            return _scalar_chain(cls, a, s, fixed, d, rng, tuple(range(n)), path)
        a, s = np.zeros(n), np.zeros(n)
        dprev = 0.0
        for j in range(n):
            s[j] = 0.0 if j == 0 else float(np.ldexp(1.0, int(rng.integers(-3, 4))))
            dj = 0.0 if j == z else float(rng.choice([-1.0, 1.0]) * np.ldexp(1.0, int(rng.integers(-4, 5))))
            a[j] = dj + (s[j] * s[j] / dprev if dprev != 0.0 else 0.0)
            dprev = dj
        zero = (z,)
    return _scalar_chain(cls, a, s, fixed, d, rng, zero, path)


@functools.lru_cache(maxsize=None)
def scalar_chains(c: ChainConfig):
    d = cdims(c)
    out, counts = [], {}
    for cls in SCALAR_CLASSES:
        rng = np.random.default_rng(name_seed(f"ipm_chain {c.case} {c.N} {cls}"))
        kept = rejected = 0
        while kept < nchain(d, cls):
            assert kept + rejected < MAX_DRAWS, (c.name, cls)
            ch = _draw_scalar(cls, kept, d, rng)
            a, b = scalar_ab(ch)
            T = full_matrix(ch.S11, ch.S00, ch.S10, ch.fix, 1, 0)
            took, margin = scan_margin(a, b)
            want = ch.path
            good = (took == (want == "scan")) and margin >= MARGIN
            if cls == "zero":
                keep = [j for j in range(d.N) if j not in ch.zero]
                rest = T[np.ix_(keep, keep)]
                # lanes either side of an inner zero pivot stay coupled in the matrix; the restarted
                # recurrence is the contract, its inertia the restatement's (not an eigenvalue inertia)
                inertia = serial_restart(a, b)[1]
                good = good and (len(ch.zero) == d.N or inertia[2] == 1) and (not keep or np.isfinite(rest).all())
            else:
                good = good and _separated(T)
                pos, neg = _ev_inertia(T)
                inertia = (pos, neg, 0)
            if not good:
                rejected += 1
                continue
            out.append(dataclasses.replace(ch, inertia=inertia, path=want))
            kept += 1
        counts[cls] = (kept, rejected)
    return tuple(out), counts


def chains(c: ChainConfig):
    return scalar_chains(c) if cdims(c).scalar else block_chains(c)


# ---------------------------------------------------------------------------
# the kernel's layout
# ---------------------------------------------------------------------------

def lay_out(c: ChainConfig, chs: Sequence[Chain], rng):
    """-> (S [nb, N * SOFF], fixm [nb, N] int64, zx [nb, N * (NX + NC)])."""
    d = cdims(c)
    NXX, NCC = d.NX * d.NX, d.NC * d.NC
    S = np.full((len(chs), d.N, d.SOFF), np.nan)       # stage 0's S00 and S10 are never read
    fixm = np.zeros((len(chs), d.N), dtype=np.uint64)
    for q, ch in enumerate(chs):
        for j in range(d.N):
            if j > 0:
                S[q, j, :NXX] = ch.S00[j].ravel()
                S[q, j, NXX + NCC:] = ch.S10[j].ravel()
            S[q, j, NXX:NXX + NCC] = ch.S11[j].ravel()
            bits = int(rng.integers(0, 1 << 62)) & ((1 << d.LX1) - 1)   # other variables' bits: not the chain's
            for i in ch.fix[j]:
                bits |= 1 << (d.LX1 + i)
            fixm[q, j] = bits
    return S.reshape(len(chs), -1), fixm.view(np.int64), np.stack([ch.zx for ch in chs])


# ---------------------------------------------------------------------------
# mpmath reference
# ---------------------------------------------------------------------------

def _mpm(A) -> np.ndarray:
    A = np.asarray(A, dtype=float)
    return _to_obj(_mp_rows(A), A.shape)


def _mp_inv(C: np.ndarray) -> np.ndarray:
    """Inverse of an object array of mpf; an all-zero block: 0 (the sweep's contract)."""
    n = len(C)
    if all(v == 0 for v in C.ravel()):
        return _mpm(np.zeros((n, n)))
    rows = [[v for v in row] for row in C]
    M = [rows[i] + [mp.mpf(1 if i == j else 0) for j in range(n)] for i in range(n)]
    for k in range(n):
        p = max(range(k, n), key=lambda i: abs(M[i][k]))
        M[k], M[p] = M[p], M[k]
        piv = M[k][k]
        Mk = M[k] = [v / piv for v in M[k]]
        for i in range(n):
            f = M[i][k]
            if i != k and f != 0:
                M[i] = [x - f * y for x, y in zip(M[i], Mk)]
    return _to_obj([row[n:] for row in M], (n, n))


def _mp_block(ch: Chain, j: int, NX: int, NMU: int) -> np.ndarray:
    return _mpm(block(ch.S11, ch.S00, ch.fix, j, NX, NMU))


def _mp_override(C: np.ndarray, fix_j, NMU: int) -> np.ndarray:
    for i in fix_j:
        C[NMU + i, :] = mp.mpf(0)
        C[:, NMU + i] = mp.mpf(0)
        C[NMU + i, NMU + i] = mp.mpf(1)
    return C


def mp_pivot_inverses(ch: Chain, d: CDims, order: str) -> Tuple[np.ndarray, ...]:
    """The inverses of the pivots of the one-sided order (D_j), of the twisted order (forward D_j
    below CMID, backward E_j above, the middle pivot with both contributions) or of the scalar
    recurrence with its zero-pivot rule, evaluated at DPS digits."""
    N, NX, NMU = d.N, d.NX, d.NMU
    with mp.workdps(DPS):
        inv: List[Optional[np.ndarray]] = [None] * N
        S10 = [None] + [_mpm(ch.S10[j]) for j in range(1, N)]

        def fwd(j):
            return S10[j].dot(inv[j - 1][NMU:, NMU:]).dot(S10[j].T)

        def bwd(j):
            return S10[j + 1].T.dot(inv[j + 1]).dot(S10[j + 1])

        if order == "serial":
            dprev = mp.mpf(0)
            for j in range(N):
                C = _mp_override(_mp_block(ch, j, NX, NMU), ch.fix[j], NMU)
                dj = C[0, 0] - (S10[j][0, 0] ** 2 * dprev if j > 0 and not ch.fix[j] else 0)
                dprev = mp.mpf(0) if abs(dj) <= ZERO_PIVOT else 1 / dj
                inv[j] = _to_obj([[dprev]], (1, 1))
            return tuple(inv)
        lo = d.CMID if order == "twisted" else N
        for j in range(lo):
            C = _mp_block(ch, j, NX, NMU)
            if j > 0:
                C = C - fwd(j)
            inv[j] = _mp_inv(_mp_override(C, ch.fix[j], NMU))
        for j in range(N - 1, lo, -1):
            C = _mp_block(ch, j, NX, NMU)
            if j + 1 < N:
                C[NMU:, NMU:] = C[NMU:, NMU:] - bwd(j)
            inv[j] = _mp_inv(_mp_override(C, ch.fix[j], NMU))
        if lo < N:
            C = _mp_block(ch, lo, NX, NMU)
            if lo > 0:
                C = C - fwd(lo)
            if lo + 1 < N:
                C[NMU:, NMU:] = C[NMU:, NMU:] - bwd(lo)
            inv[lo] = _mp_inv(_mp_override(C, ch.fix[lo], NMU))
        return tuple(inv)


def mp_solution(ch: Chain, d: CDims) -> np.ndarray:
    T = full_matrix(ch.S11, ch.S00, ch.S10, ch.fix, d.NX, d.NMU)
    b = np.concatenate(ch.rhs)
    return _to_obj(mp_solve(T, b[:, None]), (len(b), 1))


@functools.lru_cache(maxsize=None)
def refs(c: ChainConfig):
    """Per chain: (solution or None for a zero class, {order: pivot inverses})."""
    d = cdims(c)
    out = []
    for ch in chains(c)[0]:
        sol = None if ch.zero else mp_solution(ch, d)
        out.append((sol, {o: mp_pivot_inverses(ch, d, o) for o in orders_of(c)}))
    return tuple(out)


def errors(c: ChainConfig, idx: int, order: str, xs: Optional[np.ndarray], dinv: np.ndarray) -> Dict[str, float]:
    """Scaled errors of one chain's results: ``xs`` [N * NC] (None: not pinned), ``dinv`` [N, NC, NC]
    (the worst slot)."""
    d = cdims(c)
    sol, inv = refs(c)[idx]
    out = {"dinv": max(scaled_error(dinv[j], inv[order][j]) for j in range(d.N))}
    if xs is not None and sol is not None:
        out["xs"] = scaled_error(np.asarray(xs, float).reshape(-1, 1), sol)
    return out


# ---------------------------------------------------------------------------
# fp64 host restatements and the tolerance unit
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def restated(c: ChainConfig):
    """Per chain: {order: (xs, Dinv [N, NC, NC], inertia)} of the fp64 host restatement."""
    d = cdims(c)
    out = []
    for ch in chains(c)[0]:
        per = {}
        for o in orders_of(c):
            with np.errstate(all="ignore"):
                if o == "serial":
                    a, b = scalar_ab(ch)
                    r, inertia = serial_restart(a, b)
                    # chain_solve: y_j = c_j - s_j r_{j-1} y_{j-1}, x_j = r_j (y_j - s_{j+1} x_{j+1})
                    s = [0.0] + [float(ch.S10[j][0, 0]) for j in range(1, d.N)]
                    y, x = np.zeros(d.N), np.zeros(d.N)
                    for j in range(d.N):
                        y[j] = ch.rhs[j][0] - (s[j] * r[j - 1] * y[j - 1] if j > 0 else 0.0)
                    for j in range(d.N - 1, -1, -1):
                        x[j] = r[j] * (y[j] - (s[j + 1] * x[j + 1] if j + 1 < d.N else 0.0))
                    per[o] = (x, r.reshape(d.N, 1, 1), inertia)
                    continue
                keep: dict = {}
                fn = twisted if o == "twisted" else one_sided
                x, inertia = fn(list(ch.S11), list(ch.S00), list(ch.S10), ch.fix, d.NX, d.NMU, list(ch.rhs), keep)
                per[o] = (x, np.stack(keep["Dinv"]), tuple(int(v) for v in inertia))
        out.append(per)
    return tuple(out)


def fp64_errors(names: Optional[Sequence[str]] = None) -> dict:
    """Per configuration, order and class: the largest scaled errors of the restatement."""
    out: dict = {}
    for c in CHAIN_CONFIGS:
        if names is not None and c.name not in names:
            continue
        per: dict = {}
        for idx, (ch, rs) in enumerate(zip(chains(c)[0], restated(c))):
            for o, (x, dinv, _) in rs.items():
                e = errors(c, idx, o, None if ch.zero else x, dinv)
                slot = per.setdefault(o, {}).setdefault(ch.cls, {})
                for k, v in e.items():
                    slot[k] = max(slot.get(k, 0.0), v)
        out[c.name] = per
    return out


GOLDEN = os.path.join(ROOT, "tests", "golden", "ipm_chain_fp64_error.json")


@functools.lru_cache(maxsize=None)
def golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


# ---------------------------------------------------------------------------
# the HIP sources
# ---------------------------------------------------------------------------

FIELDS = ("S", "Dinv", "zx", "xs", "C", "CW", "CY", "fixm", "cperm", "cpiv", "fth", "fph")
OUTPUT_FIELDS = ("Dinv", "xs", "C", "CW", "CY", "cperm", "cpiv")
_SCALARS = ("N", "NX", "NMU", "NC", "SOFF", "LX1", "(int)CHAIN_TW", "CMID", "CSTEPS", "(int)sizeof(LdsRest)",
            "(int)WS_DOUBLES", "(int)O_FSP", "MAXF", "FSPILL")
CONST_NAMES = (*(s.replace("(int)", "").replace("sizeof(LdsRest)", "REST") for s in _SCALARS),
               *(f"off_{f}" for f in FIELDS), *(f"size_{f}" for f in FIELDS))
_CONST_EXPRS = (*_SCALARS, *(f"(int)__builtin_offsetof(LdsRest, {f})" for f in FIELDS),
                *(f"(int)sizeof(LdsRest::{f})" for f in FIELDS))

_HEAD = f"""
// generated by tests/ipm_chain_harness.py: wrapper kernels of the state chain and of the filter lists
namespace mpcx_kernel {{
static_assert(WS_DOUBLES < (1L << 31), "the constants are exported as int");
extern "C" __global__ void __launch_bounds__(64) ipmch_consts(int* __restrict__ out, int n) {{
  const int v[{len(_CONST_EXPRS)}] = {{{", ".join(_CONST_EXPRS)}}};
  if (threadIdx.x == 0 && blockIdx.x == 0)
    for (int i = 0; i < {len(_CONST_EXPRS)} && i < n; ++i) out[i] = v[i];
}}
"""

_CHAIN = f"""
// one chain per workgroup; which = 0: the one-sided order, 1: the twisted order
extern "C" __global__ void __launch_bounds__(64) ipmla_chain(const double* __restrict__ Sin, const unsigned long long* __restrict__ fixin,
                                                             const double* __restrict__ zxin, unsigned char* __restrict__ LdsBack,
                                                             int* __restrict__ res, int which) {{
  constexpr int RB_ = (int)sizeof(LdsRest), NZX = N * (NX + NCP);
  const int lane = threadIdx.x;
  const long b = blockIdx.x;
  unsigned char* rest = reinterpret_cast<unsigned char*>(static_cast<LdsRest*>(&gL));
  for (int i = lane; i < RB_; i += WAVE) rest[i] = {FILL};
  __syncthreads();
  for (int i = lane; i < N * SOFF; i += WAVE) gL.S[i] = Sin[b * (N * SOFF) + i];
  for (int i = lane; i < N; i += WAVE) gL.fixm[i] = fixin[b * N + i];
  for (int i = lane; i < NZX; i += WAVE) gL.zx[i] = zxin[b * NZX + i];
  for (int i = lane; i < N * NCC; i += WAVE) gL.Dinv[i] = __builtin_nan("");
  for (int i = lane; i < N * NC; i += WAVE) gL.xs[i] = __builtin_nan("");
  for (int i = lane; i < NCC; i += WAVE) {{ gL.C[i] = __builtin_nan(""); gL.CW[i] = __builtin_nan(""); gL.CY[i] = __builtin_nan(""); }}
  for (int i = lane; i < NCP; i += WAVE) {{ gL.cperm[i] = {IPOISON}; gL.cpiv[i] = {IPOISON}; }}
  __syncthreads();
  Agent a{{}};
  Inertia in{{-1, -1, -1}};
  int ran = 0;
  if (which == 0) {{
    in = chain_factor(a);
    chain_solve(a);
    ran = 1;
  }} else {{
    if constexpr (CHAIN_TW) {{
      in = chain_factor_tw(a);
      chain_solve_tw(a);
      ran = 1;
    }}
  }}
  __syncthreads();
  for (int i = lane; i < RB_; i += WAVE) LdsBack[b * RB_ + i] = rest[i];
  if (lane == 0) {{ int* r = res + 4 * b; r[0] = in.pos; r[1] = in.neg; r[2] = in.zero; r[3] = ran; }}
}}
"""

#: operations of the filter wrapper: ops[i] = (code, th, ph), code & 8: snapshot after it
OP_INSERT, OP_QUERY, OP_TIER, OP_SNAP = 0, 1, 2, 8

_FILTER = f"""
// one list of operations per workgroup on the filter of gL: ops [n_ops][3] = (code, th, ph), code & 7 =
// 0 insert, 1 query (the answer of spill_dominates goes to qout), 2 switch to tier (int)th -- the LDS
// part is set aside and comes back as resto_start / resto_return do through flt0, here in LDS of the
// wrapper's own, so that the slab outside the spill tiers is never written; code & 8: snapshot
// [2 MAXF | 4 FSPILL | nfilt, nsp0, nsp1, n_filt_over] after the operation
extern "C" __global__ void __launch_bounds__(64) ipmla_filter(const double* __restrict__ ops, double* __restrict__ slab,
                                                              double* __restrict__ snap, int* __restrict__ qout, int n_ops) {{
  constexpr int SNAP = 2 * MAXF + 4 * FSPILL + 4;
  __shared__ double keep[2 * MAXF];
  __shared__ int keep_n;
  const int lane = threadIdx.x;
  const long b = blockIdx.x;
  if (lane == 0) gL.ws_bits = (unsigned long long)(slab + b * WS_DOUBLES);
  __syncthreads();
  KState& K = gL.ks;
  K.nfilt = 0; K.nsp[0] = 0; K.nsp[1] = 0; K.n_filt_over = 0; K.resto = 0;
  for (int i = lane; i < MAXF; i += WAVE) {{ gL.fth[i] = {SLAB_SENTINEL!r}; gL.fph[i] = {SLAB_SENTINEL!r}; }}
  __syncthreads();
  int ns = 0;
  for (int i = 0; i < n_ops; ++i) {{
    const int code = (int)ops[3 * i];
    const double th = ops[3 * i + 1], ph = ops[3 * i + 2];
    if ((code & 7) == {OP_INSERT}) {{
      filter_insert(th, ph);
    }} else if ((code & 7) == {OP_QUERY}) {{
      const bool dom = spill_dominates(th, ph);
      if (lane == 0) qout[b * n_ops + i] = dom ? 1 : 0;
    }} else {{
      const int tier = (int)th;
      if (tier == 1) {{
        for (int j = lane; j < K.nfilt; j += WAVE) {{ keep[j] = gL.fth[j]; keep[MAXF + j] = gL.fph[j]; }}
        if (lane == 0) keep_n = K.nfilt;
        __syncthreads();
        K.nfilt = 0; K.nsp[1] = 0; K.resto = 1;
      }} else {{
        const int nf = keep_n;
        for (int j = lane; j < nf; j += WAVE) {{ gL.fth[j] = keep[j]; gL.fph[j] = keep[MAXF + j]; }}
        __syncthreads();
        K.nfilt = nf; K.resto = 0;
      }}
    }}
    __syncthreads();
    if (code & {OP_SNAP}) {{
      double* o = snap + (b * n_ops + ns) * SNAP;   // at most n_ops snapshots
      for (int j = lane; j < MAXF; j += WAVE) {{ o[j] = gL.fth[j]; o[MAXF + j] = gL.fph[j]; }}
      for (int j = lane; j < 4 * FSPILL; j += WAVE) o[2 * MAXF + j] = (slab + b * WS_DOUBLES)[O_FSP + j];
      if (lane == 0) {{
        double* t = o + 2 * MAXF + 4 * FSPILL;
        t[0] = K.nfilt; t[1] = K.nsp[0]; t[2] = K.nsp[1]; t[3] = K.n_filt_over;
      }}
      ns += 1;
    }}
    __syncthreads();
  }}
}}
"""


def chain_source(c: ChainConfig) -> str:
    d = cdims(c)
    dims = f"N == {d.N} && NX == {d.NX} && NMU == {d.NMU} && LX1 == {d.LX1} && SOFF == {d.SOFF}"
    return "".join([gen_of(c.case, c.N).source, _HEAD,
                    f'static_assert({dims}, "the generated dimensions");\n',
                    f'static_assert({c.asserts}, "what this structure is in the harness for");\n',
                    _CHAIN, "}  // namespace mpcx_kernel\n"])


def filter_source(build: str) -> str:
    maxf, fspill = FILTER_PARTS[build]
    return "".join([gen_of(FILTER_CASE, None).source, _HEAD,
                    f'static_assert(MAXF == {maxf} && FSPILL == {fspill}, "the parts of this build");\n',
                    _FILTER, "}  // namespace mpcx_kernel\n"])


def _build(text: str, stem: str, defines: Sequence[str], include_dir: Optional[os.PathLike]) -> pathlib.Path:
    csrc = pathlib.Path(include_dir) if include_dir is not None else native.CSRC
    flags = ["--genco", f"--offload-arch={native.OFFLOAD_ARCH}", "-O3", "-std=c++17", f"-I{native.INCLUDE}",
             f"-I{csrc}", f"-I{native.CSRC}", *[f"-D{x}" for x in defines]]
    deps = [p.read_bytes() for p in native.kernel_sources(csrc)]
    return _compile(text, stem, ".hsaco", flags, deps)


def build_chain(c: ChainConfig, include_dir: Optional[os.PathLike] = None) -> pathlib.Path:
    """The code object of ``c`` (device-only, the flags of ``native.compile_model`` plus the
    configuration's defines; cached by the hash of the source, ``native.kernel_sources`` and the
    command).  ``include_dir``: where the kernel is taken from (a mutated copy)."""
    return _build(chain_source(c), f"ipm_chain_{c.name}", c.defines, include_dir)


def build_filter(build: str, include_dir: Optional[os.PathLike] = None) -> pathlib.Path:
    return _build(filter_source(build), f"ipm_filter_{build}", FILTER_BUILDS[build], include_dir)


def consts(mod: Module) -> Dict[str, int]:
    import torch

    out = torch.full((len(CONST_NAMES),), -1, dtype=torch.int32, device="cuda:0")
    mod.launch("ipmch_consts", 1, [out], len(CONST_NAMES))
    return dict(zip(CONST_NAMES, (int(v) for v in out.cpu().numpy())))


# ---------------------------------------------------------------------------
# running the chain wrapper
# ---------------------------------------------------------------------------

@dataclasses.dataclass
class ChainRun:
    xs: np.ndarray        # [nb, N * NC]
    dinv: np.ndarray      # [nb, N, NC, NC]
    res: np.ndarray       # [nb, 4]: pos, neg, zero, ran
    untouched: bool       # every byte outside the output fields came back as it went in
    padding: bool         # Dinv and xs behind N * NCC / N * NC kept the fill pattern


def run_chain(mod: Module, c: ChainConfig, which: int) -> ChainRun:
    import torch

    d, K = cdims(c), consts(mod)
    assert (K["N"], K["NX"], K["NMU"], K["NC"], K["SOFF"], K["LX1"]) == (d.N, d.NX, d.NMU, d.NC, d.SOFF, d.LX1), K
    chs = chains(c)[0]
    nb, rest = len(chs), K["REST"]
    S, fixm, zx = lay_out(c, chs, np.random.default_rng(name_seed(f"ipm_chain fixm {c.name}")))
    assert S.shape[1] * 8 == K["size_S"] and zx.shape[1] * 8 == K["size_zx"] and d.N * 8 == K["size_fixm"]
    back = torch.zeros((nb, rest), dtype=torch.uint8, device="cuda:0")
    res = torch.full((nb, 4), -7, dtype=torch.int32, device="cuda:0")
    mod.launch("ipmla_chain", nb, [upload(S), torch.as_tensor(fixm, device="cuda:0"), upload(zx), back, res], which)
    back = back.cpu().numpy()
    want = np.full((nb, rest), FILL, dtype=np.uint8)
    for name, arr in (("S", S), ("fixm", fixm), ("zx", zx)):
        want[:, K[f"off_{name}"]:K[f"off_{name}"] + K[f"size_{name}"]] = np.ascontiguousarray(arr).view(np.uint8).reshape(nb, -1)
    mask = np.ones(rest, bool)
    for name in OUTPUT_FIELDS:
        mask[K[f"off_{name}"]:K[f"off_{name}"] + K[f"size_{name}"]] = False
    field = lambda name: np.ascontiguousarray(back[:, K[f"off_{name}"]:K[f"off_{name}"] + K[f"size_{name}"]])
    dv, xv = field("Dinv"), field("xs")
    ncc, nc = d.NC * d.NC, d.NC
    padding = bool((dv[:, d.N * ncc * 8:] == FILL).all() and (xv[:, d.N * nc * 8:] == FILL).all())
    return ChainRun(xs=xv.view(np.float64)[:, :d.N * nc], dinv=dv.view(np.float64)[:, :d.N * ncc].reshape(nb, d.N, nc, nc),
                    res=res.cpu().numpy(), untouched=bool(np.array_equal(back[:, mask], want[:, mask])), padding=padding)


# ---------------------------------------------------------------------------
# the filter: reference list and sequences
# ---------------------------------------------------------------------------

class ListFilter:
    """The filter as the kernel splits it, per tier a spill list and an LDS part in insertion order:
    an insertion drops every entry it dominates (ties included) from both, moves the oldest LDS
    entry to the spill list when the LDS part is still full (a full spill list first drops its own
    oldest entry, counted) and appends.  ``entries`` -- spill list, then LDS part -- is the one
    ordered list of ``simple_filter`` (tests/test_ipm_filter.py shows that on every sequence)."""

    def __init__(self, maxf: int, fspill: int):
        self.maxf, self.fspill = maxf, fspill
        self.sp: List[List[Tuple[float, float]]] = [[], []]
        self.lds: List[Tuple[float, float]] = []
        self.saved: List[Tuple[float, float]] = []
        self.tier, self.over = 0, 0

    def insert(self, th: float, ph: float) -> None:
        kept = lambda es: [e for e in es if not (th <= e[0] and ph <= e[1])]
        sp, lds = kept(self.sp[self.tier]), kept(self.lds)
        if len(lds) >= self.maxf:
            if self.fspill == 0 or len(sp) >= self.fspill:
                sp = sp[1:]
                self.over += 1
            if self.fspill > 0:
                sp.append(lds[0])
            lds = lds[1:]
        lds.append((th, ph))
        self.sp[self.tier], self.lds = sp, lds

    def entries(self) -> List[Tuple[float, float]]:
        return self.sp[self.tier] + self.lds

    def query(self, th: float, ph: float) -> bool:
        return any(th >= e[0] and ph >= e[1] for e in self.sp[self.tier])

    def switch(self, tier: int) -> None:
        if tier == 1:
            self.saved, self.lds, self.sp[1] = self.lds, [], []
        else:
            self.lds = self.saved
        self.tier = tier


def simple_filter(cap: int, ops) -> List[Tuple[List[Tuple[float, float]], int]]:
    """The issue's reference, one ordered list (single tier): per snapshot (list, dropped)."""
    cur: List[Tuple[float, float]] = []
    over, out = 0, []
    for code, th, ph in ops:
        assert (code & 7) != OP_TIER
        if (code & 7) == OP_INSERT:
            cur = [e for e in cur if not (th <= e[0] and ph <= e[1])]
            if len(cur) >= cap:
                cur, over = cur[1:], over + 1
            cur.append((th, ph))
        if code & OP_SNAP:
            out.append((list(cur), over))
    return out


def run_filter(mod: Module, ops: Sequence[Tuple[int, float, float]]):
    """-> (snapshots [nsnap] of dicts, answers {op index: bool}, slab outside the spill tiers untouched)."""
    import torch

    K = consts(mod)
    maxf, fsp, wsd, ofsp = K["MAXF"], K["FSPILL"], K["WS_DOUBLES"], K["O_FSP"]
    assert ofsp + 4 * fsp == wsd
    n = len(ops)
    snapw = 2 * maxf + 4 * fsp + 4
    nsnap = sum(1 for o in ops if o[0] & OP_SNAP)
    slab = torch.full((wsd,), SLAB_SENTINEL, dtype=torch.float64, device="cuda:0")
    snap = torch.zeros((max(nsnap, 1), snapw), dtype=torch.float64, device="cuda:0")
    qout = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    mod.launch("ipmla_filter", 1, [upload(np.asarray(ops, dtype=np.float64).reshape(-1)), slab, snap, qout], n)
    slab, snap, qout = slab.cpu().numpy(), snap.cpu().numpy(), qout.cpu().numpy()
    out = []
    for row in snap[:nsnap]:
        t = row[2 * maxf + 4 * fsp:]
        sp = row[2 * maxf:2 * maxf + 4 * fsp].reshape(2, 2, fsp)
        out.append({"fth": row[:maxf], "fph": row[maxf:2 * maxf], "spill": sp, "nfilt": int(t[0]),
                    "nsp": (int(t[1]), int(t[2])), "over": int(t[3])})
    answers = {i: bool(qout[i]) for i, o in enumerate(ops) if (o[0] & 7) == OP_QUERY}
    assert all(qout[i] in (0, 1) for i in answers)
    return out, answers, bool((slab[:ofsp] == SLAB_SENTINEL).all())


def replay(build_or_parts, ops: Sequence[Tuple[int, float, float]]):
    """The reference on the same operations: -> (per snapshot: (tier + 2 x tier switches so far, lds
    list, spill lists of both tiers, over), answers)."""
    maxf, fsp = FILTER_PARTS[build_or_parts] if isinstance(build_or_parts, str) else build_or_parts
    f = ListFilter(maxf, fsp)
    snaps, answers, switches = [], {}, 0
    for i, (code, th, ph) in enumerate(ops):
        kind = code & 7
        if kind == OP_INSERT:
            f.insert(th, ph)
        elif kind == OP_QUERY:
            answers[i] = f.query(th, ph)
        else:
            f.switch(int(th))
            switches += 1
        if code & OP_SNAP:
            snaps.append((f.tier + 2 * switches, list(f.lds), (list(f.sp[0]), list(f.sp[1])), f.over))
    return snaps, answers


if __name__ == "__main__":   # the content of tests/golden/ipm_chain_fp64_error.json
    print(json.dumps(fp64_errors(), indent=1))
