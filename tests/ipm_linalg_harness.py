"""Device unit harness of the IPM kernel's dense Bunch-Kaufman routines (csrc/ipm/bk.h:
``bk_sweep``, ``bk_sweep2``, ``bk_factor`` + ``bk_inverse``; csrc/mpcx_ipm.hip: ``interior_bk`` +
``trailing_backsolve``), support code of tests/test_ipm_linalg.py.

The routines of bk.h at the model-free sizes are built from a source that includes only the kernel's
two model-free layers (ipm/wave.h, ipm/bk.h; no ``MPCX_*`` dimension is defined); what depends on a
structure (the interior pair, the block chain's ``NB x LDB`` factor) from that structure's generated
model source (it ends with ``#include "mpcx_ipm.hip"``).  Either way wrapper kernels are appended
inside ``namespace mpcx_kernel``; the source is compiled device-only (``--genco``, as a model's own
code object) and launched through a small host launcher (hipModuleLoad / hipModuleLaunchKernel)
loaded with ctypes.  A wrapper runs one wavefront per workgroup on one
matrix (the interior wrapper: on the ``64 / G`` packed stage images of one wave).  It stages the
LDS arrays from global memory, puts a sentinel into 8 guard entries behind every LDS array, fills
the outputs with NaN (integers: a poison value), calls the routine and copies every array back
with its guards; inertia and ``bad`` are written by one lane.

Reference: mpmath at 60 digits (the inverse; the Schur complement ``T - B A^-1 B^T`` and
``B A^-1`` of the interior case); inertia from the eigenvalues, which fp64 ``eigvalsh`` decides
for matrices whose eigenvalues are at least ``SEPARATION`` of the norm away from zero (its error
is a few eps of the norm).  The unit of the tolerance is the scaled error of the plain fp64 host
restatement (tests/test_chain_sweep.py ``sweep``; ``partial_ldl`` below for the interior case) on
the same matrices, recorded in tests/golden/ipm_linalg_fp64_error.json.

Zero pivots.  The kernel calls ``solve()`` only after a factorisation that counted no zero pivot
(``mpcx_ipm_solve``: the multiplier initialisation tests ``in.zero == 0``, the Newton loop takes
the inertia-correction branch otherwise and factorises again), so an inverse, a Schur complement
or a back-substitution operator of a block with a counted zero pivot is never consumed.  What is
pinned for such inputs is therefore the inertia (``bad`` for coupled stage interiors) and, for the
sweeps, their own documented contract: the zero pivot's row and column of the inverse are exactly
0 and the rest is the inverse of the remaining block.  ``bk_inverse`` divides by a pivot in
(0, 1e-20], ``interior_bk`` (independent stages) by any counted zero pivot; neither result is read.
"""

from __future__ import annotations

import ctypes
import dataclasses
import functools
import hashlib
import json
import os
import pathlib
import subprocess
from typing import Dict, List, Optional, Sequence, Tuple

import mpmath as mp
import numpy as np

from agentlib_mpc_amd.runtime import codegen, native
from tests import configs
from tests.eval_harness_core import (DPS, FACTOR, FLOOR, GUARD, ROOT, SENTINEL, _cache_dir,
                                     name_seed, upload)
from tests.test_chain_sweep import ALPHA, BRANCHES, ZERO_PIVOT, sweep

PAD = 3.5e55            # the unused column of an LD = NN + 1 image and the odd-stride pad of a stage slot
ISENTINEL = -77077      # guard entries of the integer LDS arrays
IPOISON = 0x7F7F7F7F    # integer outputs before the routine writes them (piv is not initialised by factor())
SEPARATION = 1e-6       # inertia set: min |eigenvalue| >= SEPARATION * max |eigenvalue|
NMAT = 64               # matrices per class
#: sizes above this take NMAT_LARGE matrices per class: a 60-digit inverse costs ~n^3 x 2 us in
#: mpmath, 64 x 7 of them at n = 36 several minutes
LARGE = 14
NMAT_LARGE = 8

CLASSES = ("random", "saddle", "scaled", "extreme", "zero_rowcol", "zero", "ties")
SINGULAR = ("zero_rowcol", "zero")

SWEEP_SIZES = (1, 2, 3, 4, 6, 7, 8)      # 7: lanes 49-63 own no entry; 8: every lane, a full candidate octet
FACTOR_SIZES = (3, 8, 9, 10, 17)         # 8 | 9: the DPP branches of sigma and of the argmax; 10: wargmax
#: the structures of the interior case: independent stages (NX = 0: zero pivots are counted),
#: bordered continuity rows (NMU > 0), several trailing columns per lane with NI no multiple of G,
#: and the C1 structure.  ``INTERIOR_ASSERTS``: what the harness source asserts of each.
INTERIOR_CASES = ("exchange_supply", "rng_room_mpc", "admm_room", "one_room")
INTERIOR_ASSERTS = {
    "exchange_supply": "NX == 0",
    "rng_room_mpc": "NMU > 0",
    "admm_room": "CPL > 1 && NI % G != 0",
    "one_room": "NX == 1 && NMU == 0",
}
#: the structure with the largest block-chain block among tests/configs.py (NB = 36, LDB = 37)
LARGEST_BLOCK_CASE = "mhe_room"
CONST_NAMES = ("N", "NX", "NV", "NG", "NMU", "NI", "NC", "NLOC", "NTR", "G", "CPL", "PKB", "PKS", "NB", "LDB", "SR")


def nmat(n: int) -> int:
    return NMAT if n <= LARGE else NMAT_LARGE


# ---------------------------------------------------------------------------
# the matrices
# ---------------------------------------------------------------------------

def _sym(rng, n):
    M = rng.normal(size=(n, n))
    return M + M.T


def _draw(cls: str, n: int, m: int, rng) -> np.ndarray:
    A = _sym(rng, n)
    if cls == "saddle":          # zero leading block (bordered multipliers): forces 2x2 pivots
        A[:n // 2, :n // 2] = 0.0
        if m % 4 == 3 and n >= 3:   # the first column's only entry in the last row: the pivot
            A[1:n - 1, 0] = 0.0     # candidate sits in the last lane that holds one
            A[0, 1:n - 1] = 0.0
            A[0, 0] = 0.0
    elif cls == "scaled":        # barrier-scaled diagonal
        A[np.diag_indices(n)] *= 10.0 ** rng.integers(-6, 7, n)
    elif cls == "extreme":       # diagonals of a restoration chain: all large, all small, mixed
        e = (np.full(n, 18), np.full(n, -18), rng.choice([-18, 18], n))[m % 3]
        A[np.diag_indices(n)] = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 9.0, n) * 10.0 ** e
    elif cls == "ties":          # equal off-diagonal magnitudes in the pivot column: the tie-break
        c = float(rng.uniform(0.5, 2.0))
        sg = rng.choice([-1.0, 1.0], (n, n))
        sg = np.triu(sg, 1) + np.triu(sg, 1).T
        if m % 2 == 0:           # every off-diagonal entry
            d = np.diag(A).copy()
            A = c * sg
            A[np.diag_indices(n)] = 0.25 * d
        else:                    # the first pivot column, below a small diagonal entry
            A[1:, 0] = c * sg[1:, 0]
            A[0, 1:] = A[1:, 0]
            A[0, 0] *= 0.1
    return A


def _separated(A: np.ndarray) -> bool:
    ev = np.linalg.eigvalsh(A)
    return bool(np.abs(ev).min() >= SEPARATION * np.abs(ev).max())


@dataclasses.dataclass(frozen=True)
class Mat:
    A: np.ndarray
    cls: str
    zero: Tuple[int, ...]        # indices whose pivot is a zero on purpose
    inertia: Optional[Tuple[int, int, int]]   # (pos, neg, zero); None: not in the inertia set


@functools.lru_cache(maxsize=None)
def matrices(n: int, count: Optional[int] = None) -> Tuple[Mat, ...]:
    """The ``count`` (default ``nmat(n)``) matrices of every class at size ``n``, class-major.
    Non-singular classes are redrawn until the eigenvalues are separated from zero, except the
    mixed 1e+-18 diagonals, whose small eigenvalues are ~1e-36 of the norm by construction: those
    are checked for the inverse only.  Singular classes place their zeros on purpose; their
    inertia is the separated inertia of the remaining block plus the zeros."""
    count = count or nmat(n)
    out = []
    for cls in CLASSES:
        rng = np.random.default_rng(name_seed(f"ipm_linalg {cls} {n}"))
        for m in range(count):
            if cls == "zero":
                out.append(Mat(np.zeros((n, n)), cls, tuple(range(n)), (0, 0, n)))
                continue
            if cls == "zero_rowcol":
                z = m % n
                keep = [i for i in range(n) if i != z]
                while True:
                    A = _sym(rng, n)
                    A[z, :] = 0.0
                    A[:, z] = 0.0
                    if n == 1 or _separated(A[np.ix_(keep, keep)]):
                        break
                if m % 2 == 1:   # a pivot in (0, 1e-20]: counted as zero like an exact one
                    A[z, z] = float(rng.choice([-1.0, 1.0])) * 10.0 ** float(rng.uniform(-25.0, -20.0))
                    if m % 4 == 3:
                        A[z, z] = float(np.sign(A[z, z])) * ZERO_PIVOT
                ev = np.linalg.eigvalsh(A[np.ix_(keep, keep)])
                out.append(Mat(A, cls, (z,), (int((ev > 0).sum()), int((ev < 0).sum()), 1)))
                continue
            for _ in range(200):
                A = _draw(cls, n, m, rng)
                if _separated(A):
                    break
                if cls == "extreme" and m % 3 == 2:
                    break
            sep = _separated(A)
            assert sep or (cls == "extreme" and m % 3 == 2), (cls, n, m)
            ev = np.linalg.eigvalsh(A)
            out.append(Mat(A, cls, (), (int((ev > 0).sum()), int((ev < 0).sum()), 0) if sep else None))
    return tuple(out)


# ---------------------------------------------------------------------------
# mpmath reference
# ---------------------------------------------------------------------------

def _mp_rows(A) -> List[list]:
    return [[mp.mpf(float(v)) for v in row] for row in np.asarray(A, dtype=float)]


def mp_solve(A, R) -> List[list]:
    """A^-1 R by Gauss-Jordan elimination with partial pivoting in mpmath (DPS digits); rows as lists."""
    with mp.workdps(DPS):
        a, r = _mp_rows(A), _mp_rows(R)
        n, w = len(a), len(r[0]) if len(r) else 0
        M = [a[i] + r[i] for i in range(n)]
        for k in range(n):
            p = max(range(k, n), key=lambda i: abs(M[i][k]))
            M[k], M[p] = M[p], M[k]
            piv = M[k][k]
            Mk = M[k] = [v / piv for v in M[k]]
            for i in range(n):
                f = M[i][k]
                if i != k and f != 0:
                    M[i] = [x - f * y for x, y in zip(M[i], Mk)]
        return [row[n:n + w] for row in M]


def _to_obj(rows, shape) -> np.ndarray:
    out = np.empty(shape, dtype=object)
    for i, row in enumerate(rows):
        for j, v in enumerate(row):
            out[i, j] = v
    return out


def mp_inverse(mat: Mat) -> np.ndarray:
    """Object array of mpf: the inverse, with the rows and columns of ``mat.zero`` exactly 0 and the
    inverse of the remaining block elsewhere (the sweeps' contract for a counted zero pivot)."""
    n = len(mat.A)
    keep = [i for i in range(n) if i not in mat.zero]
    out = np.empty((n, n), dtype=object)
    out[:, :] = mp.mpf(0)
    if keep:
        sub = mat.A[np.ix_(keep, keep)]
        out[np.ix_(keep, keep)] = _to_obj(mp_solve(sub, np.eye(len(keep))), (len(keep), len(keep)))
    return out


@functools.lru_cache(maxsize=None)
def inverse_refs(n: int) -> Tuple[np.ndarray, ...]:
    return tuple(mp_inverse(m) for m in matrices(n))


def scaled_error(got, ref) -> float:
    """max |got - ref| / max |ref| of one matrix; an all-zero reference must be met exactly, a
    non-finite entry is an infinite error."""
    got = np.asarray(got, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float("inf")
    with mp.workdps(DPS):
        scale = max((abs(r) for r in ref.ravel()), default=mp.mpf(0))
        worst = max((abs(mp.mpf(float(g)) - r) for g, r in zip(got.ravel(), ref.ravel())), default=mp.mpf(0))
        if scale == 0:
            return 0.0 if worst == 0 else float("inf")
        return float(worst / scale)


# ---------------------------------------------------------------------------
# fp64 host restatements
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def swept(n: int):
    """(inverse, inertia, branches) of the host sweep for every matrix of ``matrices(n)``."""
    out = []
    for m in matrices(n):
        br: List[str] = []
        with np.errstate(all="ignore"):
            inv, inertia = sweep(m.A, br)
        out.append((inv, tuple(int(v) for v in inertia), tuple(br)))
    return tuple(out)


def partial_ldl(W0: np.ndarray, ni: int, coupled: bool):
    """``interior_bk`` + ``trailing_backsolve`` on the full symmetric image ``W0`` (interior
    ``ni x ni`` first, then the trailing rows): Bunch-Kaufman over the interior pivots only, the
    trailing rows receive the updates and the multipliers.  Returns (Schur complement on the
    trailing rows, trailing rows' interior columns after the back-substitution, perm, (pos, neg,
    zero), bad, branches); ``coupled``: a zero pivot ends the factorisation (``bad``)."""
    W = np.array(W0, float)
    perm = list(range(ni))
    piv = [0] * ni
    pos = neg = nz = 0
    branches = []
    k = 0
    while k < ni:
        akk = abs(W[k, k])
        cand = range(k + 1, ni)
        r = max(cand, key=lambda i: (abs(W[i, k]), -i)) if k + 1 < ni else -1
        lam = abs(W[r, k]) if r >= 0 else 0.0
        if max(akk, lam) == 0.0:
            branches.append("k_first")
            if coupled:
                return None, None, perm, (pos, neg, nz), 1, branches
            nz += 1
            piv[k] = 1
            k += 1
            continue
        size, kp, branch = 1, k, "k_first"
        if akk < ALPHA * lam:
            sigma = max([abs(W[r, j]) for j in range(k, ni) if j != r], default=0.0)
            if akk * sigma >= ALPHA * lam * lam:
                branch = "k_second"
            elif abs(W[r, r]) >= ALPHA * sigma:
                kp, branch = r, "r"
            else:
                size, kp, branch = 2, r, "2x2"
        branches.append(branch)
        p = k + size - 1
        if kp != p:
            W[[p, kp], :] = W[[kp, p], :]
            W[:, [p, kp]] = W[:, [kp, p]]
            perm[p], perm[kp] = perm[kp], perm[p]
        if size == 1:
            d = W[k, k]
            if abs(d) <= ZERO_PIVOT:
                if coupled:
                    return None, None, perm, (pos, neg, nz), 1, branches
                nz += 1
            elif d > 0:
                pos += 1
            else:
                neg += 1
            with np.errstate(all="ignore"):
                l = W[k + 1:, k] / d
                W[k + 1:, k + 1:] -= np.outer(W[k + 1:, k], l)
            W[k + 1:, k] = l
            W[k, k + 1:] = l
            piv[k] = 1
        else:
            a11, a21, a22 = W[k, k], W[k + 1, k], W[k + 1, k + 1]
            det = a11 * a22 - a21 * a21
            if abs(det) <= ZERO_PIVOT ** 2:
                if coupled:
                    return None, None, perm, (pos, neg, nz), 1, branches
                nz += 2
            elif det < 0:
                pos, neg = pos + 1, neg + 1
            elif a11 + a22 > 0:
                pos += 2
            else:
                neg += 2
            with np.errstate(all="ignore"):
                c1, c2 = W[k + 2:, k].copy(), W[k + 2:, k + 1].copy()
                l1, l2 = (c1 * a22 - c2 * a21) / det, (c2 * a11 - c1 * a21) / det
                W[k + 2:, k + 2:] -= np.outer(c1, l1) + np.outer(c2, l2)
            W[k + 2:, k], W[k + 2:, k + 1] = l1, l2
            W[k, k + 2:], W[k + 1, k + 2:] = l1, l2
            piv[k], piv[k + 1] = 2, 0
        k += size
    Z = W[ni:, :ni].copy()
    with np.errstate(all="ignore"):
        for m in range(ni - 1, 0, -1):
            skip = m - 1 if piv[m - 1] == 2 else -1
            for i in range(m):
                if i != skip:
                    Z[:, i] -= W[m, i] * Z[:, m]
    return W[ni:, ni:].copy(), Z, perm, (pos, neg, nz), 0, branches


# ---------------------------------------------------------------------------
# the interior case: stage images of a structure
# ---------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Dims:
    """The constants of mpcx_ipm.hip that fix the image layout, from the generated dimensions."""
    NX: int
    NI: int
    NC: int

    @property
    def NLOC(self) -> int:
        return self.NI + self.NX + self.NC

    @property
    def NTR(self) -> int:
        return self.NX + self.NC + 1

    @property
    def PKB(self) -> int:
        return (self.NLOC + 1) * (self.NLOC + 2) // 2

    @property
    def PKS(self) -> int:
        return self.PKB | 1


@functools.lru_cache(maxsize=None)
def case_gen(case: str):
    return configs.CASES[case]().backend.problem.gen


def nmu_of(gen) -> int:
    import re

    m = re.search(r"#define MPCX_NMU (\d+)", gen.source)
    return int(m.group(1)) if m else 0


@functools.lru_cache(maxsize=None)
def dims_of(case: str) -> Dims:
    gen = case_gen(case)
    d, nmu = gen.dims, nmu_of(gen)
    return Dims(NX=d["NX"], NI=d["NV"] + d["NG"] - nmu, NC=d["NX"] + nmu)


@dataclasses.dataclass(frozen=True)
class Image:
    W: np.ndarray        # full symmetric (NLOC + 1) x (NLOC + 1): [[A, B^T], [B, T]]
    mat: Mat             # the interior block


@functools.lru_cache(maxsize=None)
def images(case: str) -> Tuple[Image, ...]:
    """One stage image per interior matrix, in launch order: the classes interleaved, so that the
    lane groups of one wave hold matrices of different classes and (coupled stages) a singular
    interior, which ends ``bad``, sits between groups that run on."""
    d = dims_of(case)
    mats = matrices(d.NI)
    per = len(mats) // len(CLASSES)
    rng = np.random.default_rng(name_seed(f"ipm_linalg images {case}"))
    out = []
    for m in range(per):
        for c in range(len(CLASSES)):
            mat = mats[c * per + m]
            W = _sym(rng, d.NLOC + 1)
            W[:d.NI, :d.NI] = mat.A
            out.append(Image(W, mat))
    return tuple(out)


def pack(W: np.ndarray, d: Dims) -> np.ndarray:
    """Packed lower triangle of one slot (PKS doubles; the odd-stride pad holds PAD)."""
    F = np.full(d.PKS, PAD)
    i, j = np.tril_indices(d.NLOC + 1)
    F[i * (i + 1) // 2 + j] = W[i, j]
    return F


def unpack_trailing(F: np.ndarray, d: Dims):
    """(trailing block [NTR, NTR] (lower, mirrored), trailing rows' interior columns [NTR, NI])."""
    pko = lambda i: i * (i + 1) // 2
    T = np.zeros((d.NTR, d.NTR))
    Z = np.zeros((d.NTR, d.NI))
    for t in range(d.NTR):
        o = pko(d.NI + t)
        Z[t] = F[o:o + d.NI]
        for s in range(t + 1):
            T[t, s] = T[s, t] = F[o + d.NI + s]
    return T, Z


def trailing_mask(d: Dims) -> np.ndarray:
    """Entries of the trailing block that are defined: all but the (rhs, rhs) corner, which the
    kernel uses as the target of its predicated-off writes."""
    mask = np.ones((d.NTR, d.NTR), bool)
    mask[-1, -1] = False
    return mask


@functools.lru_cache(maxsize=None)
def interior_refs(case: str):
    """Per image (None where the interior is singular on purpose): (Schur complement
    ``T - B A^-1 B^T`` with the undefined corner 0, ``B A^-1`` [NTR, NI] in original column order),
    object arrays of mpf."""
    d = dims_of(case)
    out = []
    for im in images(case):
        if im.mat.zero:
            out.append(None)
            continue
        A, B, T = im.W[:d.NI, :d.NI], im.W[d.NI:, :d.NI], im.W[d.NI:, d.NI:]
        with mp.workdps(DPS):
            X = _to_obj(mp_solve(A, B.T), (d.NI, d.NTR))         # A^-1 B^T
            Bm = _to_obj(_mp_rows(B), B.shape)
            S = _to_obj(_mp_rows(T), T.shape) - Bm.dot(X)
            S[-1, -1] = mp.mpf(0)
        out.append((S, X.T.copy()))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def interior_restated(case: str):
    d = dims_of(case)
    return tuple(partial_ldl(im.W, d.NI, d.NX > 0) for im in images(case))


def interior_errors(case: str, idx: int, T: np.ndarray, Z: np.ndarray, perm: Sequence[int]) -> Dict[str, float]:
    """Scaled errors of one image's results: ``T`` the trailing block, ``Z`` the trailing rows'
    interior columns in pivot order (column p belongs to interior index ``perm[p]``: solve() writes
    the entry of operator column p to local index ``a.prm(k)[p]``)."""
    d = dims_of(case)
    S, BAinv = interior_refs(case)[idx]
    Tm = np.where(trailing_mask(d), T, 0.0)
    Zo = np.empty_like(Z)
    Zo[:, list(perm)] = Z
    return {"schur": scaled_error(Tm, S), "z": scaled_error(Zo, BAinv)}


# ---------------------------------------------------------------------------
# the tolerance unit
# ---------------------------------------------------------------------------

def _class_max(n_or_mats, errs) -> Dict[str, float]:
    out: Dict[str, float] = {}
    for m, e in zip(n_or_mats, errs):
        out[m.cls] = max(out.get(m.cls, 0.0), e)
    return out


def block_case_size() -> Tuple[int, int]:
    d = case_gen(LARGEST_BLOCK_CASE).dims
    nb = d["NV"] + d["NX"] + d["NG"]
    return nb, nb + 1 if nb % 2 == 0 else nb


def inverse_sizes() -> List[int]:
    return sorted(set(SWEEP_SIZES) | set(FACTOR_SIZES) | {block_case_size()[0]})


def fp64_errors() -> dict:
    """The unit of the tolerance: per routine family, size or structure, and matrix class, the
    largest scaled error of the fp64 host restatement against the mpmath reference."""
    inv = {}
    for n in inverse_sizes():
        errs = [scaled_error(s[0], r) for s, r in zip(swept(n), inverse_refs(n))]
        inv[f"n{n}"] = _class_max(matrices(n), errs)
    inter = {}
    for case in INTERIOR_CASES:
        per: Dict[str, Dict[str, float]] = {}
        for idx, (im, rs) in enumerate(zip(images(case), interior_restated(case))):
            if im.mat.zero:
                continue
            e = interior_errors(case, idx, rs[0], rs[1], rs[2])
            slot = per.setdefault(im.mat.cls, {"schur": 0.0, "z": 0.0})
            for k, v in e.items():
                slot[k] = max(slot[k], v)
        inter[case] = per
    return {"inverse": inv, "interior": inter}


GOLDEN = os.path.join(ROOT, "tests", "golden", "ipm_linalg_fp64_error.json")


@functools.lru_cache(maxsize=None)
def golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


def bound(recorded: float) -> float:
    return max(FACTOR * recorded, FLOOR)


# ---------------------------------------------------------------------------
# the HIP source and its build
# ---------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Config:
    """One harness source: a structure's (``case``: the interior pair, the block-chain size), or the
    model-free one (``case`` None: sweeps, LDL^T + inverse at the listed sizes)."""
    case: Optional[str]
    sweeps: Tuple[Tuple[int, int], ...] = ()
    factors: Tuple[Tuple[int, int], ...] = ()
    interior: bool = False

    @property
    def name(self) -> str:
        return self.case or "dense"


#: the model-free source: every size of the sweeps and of the LDL^T + inverse pair
DENSE = Config(None, tuple((n, ld) for n in SWEEP_SIZES for ld in (n, n + 1)), tuple((n, n) for n in FACTOR_SIZES))
CONFIGS = (*(Config(case, interior=True) for case in INTERIOR_CASES),
           Config(LARGEST_BLOCK_CASE, factors=(("NB", "LDB"),)))
BY_NAME = {c.name: c for c in (DENSE, *CONFIGS)}

#: what the model-free source includes, all of it
DENSE_INCLUDES = ("hip/hip_runtime.h", "ipm/wave.h", "ipm/bk.h")

# a structure's source only: the kernel's constants
_CONSTS = f"""
extern "C" __global__ void __launch_bounds__(64) ipmla_consts(int* __restrict__ out, int n) {{
  const int v[{len(CONST_NAMES)}] = {{{", ".join(CONST_NAMES)}}};
  if (threadIdx.x == 0 && blockIdx.x == 0)
    for (int i = 0; i < {len(CONST_NAMES)} && i < n; ++i) out[i] = v[i];
}}
"""

_COMMON = f"""
// generated by tests/ipm_linalg_harness.py: wrapper kernels of the dense Bunch-Kaufman routines
namespace mpcx_kernel {{
#define H_GUARD {GUARD}
#define H_SENT ({SENTINEL!r})
#define H_ISENT ({ISENTINEL})
#define H_IPOISON ({IPOISON})

__device__ __forceinline__ void h_put(int* res, const Inertia in, int bad) {{
  res[0] = in.pos; res[1] = in.neg; res[2] = in.zero; res[3] = bad;
}}

// one matrix per workgroup: A (destroyed) and out, NN x LD each
template <int NN, int LD>
__device__ __forceinline__ void h_sweep(const double* __restrict__ Ain, double* __restrict__ Aback,
                                        double* __restrict__ Oback, int* __restrict__ res) {{
  constexpr int SZ = NN * LD, GD = H_GUARD;
  __shared__ double sa[SZ + GD];
  __shared__ double so[SZ + GD];
  const int lane = threadIdx.x, b = blockIdx.x;
  for (int i = lane; i < SZ; i += WAVE) {{ sa[i] = Ain[b * SZ + i]; so[i] = __builtin_nan(""); }}
  if (lane < GD) {{ sa[SZ + lane] = H_SENT; so[SZ + lane] = H_SENT; }}
  __syncthreads();
  const Inertia in = bk_sweep<NN, LD>(LDSP(sa), LDSP(so), lane);
  __syncthreads();
  for (int i = lane; i < SZ + GD; i += WAVE) {{ Aback[b * (SZ + GD) + i] = sa[i]; Oback[b * (SZ + GD) + i] = so[i]; }}
  if (lane == 0) h_put(res + 4 * b, in, 0);
}}

// two matrices per workgroup, swept in place; twob[b] == 0: A alone
template <int NN, int LD>
__device__ __forceinline__ void h_sweep2(const double* __restrict__ Ain, const double* __restrict__ Bin,
                                         const int* __restrict__ twob, double* __restrict__ Aback,
                                         double* __restrict__ Bback, int* __restrict__ res) {{
  constexpr int SZ = NN * LD, GD = H_GUARD;
  __shared__ double sa[SZ + GD];
  __shared__ double sb[SZ + GD];
  const int lane = threadIdx.x, b = blockIdx.x;
  for (int i = lane; i < SZ; i += WAVE) {{ sa[i] = Ain[b * SZ + i]; sb[i] = Bin[b * SZ + i]; }}
  if (lane < GD) {{ sa[SZ + lane] = H_SENT; sb[SZ + lane] = H_SENT; }}
  __syncthreads();
  const Inertia in = bk_sweep2<NN, LD>(LDSP(sa), LDSP(sb), twob[b] != 0, lane);
  __syncthreads();
  for (int i = lane; i < SZ + GD; i += WAVE) {{ Aback[b * (SZ + GD) + i] = sa[i]; Bback[b * (SZ + GD) + i] = sb[i]; }}
  if (lane == 0) h_put(res + 4 * b, in, 0);
}}

// one matrix per workgroup: back come A (factored) | W | Y | out and perm | piv
template <int NN, int LD>
__device__ __forceinline__ void h_factor(const double* __restrict__ Ain, double* __restrict__ Dback,
                                         int* __restrict__ Iback, int* __restrict__ res) {{
  constexpr int SZ = NN * LD, GD = H_GUARD;
  __shared__ double sd[4][SZ + GD];
  __shared__ int si[2][NN + GD];
  const int lane = threadIdx.x, b = blockIdx.x;
  for (int i = lane; i < SZ; i += WAVE) {{
    sd[0][i] = Ain[b * SZ + i];
    sd[1][i] = __builtin_nan(""); sd[2][i] = __builtin_nan(""); sd[3][i] = __builtin_nan("");
  }}
  for (int i = lane; i < NN; i += WAVE) {{ si[0][i] = H_IPOISON; si[1][i] = H_IPOISON; }}
  if (lane < GD) {{
    for (int a = 0; a < 4; ++a) sd[a][SZ + lane] = H_SENT;
    si[0][NN + lane] = H_ISENT; si[1][NN + lane] = H_ISENT;
  }}
  __syncthreads();
  const Inertia in = bk_factor<NN, LD>(LDSP(sd[0]), LDSI(si[0]), LDSI(si[1]), lane);
  bk_inverse<NN, LD>(LDSP(sd[0]), LDSI(si[0]), LDSI(si[1]), LDSP(sd[1]), LDSP(sd[2]), LDSP(sd[3]), lane);
  __syncthreads();
  for (int i = lane; i < 4 * (SZ + GD); i += WAVE) Dback[b * 4 * (SZ + GD) + i] = sd[i / (SZ + GD)][i % (SZ + GD)];
  for (int i = lane; i < 2 * (NN + GD); i += WAVE) Iback[b * 2 * (NN + GD) + i] = si[i / (NN + GD)][i % (NN + GD)];
  if (lane == 0) h_put(res + 4 * b, in, 0);
}}
"""

_INTERIOR = """
// the WAVE / G packed stage images of one wave, laid out as factor()'s dense pass lays them out:
// slot = lane / G, g = lane % G, the images PKS doubles apart, perm and piv NI entries apart, perm
// set to the identity by the slot's lanes, piv left as it is (here: poisoned).  A slot that ends
// bad skips the back-substitution, as the kernel does (it takes the block chain then).
extern "C" __global__ void __launch_bounds__(64) ipmla_interior(const double* __restrict__ Fin, double* __restrict__ Fback,
                                                                int* __restrict__ Iback, int* __restrict__ res, int n) {
  constexpr int NS = WAVE / G, GD = H_GUARD;
  __shared__ double sf[NS * PKS + GD];
  __shared__ int si[2][NS * NI + GD];
  const int lane = threadIdx.x, b = blockIdx.x;
  for (int i = lane; i < NS * PKS; i += WAVE) sf[i] = Fin[(long)b * NS * PKS + i];
  for (int i = lane; i < NS * NI; i += WAVE) { si[0][i] = H_IPOISON; si[1][i] = H_IPOISON; }
  if (lane < GD) { sf[NS * PKS + lane] = H_SENT; si[0][NS * NI + lane] = H_ISENT; si[1][NS * NI + lane] = H_ISENT; }
  __syncthreads();
  const int g = lane % G, slot = lane / G;
  ldsd* F = LDSP(sf + slot * PKS);
  ldsi* perm = LDSI(si[0] + slot * NI);
  ldsi* piv = LDSI(si[1] + slot * NI);
  for (int i = g; i < NI; i += G) perm[i] = i;
  wsync();
  const BKOut bo = interior_bk(F, perm, piv, g);
  wsync();
  if (!bo.bad) trailing_backsolve(F, piv, g);
  __syncthreads();
  for (int i = lane; i < NS * PKS + GD; i += WAVE) Fback[(long)b * (NS * PKS + GD) + i] = sf[i];
  for (int i = lane; i < 2 * (NS * NI + GD); i += WAVE)
    Iback[(long)b * 2 * (NS * NI + GD) + i] = si[i / (NS * NI + GD)][i % (NS * NI + GD)];
  if (g == 0) {
    int* r = res + 4 * (b * NS + slot);
    r[0] = bo.pos; r[1] = bo.neg; r[2] = bo.zero; r[3] = bo.bad;
  }
  (void)n;
}
"""


def kernel_name(kind: str, n, ld) -> str:
    return f"ipmla_{kind}_{n}_{ld}"


def dense_head() -> str:
    """What the wrappers of bk.h need in front of them: the two model-free layers and the reciprocal
    ``MPCX_RCP`` as the code generator writes it into every model source."""
    first, *layers = DENSE_INCLUDES
    return f"#include <{first}>\n" + "\n".join(codegen.RCP_LINES) + "\n" + "".join(f'#include "{name}"\n' for name in layers)


def source(c: Config) -> str:
    parts = [dense_head(), _COMMON] if c.case is None else [case_gen(c.case).source, _COMMON, _CONSTS]
    for n, ld in c.sweeps:
        parts.append(f"""
extern "C" __global__ void __launch_bounds__(64) {kernel_name("sweep", n, ld)}(
    const double* Ain, double* Aback, double* Oback, int* res, int n) {{ h_sweep<{n}, {ld}>(Ain, Aback, Oback, res); (void)n; }}
extern "C" __global__ void __launch_bounds__(64) {kernel_name("sweep2", n, ld)}(
    const double* Ain, const double* Bin, const int* twob, double* Aback, double* Bback, int* res, int n) {{
  h_sweep2<{n}, {ld}>(Ain, Bin, twob, Aback, Bback, res); (void)n; }}
""")
    for n, ld in c.factors:
        parts.append(f"""
extern "C" __global__ void __launch_bounds__(64) {kernel_name("factor", n, ld)}(
    const double* Ain, double* Dback, int* Iback, int* res, int n) {{ h_factor<{n}, {ld}>(Ain, Dback, Iback, res); (void)n; }}
""")
    if c.interior:
        parts.append(f'static_assert({INTERIOR_ASSERTS[c.case]}, "what this structure is in the harness for");\n')
        parts.append(_INTERIOR)
    parts.append("}  // namespace mpcx_kernel\n")
    return "".join(parts)


_LAUNCHER = """// generated by tests/ipm_linalg_harness.py: loads a code object, launches its wrapper kernels
#include <hip/hip_runtime.h>

extern "C" int ipmla_load(const char* path, void** mod) {
  hipModule_t m;
  if (hipModuleLoad(&m, path) != hipSuccess) return 1;
  *mod = (void*)m;
  return 0;
}

// kernel(ptrs[0], ..., ptrs[nptr - 1], n) on nb workgroups of one wavefront
extern "C" int ipmla_launch(void* mod, const char* name, int nb, int nptr, void** ptrs, int n) {
  hipFunction_t f;
  if (nptr > 15 || hipModuleGetFunction(&f, (hipModule_t)mod, name) != hipSuccess) return 2;
  void* args[16];
  for (int i = 0; i < nptr; ++i) args[i] = &ptrs[i];
  args[nptr] = &n;
  if (hipModuleLaunchKernel(f, nb, 1, 1, 64, 1, 1, 0, 0, args, nullptr) != hipSuccess) return 3;
  return hipDeviceSynchronize() == hipSuccess ? 0 : 4;
}
"""


def _compile(text: str, stem: str, suffix: str, flags: Sequence[str], deps: Sequence[bytes]) -> pathlib.Path:
    key = hashlib.sha1()
    for part in (text.encode(), *deps, " ".join(flags).encode()):
        key.update(part)
    d = _cache_dir()
    name = f"{stem}_{key.hexdigest()[:12]}"
    out = d / f"{name}{suffix}"
    if out.exists():
        return out
    src = d / f"{name}.hip"
    src.write_text(text)
    tmp = d / f"{name}.{os.getpid()}{suffix}.tmp"
    res = subprocess.run([native._hipcc(), *flags, str(src), "-o", str(tmp)], capture_output=True, text=True)
    if res.returncode != 0:
        tmp.unlink(missing_ok=True)
        raise RuntimeError(f"building {stem} failed:\n{res.stderr[-4000:]}")
    os.replace(tmp, out)
    return out


def build(c: Config, include_dir: Optional[os.PathLike] = None) -> pathlib.Path:
    """The code object of config ``c`` (device-only, the flags of ``native.compile_model``; cached by
    the hash of the source, ``native.kernel_sources`` and the command).  ``include_dir``: where the
    kernel (mpcx_ipm.hip, ipm/) is taken from (a mutated copy)."""
    csrc = pathlib.Path(include_dir) if include_dir is not None else native.CSRC
    flags = ["--genco", f"--offload-arch={native.OFFLOAD_ARCH}", "-O3", "-std=c++17", f"-I{native.INCLUDE}",
             f"-I{csrc}", f"-I{native.CSRC}"]
    deps = [p.read_bytes() for p in native.kernel_sources(csrc)]
    return _compile(source(c), f"ipm_linalg_{c.name}", ".hsaco", flags, deps)


def build_launcher() -> pathlib.Path:
    flags = ["-shared", "-fPIC", "-O2", "-std=c++17"]
    return _compile(_LAUNCHER, "ipm_linalg_launcher", ".so", flags, [])


class Module:
    """A loaded code object and the launcher."""

    def __init__(self, hsaco: os.PathLike):
        self.lib = ctypes.CDLL(str(build_launcher()))
        self.lib.ipmla_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        self.lib.ipmla_launch.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
        mod = ctypes.c_void_p()
        rc = self.lib.ipmla_load(str(hsaco).encode(), ctypes.byref(mod))
        if rc != 0:
            raise RuntimeError(f"loading {hsaco} failed ({rc})")
        self.mod = mod

    def launch(self, kernel: str, nb: int, tensors, n: int = 0) -> None:
        import torch

        ptrs = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        torch.cuda.synchronize()
        rc = self.lib.ipmla_launch(self.mod, kernel.encode(), nb, len(tensors), ptrs, n)
        assert rc == 0, (kernel, rc)

    def consts(self) -> Dict[str, int]:
        import torch

        out = torch.full((len(CONST_NAMES),), -1, dtype=torch.int32, device="cuda:0")
        self.launch("ipmla_consts", 1, [out], len(CONST_NAMES))
        return dict(zip(CONST_NAMES, (int(v) for v in out.cpu().numpy())))


def _zeros(shape, dtype):
    import torch

    return torch.zeros(shape, dtype=dtype, device="cuda:0")


def embed(mats: Sequence[np.ndarray], n: int, ld: int) -> np.ndarray:
    """[len, n * ld]: row-major images with leading dimension ``ld``, the unused column PAD."""
    X = np.full((len(mats), n, ld), PAD)
    for b, A in enumerate(mats):
        X[b, :, :n] = A
    return X.reshape(len(mats), n * ld)


def run_sweep(mod: Module, n: int, ld: int, mats: Sequence[np.ndarray]):
    """-> (A back [nb, n*ld + GUARD], out back, res [nb, 4])."""
    import torch

    nb, sz = len(mats), n * ld
    Ab, Ob = _zeros((nb, sz + GUARD), torch.float64), _zeros((nb, sz + GUARD), torch.float64)
    res = torch.full((nb, 4), -1, dtype=torch.int32, device="cuda:0")
    mod.launch(kernel_name("sweep", n, ld), nb, [upload(embed(mats, n, ld)), Ab, Ob, res])
    return Ab.cpu().numpy(), Ob.cpu().numpy(), res.cpu().numpy()


def run_sweep2(mod: Module, n: int, ld: int, matsA, matsB, twob):
    import torch

    nb, sz = len(matsA), n * ld
    Ab, Bb = _zeros((nb, sz + GUARD), torch.float64), _zeros((nb, sz + GUARD), torch.float64)
    res = torch.full((nb, 4), -1, dtype=torch.int32, device="cuda:0")
    mod.launch(kernel_name("sweep2", n, ld), nb,
               [upload(embed(matsA, n, ld)), upload(embed(matsB, n, ld)), upload(np.asarray(twob, dtype=np.int32)),
                Ab, Bb, res])
    return Ab.cpu().numpy(), Bb.cpu().numpy(), res.cpu().numpy()


def run_factor(mod: Module, n: int, ld: int, mats, kernel: Optional[str] = None):
    """-> (doubles back [nb, 4, n*ld + GUARD]: A | W | Y | out, ints back [nb, 2, n + GUARD]: perm | piv, res)."""
    import torch

    nb, sz = len(mats), n * ld
    Db = _zeros((nb, 4, sz + GUARD), torch.float64)
    Ib = _zeros((nb, 2, n + GUARD), torch.int32)
    res = torch.full((nb, 4), -1, dtype=torch.int32, device="cuda:0")
    mod.launch(kernel or kernel_name("factor", n, ld), nb, [upload(embed(mats, n, ld)), Db, Ib, res])
    return Db.cpu().numpy(), Ib.cpu().numpy(), res.cpu().numpy()


def run_interior(mod: Module, case: str, G: int):
    """All images of ``case``, 64 / G per workgroup (the last workgroup is filled up with copies of
    the first images) -> (F back [nimg, PKS], guard [nb, GUARD], perm [nimg, NI], piv [nimg, NI],
    int guards [nb, 2, GUARD], res [nimg, 4], number of images)."""
    import torch

    d = dims_of(case)
    ims = images(case)
    ns = 64 // G
    nb = (len(ims) + ns - 1) // ns
    F = np.stack([pack(ims[i % len(ims)].W, d) for i in range(nb * ns)])
    Fb = _zeros((nb, ns * d.PKS + GUARD), torch.float64)
    Ib = _zeros((nb, 2, ns * d.NI + GUARD), torch.int32)
    res = torch.full((nb * ns, 4), -1, dtype=torch.int32, device="cuda:0")
    mod.launch("ipmla_interior", nb, [upload(F.reshape(nb, ns * d.PKS)), Fb, Ib, res])
    Fb, Ib = Fb.cpu().numpy(), Ib.cpu().numpy()
    return (Fb[:, :ns * d.PKS].reshape(nb * ns, d.PKS), Fb[:, ns * d.PKS:],
            Ib[:, 0, :ns * d.NI].reshape(nb * ns, d.NI), Ib[:, 1, :ns * d.NI].reshape(nb * ns, d.NI),
            Ib[:, :, ns * d.NI:], res.cpu().numpy(), len(ims))


# ---------------------------------------------------------------------------
# sweep2 pairs
# ---------------------------------------------------------------------------

def sweep2_pairs(n: int) -> List[Tuple[int, int, bool]]:
    """(index of A, index of B, twob) into ``matrices(n)``: every matrix is A once; B walks the set
    with a stride coprime to its length, so the classes of a pair differ for most pairs; every
    eighth pair sweeps A alone."""
    total = len(matrices(n))
    stride = 149   # prime, no divisor of 7 * 64
    return [(a, (a * stride + 67) % total, a % 8 != 7) for a in range(total)]


if __name__ == "__main__":   # the content of tests/golden/ipm_linalg_fp64_error.json
    print(json.dumps(fp64_errors(), indent=1))
