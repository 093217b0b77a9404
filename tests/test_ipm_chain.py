"""The IPM kernel's state chain on the device, alone: ``chain_factor`` + ``chain_solve`` (the scalar
scan with its guard and the serial recurrence; the one-sided block chain, through the sweep and --
``MPCX_CHAIN_BK`` -- through ``bk_factor`` + ``bk_inverse``) and ``chain_factor_tw`` +
``chain_solve_tw`` at the horizons where the twisted order's step structure changes, against an
mpmath reference (tests/ipm_chain_harness.py: the wrapper, the chains, the references, what is
pinned at a zero pivot).

Tolerance: the scaled error of ``xs`` and of every ``Dinv`` slot stays within FACTOR = 8 times the
largest scaled error of the fp64 host restatement on the chains of the same structure, horizon,
order and class (tests/golden/ipm_chain_fp64_error.json) and is never held below 4 eps.  Inertia
must match exactly.
"""

import itertools
import os
import shutil

import numpy as np
import pytest

from tests import ipm_chain_harness as h

GOLD = h.golden()
HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
NAMES = [c.name for c in h.CHAIN_CONFIGS]
SCALAR = [c.name for c in h.CHAIN_CONFIGS if h.cdims(c).scalar]
BLOCK = [c.name for c in h.CHAIN_CONFIGS if not h.cdims(c).scalar]
BOTH_ORDERS = [c.name for c in h.CHAIN_CONFIGS if h.orders_of(c) == h.ORDERS]


# ---------------------------------------------------------------------------
# CPU: the chains, the restatements, the recorded unit, the build
# ---------------------------------------------------------------------------

def test_configurations():
    """The horizons of the issue: the scalar chain at 1, 2, 4, 15, a full DPP row and one past it;
    the twisted chain from one boundary up to the shipped 15; the LDL^T pair; two assembly passes."""
    got = {(c.case, c.defines): [] for c in h.CHAIN_CONFIGS}
    for c in h.CHAIN_CONFIGS:
        got[(c.case, c.defines)].append(c.N)
    assert got == {("one_room", ()): [1, 2, 4, 15, 16, 17], ("one_room_du", ()): [1, 2, 3, 4, 5, 15],
                   ("one_room_du", ("MPCX_CHAIN_BK",)): [2, 5], ("mhe_room", ()): [2, 15]}
    for c in h.CHAIN_CONFIGS:
        d = h.cdims(c)
        assert (d.NX, d.NMU) == {"one_room": (1, 0), "one_room_du": (2, 2), "mhe_room": (3, 3)}[c.case]
        assert h.nchain(d) == (16 if d.N * d.NC <= 20 else 4)


@pytest.mark.parametrize("name", NAMES)
def test_chain_sets(name):
    """Every chain of a non-zero class is in the inertia set (eigenvalues at least SEPARATION of the
    largest away from zero; the scaled classes: of the congruent unscaled chain), no class rejected
    more draws than it kept, no member is left out, and the host restatement's inertia is the
    eigenvalues' (zero classes: of the rest, plus the zeros)."""
    c = h.CHAIN_BY_NAME[name]
    d = h.cdims(c)
    chs, counts = h.chains(c)
    classes = h.SCALAR_CLASSES if d.scalar else h.BLOCK_CLASSES
    assert [ch.cls for ch in chs] == [cls for cls in classes for _ in range(h.nchain(d, cls))]
    for cls, (kept, rejected) in counts.items():
        assert kept == h.nchain(d, cls) and rejected <= kept, (cls, kept, rejected)
    for ch, rs in zip(chs, h.restated(c)):
        assert ch.inertia is not None and sum(ch.inertia) == d.N * d.NC
        assert bool(ch.zero) == (ch.cls == "zero")
        T = h.full_matrix(ch.S11, ch.S00, ch.S10, ch.fix, d.NX, d.NMU)
        assert np.array_equal(T, T.T)
        if not ch.zero and ch.cls not in ("scaled", "extreme"):
            ev = np.linalg.eigvalsh(T / np.abs(T).max())
            assert np.abs(ev).min() >= h.SEPARATION * np.abs(ev).max()
            assert ch.inertia == (int((ev > 0).sum()), int((ev < 0).sum()), 0)
        for o, (x, dinv, inertia) in rs.items():
            assert inertia == ch.inertia, (ch.cls, o, inertia, ch.inertia)
            assert np.isfinite(dinv).all() and (ch.zero or np.isfinite(x).all())
        for j in range(d.N):     # fixed entries of the right-hand side are 0
            for i in ch.fix[j]:
                assert ch.rhs[j][d.NMU + i] == 0.0
        assert np.isnan(ch.zx[:d.NX]).all() and np.isfinite(ch.zx[d.NX:]).all()
    if not d.scalar:
        fixed = [ch for ch in chs if ch.cls == "fixed"]
        where = {j for ch in fixed for j in range(d.N) if ch.fix[j]}
        assert {0, d.CMID, d.N - 1} <= where and any(len(ch.fix[j]) == d.NX for ch in fixed for j in range(d.N))
        assert {ch.zero[0] for ch in chs if ch.zero} == {0, d.CMID, d.N - 1}


@pytest.mark.parametrize("name", SCALAR)
def test_scalar_chains_take_the_path_they_are_meant_for(name):
    """The host scan with the kernel's ok rule: every chain is accepted, or rejected, by a factor of
    at least MARGIN on the nearest threshold (MPCX_RCP is not an exact division).  Above one DPP
    row there is no scan.  The near-singular and the zero class must take the serial recurrence
    (from three lanes on: below, no leading minor but the matrix itself can be nearly singular)."""
    c = h.CHAIN_BY_NAME[name]
    d = h.cdims(c)
    seen = {}
    for ch in h.chains(c)[0]:
        a, b = h.scalar_ab(ch)
        took, margin = h.scan_margin(a, b)
        assert ("scan" if took else "serial") == ch.path and margin >= h.MARGIN, (ch.cls, ch.path, took, margin)
        seen.setdefault(ch.cls, set()).add(ch.path)
        if ch.cls == "zero":
            r, inertia = h.serial_restart(a, b)
            assert inertia == ch.inertia and all(r[z] == 0.0 for z in ch.zero)
            if not 0.0 < np.abs(a).max() < 1e-100:      # an exact zero: the recurrence's pivots are powers of two
                assert len(ch.zero) == 1 and a[ch.zero[0]] - b[ch.zero[0]] * (r[ch.zero[0] - 1] if ch.zero[0] else 0.0) == 0.0
    if d.N > 16:
        assert all(p == {"serial"} for p in seen.values())
    else:
        assert seen["dominant"] == seen["indefinite"] == seen["fixed"] == {"scan"}
        assert seen["zero"] == {"serial"}
        assert seen["near_singular"] == ({"serial"} if d.N >= 3 else {"scan"})
        assert seen["overflow"] == ({"scan", "serial"} if d.N >= 3 else {"scan"})
    zs = {ch.zero for ch in h.chains(c)[0] if ch.zero and not 0.0 < np.abs(h.scalar_ab(ch)[0]).max() < 1e-100}
    assert zs == {(0,), (d.N - 1,), (d.N // 2,)}


def _flat(d, pre=()):
    return (itertools.chain.from_iterable(_flat(v, pre + (k,)) for k, v in d.items())
            if isinstance(d, dict) else [(pre, d)])


def test_fp64_error_file_reproduces():
    """The recorded unit is what the restatements give here (the chains are seeded; BLAS and libm
    differences between machines stay far inside the factor)."""
    now = h.fp64_errors()
    assert set(now) == set(GOLD) == set(NAMES)
    a, b = dict(_flat(now)), dict(_flat(GOLD))
    assert set(a) == set(b)
    for key in a:
        print(key, a[key], b[key])
        assert a[key] <= h.bound(b[key]) and b[key] <= h.bound(a[key]), (key, a[key], b[key])
    for c in h.CHAIN_CONFIGS:
        assert set(GOLD[c.name]) == set(h.orders_of(c))
        for o in h.orders_of(c):
            assert set(GOLD[c.name][o]) == set(h.SCALAR_CLASSES if h.cdims(c).scalar else h.BLOCK_CLASSES)


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
@pytest.mark.parametrize("name", NAMES)
def test_harness_source_compiles_for_gfx950(name):
    """Device-only, with the static_asserts of the generated dimensions and of what the structure is
    in the harness for; both orders are compiled into an unflagged build."""
    c = h.CHAIN_BY_NAME[name]
    src = h.chain_source(c)
    wrappers = src.index("// generated by tests/ipm_chain_harness.py")
    assert src.count('#include "mpcx_ipm.hip"') == 1 and wrappers > src.index('#include "mpcx_ipm.hip"')
    assert src.count("static_assert(N == ") == 1 and "ipmla_chain" in src and "ipmla_filter" not in src
    path = h.build_chain(c)
    assert path.exists() and path.stat().st_size > 0


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def runs():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    done = {}

    def get(name, which):
        c = h.CHAIN_BY_NAME[name]
        if name not in done:
            done[name] = (h.Module(h.build_chain(c)), {})
        mod, per = done[name]
        if which not in per:
            per[which] = h.run_chain(mod, c, which)
        return per[which]
    return get


def _ratio(e, unit):
    return e / unit if unit else (0.0 if e == 0 else float("inf"))


def check_run(c, order, run):
    """One launch against the references; returns the worst kernel-to-unit ratio per class and kind."""
    d = h.cdims(c)
    chs, rst = h.chains(c)[0], h.restated(c)
    unit = GOLD[c.name][order]
    assert run.untouched, "bytes of LdsRest outside Dinv, xs, C, CW, CY, cperm, cpiv changed"
    assert run.padding
    assert (run.res[:, 3] == 1).all()
    bk = bool(c.defines)
    worst, ratio = {}, {}
    for idx, ch in enumerate(chs):
        got = tuple(int(v) for v in run.res[idx, :3])
        if ch.zero and bk and ch.zero[0] != d.N - 1:
            # bk_inverse divides by the zero pivot (tests/ipm_linalg_harness.py): what follows is not defined
            assert got[2] >= d.NC, (idx, got)
            continue
        assert got == ch.inertia == rst[idx][order][2], (ch.cls, idx, got, ch.inertia)
        if ch.zero and bk:
            continue
        dinv = run.dinv[idx]
        assert np.isfinite(dinv).all(), (ch.cls, idx)
        xs = None
        if not ch.zero:
            xs = run.xs[idx]
            assert np.isfinite(xs).all(), (ch.cls, idx, xs)
        elif d.scalar:       # a zero-pivot lane is exactly 0, the lanes after it the restarted recurrence
            assert all(dinv[z, 0, 0] == 0.0 for z in ch.zero), (idx, dinv.ravel())
        for kind, e in h.errors(c, idx, order, xs, dinv).items():
            slot = worst.setdefault(ch.cls, {})
            slot[kind] = max(slot.get(kind, 0.0), e)
    for cls, w in worst.items():
        ratio[cls] = {k: _ratio(e, unit[cls][k]) for k, e in w.items()}
    print(f"chain {c.name} {order}: kernel scaled error {worst}; ratio to the fp64 unit {ratio}")
    for cls, w in worst.items():
        for kind, e in w.items():
            assert e <= h.bound(unit[cls][kind]), (c.name, order, cls, kind, e, unit[cls][kind])
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCALAR)
def test_scalar_chain(name, runs):
    """The scan where its guard accepts it, the serial recurrence where it does not (near-singular
    leading minors, products that overflow inside the scan, exact zero pivots, above 16 lanes)."""
    c = h.CHAIN_BY_NAME[name]
    check_run(c, "serial", runs(name, 0))
    assert (runs(name, 1).res[:, 3] == 0).all()      # no twisted order for the scalar chain


@pytest.mark.gpu
@pytest.mark.parametrize("name", BLOCK)
def test_one_sided_block_chain(name, runs):
    """The general branch of ``chain_factor`` / ``chain_solve``; ``MPCX_CHAIN_BK``: its pivots through
    ``bk_factor`` + ``bk_inverse``, held to the unit of the host's sweep as the routines themselves are
    in tests/test_ipm_linalg.py."""
    check_run(h.CHAIN_BY_NAME[name], "one_sided", runs(name, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH_ORDERS)
def test_twisted_block_chain(name, runs):
    check_run(h.CHAIN_BY_NAME[name], "twisted", runs(name, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in BOTH_ORDERS if n.startswith("one_room_du")])
def test_both_orders_agree(name, runs):
    """One-sided against twisted on the same input: both meet the bound (the two tests above) and
    report the same inertia; the solutions agree to the sum of their bounds."""
    c = h.CHAIN_BY_NAME[name]
    a, b = runs(name, 0), runs(name, 1)
    assert np.array_equal(a.res[:, :3], b.res[:, :3])
    for idx, ch in enumerate(h.chains(c)[0]):
        if ch.zero:
            continue
        tol = sum(h.bound(GOLD[name][o][ch.cls]["xs"]) for o in h.ORDERS)
        scale = np.abs(a.xs[idx]).max()
        assert np.abs(a.xs[idx] - b.xs[idx]).max() <= 1.01 * tol * scale, (ch.cls, idx)
