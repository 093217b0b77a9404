"""The dense Bunch-Kaufman routines of the IPM kernel (csrc/ipm/bk.h, csrc/mpcx_ipm.hip) on the device, one routine at a time:
``bk_sweep``, ``bk_sweep2``, ``bk_factor`` + ``bk_inverse`` and ``interior_bk`` +
``trailing_backsolve`` against an mpmath reference (tests/ipm_linalg_harness.py: wrappers,
matrices, references, what is pinned at a zero pivot and why).

Tolerance: a result's scaled error (max |got - ref| / max |ref| of one matrix) stays within
FACTOR = 8 times the largest scaled error of the plain fp64 host restatement on the matrices of
the same class and size (tests/golden/ipm_linalg_fp64_error.json, regenerate with
``python -m tests.ipm_linalg_harness``) and is never held below 4 eps: the kernel's reciprocal
(MPCX_RCP), FMA contraction and a different but valid pivot at a near-tie move the error by small
factors, a wrong entry by many orders.  Inertia must match exactly.
"""

import itertools
import os
import shutil

import numpy as np
import pytest

from tests import ipm_linalg_harness as h

GOLD = h.golden()
HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
SWEEP_CASES = [(n, ld) for n in h.SWEEP_SIZES for ld in (n, n + 1)]


def inv_bound(n, cls):
    return h.bound(GOLD["inverse"][f"n{n}"][cls])


# ---------------------------------------------------------------------------
# CPU: the matrices, the restatements, the recorded unit, the build
# ---------------------------------------------------------------------------

def test_matrix_sets():
    """64 matrices per class (8 above n = 14); every matrix of the inertia set has its eigenvalues
    at least 1e-6 of the norm away from zero, except the zeros placed on purpose, which leave a
    separated remaining block."""
    for n in h.inverse_sizes() + [h.dims_of(c).NI for c in h.INTERIOR_CASES]:
        mats = h.matrices(n)
        assert len(mats) == len(h.CLASSES) * h.nmat(n)
        assert [m.cls for m in mats] == [c for c in h.CLASSES for _ in range(h.nmat(n))]
        for m in mats:
            assert np.array_equal(m.A, m.A.T)
            assert (m.cls in h.SINGULAR) == bool(m.zero)
            if m.inertia is None:
                assert m.cls == "extreme"
                continue
            keep = [i for i in range(n) if i not in m.zero]
            ev = np.linalg.eigvalsh(m.A[np.ix_(keep, keep)]) if keep else np.ones(1)
            assert np.abs(ev).min() >= h.SEPARATION * np.abs(ev).max()
            assert m.inertia == (int((ev > 0).sum()) if keep else 0, int((ev < 0).sum()) if keep else 0, len(m.zero))
            for z in m.zero:     # an exact zero or a pivot in (0, 1e-20]; nothing else in its row
                assert abs(m.A[z, z]) <= h.ZERO_PIVOT and not np.delete(m.A[z], z).any()
        tiny = [m for m in mats if m.cls == "zero_rowcol" and m.A[m.zero[0], m.zero[0]] != 0.0]
        assert tiny and len(tiny) < h.nmat(n)
        # most of the set decides the inertia
        assert sum(m.inertia is None for m in mats) <= h.nmat(n) // 3 + 1


@pytest.mark.parametrize("n", h.inverse_sizes())
def test_every_size_takes_every_branch(n):
    """The host sweep on the set of each size: 1x1 at k by the first and by the second test, 1x1
    at r, 2x2 (the last two need n >= 2, the second test n >= 3); its inertia is the reference's."""
    seen = {b for s in h.swept(n) for b in s[2]}
    want = {"k_first"} | ({"r", "2x2"} if n >= 2 else set()) | ({"k_second"} if n >= 3 else set())
    assert seen == want and want <= set(h.BRANCHES)
    for m, s in zip(h.matrices(n), h.swept(n)):
        if m.inertia is not None:
            assert s[1] == m.inertia, (m.cls, s[1], m.inertia)


@pytest.mark.parametrize("case", h.INTERIOR_CASES)
def test_interior_sets_take_every_branch(case):
    d = h.dims_of(case)
    rs = h.interior_restated(case)
    assert {b for r in rs for b in r[5]} == set(h.BRANCHES)
    for im, r in zip(h.images(case), rs):
        if im.mat.zero:
            # coupled stages: a singular interior is bad; independent stages count the zeros
            assert r[4] == (1 if d.NX > 0 else 0)
            if d.NX == 0:
                assert r[3] == im.mat.inertia
        else:
            assert r[4] == 0 and sorted(r[2]) == list(range(d.NI))
            if im.mat.inertia is not None:
                assert r[3] == im.mat.inertia
    # neighbours in launch order are of different classes
    assert all(a.mat.cls != b.mat.cls for a, b in zip(h.images(case), h.images(case)[1:]))


@pytest.mark.parametrize("n", [n for n in h.SWEEP_SIZES if n >= 2])
def test_sweep2_pairs_differ(n):
    """Pairs where one block takes 2x2 pivots and the other only 1x1, where one finishes in fewer
    rounds, and where only one has a zero pivot -- each both ways round; one pair in eight sweeps
    A alone."""
    sw, mats = h.swept(n), h.matrices(n)
    seen = set()
    for a, b, twob in h.sweep2_pairs(n):
        if not twob:
            seen.add("alone")
            continue
        ba, bb = sw[a][2], sw[b][2]
        for x, y, tag in ((ba, bb, "A"), (bb, ba, "B")):
            if "2x2" in x and "2x2" not in y:
                seen.add(f"2x2 in {tag} only")
            if len(x) < len(y):
                seen.add(f"{tag} done first")
        if bool(mats[a].zero) != bool(mats[b].zero):
            seen.add("zero in " + ("A" if mats[a].zero else "B") + " only")
    assert seen == {"alone", "2x2 in A only", "2x2 in B only", "A done first", "B done first",
                    "zero in A only", "zero in B only"}
    assert sorted(a for a, _, _ in h.sweep2_pairs(n)) == sorted({b for _, b, _ in h.sweep2_pairs(n)})


def test_fp64_error_file_reproduces():
    """The recorded unit is what the restatements give here (the matrices are seeded; BLAS and
    libm differences between machines stay far inside the factor)."""
    now = h.fp64_errors()
    assert set(now) == set(GOLD) == {"inverse", "interior"}
    assert set(now["inverse"]) == set(GOLD["inverse"]) == {f"n{n}" for n in h.inverse_sizes()}
    assert set(now["interior"]) == set(GOLD["interior"]) == set(h.INTERIOR_CASES)
    flat = lambda d, pre=(): (itertools.chain.from_iterable(flat(v, pre + (k,)) for k, v in d.items())
                              if isinstance(d, dict) else [(pre, d)])
    a, b = dict(flat(now)), dict(flat(GOLD))
    assert set(a) == set(b)
    for key in a:
        print(key, a[key], b[key])
        assert a[key] <= h.bound(b[key]) and b[key] <= h.bound(a[key]), (key, a[key], b[key])
    for n in h.inverse_sizes():
        assert set(GOLD["inverse"][f"n{n}"]) == set(h.CLASSES)
    for case in h.INTERIOR_CASES:
        assert set(GOLD["interior"][case]) == set(h.CLASSES) - set(h.SINGULAR)


def test_structures_of_the_harness():
    d = {c: h.dims_of(c) for c in h.INTERIOR_CASES}
    assert d["exchange_supply"].NX == 0 and d["rng_room_mpc"].NC > d["rng_room_mpc"].NX
    nb = {name: (lambda g: g["NV"] + g["NX"] + g["NG"])(h.case_gen(name).dims) for name in h.configs.CASES}
    assert max(nb, key=nb.get) == h.LARGEST_BLOCK_CASE and h.block_case_size() == (36, 37)
    assert {c.case for c in h.CONFIGS} == set(h.INTERIOR_CASES) | {h.LARGEST_BLOCK_CASE}


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
@pytest.mark.parametrize("name", list(h.BY_NAME))
def test_harness_source_compiles_for_gfx950(name):
    """Device-only, with the static_assert of what the structure is in the harness for.  The
    model-free source: csrc/ipm/wave.h and csrc/ipm/bk.h compile, and the four routines of bk.h
    instantiate, in a translation unit that includes nothing else of the kernel and defines no
    ``MPCX_*`` dimension (the reciprocal ``MPCX_RCP`` is the code generator's)."""
    import re

    c = h.BY_NAME[name]
    src = h.source(c)
    wrappers = src.index("// generated by tests/ipm_linalg_harness.py")
    if c.case is None:
        assert tuple(re.findall(r'#include [<"]([^>"]+)[>"]', src)) == h.DENSE_INCLUDES
        assert wrappers > src.index('#include "ipm/bk.h"') > src.index('#include "ipm/wave.h"')
        assert set(re.findall(r"#define (MPCX_\w+)", src)) == {"MPCX_RCP"} and "ipmla_consts" not in src
        assert all(f"{r}<" in src for r in ("bk_sweep", "bk_sweep2", "bk_factor", "bk_inverse"))
        assert {(n, ld) for n in h.SWEEP_SIZES for ld in (n, n + 1)} == set(c.sweeps)
        assert {(n, n) for n in h.FACTOR_SIZES} == set(c.factors)
    else:
        assert src.count('#include "mpcx_ipm.hip"') == 1 and wrappers > src.index('#include "mpcx_ipm.hip"')
        assert src.index("ipmla_consts") > wrappers and not c.sweeps
    assert ("ipmla_interior" in src) == c.interior
    path = h.build(c)
    assert path.exists() and path.stat().st_size > 0
    assert h.build_launcher().exists()


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def modules():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    loaded = {}

    def get(name):
        if name not in loaded:
            loaded[name] = h.Module(h.build(h.BY_NAME[name]))
        return loaded[name]
    return get


SENT = np.full(h.GUARD, h.SENTINEL)
ISENT = np.full(h.GUARD, h.ISENTINEL)


def _images(back, n, ld):
    """[nb, n*ld + GUARD] -> (matrices [nb, n, n], pad column [nb, n, ld - n], guards [nb, GUARD])."""
    body = back[:, :n * ld].reshape(len(back), n, ld)
    return body[:, :, :n], body[:, :, n:], back[:, n * ld:]


def check_inverse(n, idx, got, worst):
    """One produced inverse of ``matrices(n)[idx]`` against the reference; the zero pivots' rows
    and columns exactly 0, every entry finite."""
    m = h.matrices(n)[idx]
    assert np.isfinite(got).all(), (m.cls, idx, got)
    for z in m.zero:
        assert not got[z, :].any() and not got[:, z].any(), (m.cls, idx, got)
    e = h.scaled_error(got, h.inverse_refs(n)[idx])
    worst[m.cls] = max(worst.get(m.cls, 0.0), e)
    assert e <= inv_bound(n, m.cls), (n, m.cls, idx, e, inv_bound(n, m.cls))


def _ratio(e, unit):
    return e / unit if unit else (0.0 if e == 0 else float("inf"))


def report(what, n, worst):
    unit = GOLD["inverse"][f"n{n}"]
    ratio = {c: _ratio(e, unit[c]) for c, e in worst.items()}
    print(f"{what} n={n}: kernel scaled error {worst}; ratio to the fp64 unit {ratio}")


@pytest.mark.gpu
@pytest.mark.parametrize("n,ld", SWEEP_CASES)
def test_bk_sweep(n, ld, modules):
    mats = h.matrices(n)
    ab, ob, res = h.run_sweep(modules(h.DENSE.name), n, ld, [m.A for m in mats])
    _, apad, aguard = _images(ab, n, ld)
    out, opad, oguard = _images(ob, n, ld)
    assert np.array_equal(aguard, np.tile(SENT, (len(mats), 1))) and np.array_equal(oguard, aguard)
    assert (apad == h.PAD).all() and np.isnan(opad).all()
    worst = {}
    for idx, m in enumerate(mats):
        check_inverse(n, idx, out[idx], worst)
        assert res[idx, 3] == 0 and res[idx, :3].sum() == n
        if m.inertia is not None:
            assert tuple(res[idx, :3]) == m.inertia, (m.cls, idx, res[idx], m.inertia)
    report("bk_sweep", n, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("n,ld", SWEEP_CASES)
def test_bk_sweep2(n, ld, modules):
    """Two different blocks per call, each in place; a call with twob false leaves B bit-identical.
    The inertia returned is the sum over the blocks swept."""
    mats, pairs = h.matrices(n), h.sweep2_pairs(n)
    A = [mats[a].A for a, _, _ in pairs]
    B = [mats[b].A for _, b, _ in pairs]
    ab, bb, res = h.run_sweep2(modules(h.DENSE.name), n, ld, A, B, [int(t) for _, _, t in pairs])
    ga, apad, aguard = _images(ab, n, ld)
    gb, bpad, bguard = _images(bb, n, ld)
    assert np.array_equal(aguard, np.tile(SENT, (len(pairs), 1))) and np.array_equal(bguard, aguard)
    assert (apad == h.PAD).all() and (bpad == h.PAD).all()
    worst = {}
    for q, (a, b, twob) in enumerate(pairs):
        check_inverse(n, a, ga[q], worst)
        want = mats[a].inertia
        if twob:
            check_inverse(n, b, gb[q], worst)
            want = None if want is None or mats[b].inertia is None else tuple(np.add(want, mats[b].inertia))
        else:
            assert np.array_equal(gb[q].view(np.int64), mats[b].A.view(np.int64)), (q, gb[q], mats[b].A)
        assert res[q, :3].sum() == (2 * n if twob else n)
        if want is not None:
            assert tuple(res[q, :3]) == want, (q, a, b, twob, res[q], want)
    report("bk_sweep2", n, worst)


def check_factor(n, ld, db, ib, res):
    mats = h.matrices(n)
    nb = len(mats)
    for arr in range(4):     # A (factored) | W | Y | out: guards untouched
        assert np.array_equal(db[:, arr, n * ld:], np.tile(SENT, (nb, 1))), arr
    assert np.array_equal(ib[:, 0, n:], np.tile(ISENT, (nb, 1))) and np.array_equal(ib[:, 1, n:], ib[:, 0, n:])
    _, apad, _ = _images(db[:, 0], n, ld)
    out, opad, _ = _images(db[:, 3], n, ld)
    assert (apad == h.PAD).all() and np.isnan(opad).all()
    worst = {}
    for idx, m in enumerate(mats):
        perm, piv = ib[idx, 0, :n], ib[idx, 1, :n]
        assert sorted(perm) == list(range(n)), (idx, perm)
        k = 0
        while k < n:         # 1, or 2 followed by 0
            assert piv[k] in (1, 2) and (piv[k] == 1 or (k + 1 < n and piv[k + 1] == 0)), (idx, piv)
            k += piv[k]
        assert res[idx, 3] == 0 and res[idx, :3].sum() == n
        if m.inertia is not None:
            assert tuple(res[idx, :3]) == m.inertia, (m.cls, idx, res[idx], m.inertia)
        if not m.zero:       # a counted zero pivot: the callers discard the inverse (harness docstring)
            check_inverse(n, idx, out[idx], worst)
    report("bk_factor + bk_inverse", n, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("n", h.FACTOR_SIZES)
def test_bk_factor_inverse(n, modules):
    db, ib, res = h.run_factor(modules(h.DENSE.name), n, n, [m.A for m in h.matrices(n)])
    check_factor(n, n, db, ib, res)


@pytest.mark.gpu
def test_bk_factor_inverse_at_the_largest_block(modules):
    """NB x LDB of the structure with the largest block-chain block (36 x 37)."""
    n, ld = h.block_case_size()
    mod = modules(h.LARGEST_BLOCK_CASE)
    k = mod.consts()
    assert (k["NB"], k["LDB"]) == (n, ld)
    db, ib, res = h.run_factor(mod, n, ld, [m.A for m in h.matrices(n)], kernel=h.kernel_name("factor", "NB", "LDB"))
    check_factor(n, ld, db, ib, res)


@pytest.mark.gpu
@pytest.mark.parametrize("case", h.INTERIOR_CASES)
def test_interior_bk_and_trailing_backsolve(case, modules):
    """Per stage image [[A, B^T], [B, T]]: the trailing block becomes T - B A^-1 B^T, the trailing
    rows' interior columns B A^-1 in the pivot order perm, the inertia that of A.  A singular
    interior ends bad where stages are coupled (its neighbours in the wave run on) and is counted
    where they are not."""
    mod = modules(case)
    d, k = h.dims_of(case), mod.consts()
    assert (k["NX"], k["NI"], k["NC"], k["NLOC"], k["NTR"], k["PKS"]) == (d.NX, d.NI, d.NC, d.NLOC, d.NTR, d.PKS)
    F, fguard, perm, piv, iguard, res, nimg = h.run_interior(mod, case, k["G"])
    ns = 64 // k["G"]
    assert np.array_equal(fguard, np.tile(SENT, (len(fguard), 1)))
    assert np.array_equal(iguard, np.tile(ISENT, (len(iguard), 2, 1)))
    assert (F[:, d.PKB:] == h.PAD).all()
    ims, unit = h.images(case), GOLD["interior"][case]
    worst = {}
    for idx in range(len(F)):
        im = ims[idx % nimg]
        m = im.mat
        if m.zero:
            if d.NX > 0:
                assert res[idx, 3] == 1, (idx, m.cls, res[idx])
            else:
                assert tuple(res[idx]) == m.inertia + (0,), (idx, m.cls, res[idx], m.inertia)
            continue
        assert res[idx, 3] == 0 and res[idx, :3].sum() == d.NI, (idx, m.cls, res[idx])
        if m.inertia is not None:
            assert tuple(res[idx, :3]) == m.inertia, (idx, m.cls, res[idx], m.inertia)
        assert sorted(perm[idx]) == list(range(d.NI)), (idx, perm[idx])
        j = 0
        while j < d.NI:
            assert piv[idx, j] in (1, 2) and (piv[idx, j] == 1 or (j + 1 < d.NI and piv[idx, j + 1] == 0)), (idx, piv[idx])
            j += piv[idx, j]
        T, Z = h.unpack_trailing(F[idx], d)
        assert np.isfinite(Z).all() and np.isfinite(T[h.trailing_mask(d)]).all(), (idx, m.cls)
        for kind, e in h.interior_errors(case, idx % nimg, T, Z, perm[idx]).items():
            slot = worst.setdefault(m.cls, {})
            slot[kind] = max(slot.get(kind, 0.0), e)
            assert e <= h.bound(unit[m.cls][kind]), (idx, m.cls, kind, e, unit[m.cls][kind])
    ratio = {c: {kd: _ratio(e, unit[c][kd]) for kd, e in w.items()} for c, w in worst.items()}
    print(f"interior {case}: kernel scaled error {worst}; ratio to the fp64 unit {ratio}")
    if d.NX > 0 and ns > 1:      # a wave with a bad group between groups that ran on
        bad = res[:, 3].reshape(-1, ns)
        assert ((bad == 1).any(axis=1) & (bad == 0).any(axis=1)).any()
    assert d.NX == 0 or ns > 1
