"""The IPM kernel's filter lists on the device, alone: ``filter_insert`` with ``spill_prune`` and
``spill_shift``, and ``spill_dominates``, driven by lists of operations (tests/ipm_chain_harness.py:
the wrapper, the reference list).  The parity cases hold at most 22 filter entries, so no chunk of
the spill list beyond the first 64 lanes ever ran there and the shipped parts (48 entries in LDS,
976 in the spill list) never spilled at all.

The reference is an ordered list: an insertion drops every entry it dominates (ties included),
appends, and at capacity drops the oldest entry, counted; the device's spill list followed by its
LDS part is that list.  Equality is exact, bit for bit; the workspace slab outside the two spill
tiers keeps its sentinel.
"""

import os
import shutil

import numpy as np
import pytest

from tests import ipm_chain_harness as h
from tests.ipm_chain_harness import OP_INSERT, OP_QUERY, OP_SNAP, OP_TIER

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
BUILDS = list(h.FILTER_BUILDS)
CROSSINGS = (63, 64, 65, 128, 129)     # spill-list lengths either side of a chunk of 64 lanes


def staircase(n, base=0.0):
    """Mutually non-dominating entries, theta strictly decreasing and phi strictly increasing:
    entry i = (base + n - i, base + i)."""
    return [(OP_INSERT, base + n - i, base + float(i)) for i in range(n)]


def snap(op):
    return (op[0] | OP_SNAP, op[1], op[2])


def every(ops, k):
    return [snap(o) if (i + 1) % k == 0 or i + 1 == len(ops) else o for i, o in enumerate(ops)]


def seq_staircase(maxf, fspill):
    """Long enough that the spill list crosses 63, 64, 65, 128 and 129 entries, a snapshot at each."""
    ops = staircase(maxf + 140)
    return [snap(o) if (i + 1 - maxf) in CROSSINGS else o for i, o in enumerate(ops)][:-1] + [snap(ops[-1])]


def seq_dominating(maxf, fspill, which):
    """A staircase of maxf + 140 entries (entry i dominated by (th, ph) iff ph <= i <= L - th), then
    one insertion that dominates a band of it, ties at both ends of the band, then queries that tie
    with a spill entry, miss every entry, or are dominated by the inserted one."""
    L = maxf + 140
    ns = L - maxf
    lo, hi = {"chunk": (10, 20), "straddle": (60, 130), "oldest": (0, 0), "newest": (ns - 1, ns - 1),
              "spill": (0, ns - 1), "all": (0, L - 1)}[which]
    ops = staircase(L)
    ops[-1] = snap(ops[-1])
    ops.append((OP_INSERT | OP_SNAP, float(L - hi), float(lo)))
    for i in (0, 5, 63, 64, 127, 128, ns - 1, ns, L - 1):
        ops.append((OP_QUERY, float(L - i), float(i)))             # equal to entry i (if it is still there)
        ops.append((OP_QUERY, L - i - 0.5, i + 0.5))               # between entries: dominated by none of the staircase
        ops.append((OP_QUERY, L - i + 0.5, i + 0.5))
    ops.append(snap(ops.pop()))
    return ops


def seq_overflow(maxf, fspill):
    """70 insertions past the capacity: the final list is the last maxf + fspill entries."""
    return every(staircase(maxf + fspill + 70), 64)


def seq_tiers(maxf, fspill):
    """Tier 0 filled past one chunk, then work on tier 1 (its own staircase, a dominating band,
    queries that tier 0's entries would dominate), then back."""
    n = maxf + 70
    ops = staircase(n)
    ops[-1] = snap(ops[-1])
    ops.append((OP_QUERY, 500.0, 500.0))                          # dominated by tier 0's spill entries
    ops.append((OP_TIER | OP_SNAP, 1.0, 0.0))
    ops.append((OP_QUERY, 500.0, 500.0))                          # tier 1 is empty
    ops += every(staircase(n, base=1000.0), 16)
    ops.append((OP_QUERY | OP_SNAP, 500.0, 500.0))                # below every entry of tier 1
    ops.append((OP_QUERY, 5000.0, 5000.0))
    ops.append((OP_INSERT | OP_SNAP, 1000.0 + n - 66, 1003.0))    # a band across entry 64 of tier 1
    ops.append((OP_TIER | OP_SNAP, 0.0, 0.0))
    ops.append((OP_QUERY, 500.0, 500.0))
    ops.append((OP_INSERT | OP_SNAP, 0.5, n + 1.0))               # dominates nothing of tier 0, appended
    return ops


def seq_random(maxf, fspill, n=2000):
    """Values on a grid of sixteenths near an anti-diagonal 400 steps long: fronts of a few hundred
    entries, frequent ties."""
    rng = np.random.default_rng(h.name_seed("ipm_filter random"))
    ops, tier = [], 0
    for _ in range(n):
        u = rng.uniform()
        k = int(rng.integers(0, 400))
        th, ph = k / 16.0, (400 - k + int(rng.integers(-2, 3))) / 16.0
        if u < 0.70:
            ops.append((OP_INSERT, th, ph))
        elif u < 0.995:
            ops.append((OP_QUERY, th + int(rng.integers(0, 2)) / 16.0, ph))
        else:
            tier = 1 - tier
            ops.append((OP_TIER, float(tier), 0.0))
    return ops


def seq_nonfinite(maxf, fspill):
    inf, nan = float("inf"), float("nan")
    ops = staircase(maxf + 70)
    for th, ph in ((nan, 1e9), (1e9, nan), (nan, nan), (inf, inf), (-inf, 1e9), (inf, -inf), (1e9, inf), (-inf, -inf)):
        ops.append((OP_QUERY, th, ph))
    ops.append(snap(ops.pop()))
    return ops


SEQUENCES = {
    "staircase": seq_staircase,
    **{f"dominating_{w}": (lambda m, f, w=w: seq_dominating(m, f, w))
       for w in ("chunk", "straddle", "oldest", "newest", "spill", "all")},
    "overflow": seq_overflow,
    "tiers": seq_tiers,
    "random": seq_random,
    "nonfinite": seq_nonfinite,
}


def ops_of(build, seq):
    maxf, fspill = h.FILTER_PARTS[build]
    ops = SEQUENCES[seq](maxf, fspill)
    if seq == "random":     # a snapshot after every operation on the small builds, every 64th on the shipped one
        ops = every(ops, 64 if build == "shipped" else 1)
    return ops


# ---------------------------------------------------------------------------
# CPU: the reference and what the sequences reach
# ---------------------------------------------------------------------------

def test_filter_builds():
    assert h.FILTER_BUILDS["shipped"] == () and h.FILTER_PARTS["shipped"] == (48, 976)
    assert h.FILTER_BUILDS["spill"] == ("MPCX_MAXF=8",) and h.FILTER_BUILDS["capped"] == ("MPCX_MAXF=8", "MPCX_FSPILL=4")
    for build, (maxf, fspill) in h.FILTER_PARTS.items():
        defs = dict(d.split("=") for d in h.FILTER_BUILDS[build])
        assert maxf == int(defs.get("MPCX_MAXF", 48)) and fspill == int(defs.get("MPCX_FSPILL", 1024 - maxf))


@pytest.mark.parametrize("build", BUILDS)
def test_reference_is_the_ordered_list(build):
    """The reference keeps the kernel's split into a spill list and an LDS part; joined, they are the
    one ordered list of the plain rule on every single-tier sequence."""
    maxf, fspill = h.FILTER_PARTS[build]
    for seq in SEQUENCES:
        ops = [o for o in ops_of(build, seq)]
        if any((o[0] & 7) == OP_TIER for o in ops):
            continue
        snaps, _ = h.replay(build, ops)
        plain = h.simple_filter(maxf + fspill, ops)
        assert len(snaps) == len(plain) > 0
        for (tier, lds, sp, over), (cur, dropped) in zip(snaps, plain):
            assert tier == 0 and sp[0] + lds == cur and over == dropped and len(lds) <= maxf and len(sp[0]) <= fspill


def test_sequences_reach_what_they_are_for():
    """On the shipped parts: the spill list crosses every chunk boundary with a snapshot there; each
    dominating insertion removes exactly its band; 70 entries are dropped past 1024; the random
    sequence spills past two chunks, ties occur, and every query answer occurs."""
    maxf, fspill = h.FILTER_PARTS["shipped"]
    snaps, _ = h.replay("shipped", ops_of("shipped", "staircase"))
    assert [len(s[2][0]) for s in snaps][:5] == list(CROSSINGS)
    L, ns = maxf + 140, 140
    removed = {"chunk": range(10, 21), "straddle": range(60, 131), "oldest": range(0, 1), "newest": range(ns - 1, ns),
               "spill": range(0, ns), "all": range(0, L)}
    for w, band in removed.items():
        (_, lds0, sp0, _), (_, lds1, sp1, _) = h.replay("shipped", ops_of("shipped", f"dominating_{w}"))[0][:2]
        before = sp0[0] + lds0
        want = [e for i, e in enumerate(before) if i not in band] + [(float(L - band[-1]), float(band[0]))]
        assert sp1[0] + lds1 == want, w
    assert [e for i, e in enumerate(before) if i in removed["oldest"]] == [(float(L), 0.0)]   # equal to the inserted one
    snaps, _ = h.replay("shipped", ops_of("shipped", "overflow"))
    stairs = [(o[1], o[2]) for o in ops_of("shipped", "overflow")]
    assert snaps[-1][3] == 70 and snaps[-1][2][0] + snaps[-1][1] == stairs[-1024:]
    ops = ops_of("shipped", "random")
    snaps, answers = h.replay("shipped", ops)
    assert len(ops) == 2000 and max(len(s[2][0]) for s in snaps) > 128 and max(len(s[2][1]) for s in snaps) > 0
    assert set(answers.values()) == {True, False}
    ins = [(o[1], o[2]) for o in ops if (o[0] & 7) == OP_INSERT]
    assert len(set(ins)) < len(ins)
    snaps, answers = h.replay("shipped", ops_of("shipped", "tiers"))
    q = [a for _, a in sorted(answers.items())]
    assert q == [True, False, False, True, True]
    _, answers = h.replay("shipped", ops_of("shipped", "nonfinite"))
    assert [a for _, a in sorted(answers.items())] == [False, False, False, True, False, False, True, False]


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
@pytest.mark.parametrize("build", BUILDS)
def test_harness_source_compiles_for_gfx950(build):
    src = h.filter_source(build)
    assert src.count('#include "mpcx_ipm.hip"') == 1 and "ipmla_filter" in src and "ipmla_chain" not in src
    path = h.build_filter(build)
    assert path.exists() and path.stat().st_size > 0


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def modules():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    loaded = {}

    def get(build):
        if build not in loaded:
            loaded[build] = h.Module(h.build_filter(build))
        return loaded[build]
    return get


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def check_filter(build, ops, mod):
    maxf, fspill = h.FILTER_PARTS[build]
    K = h.consts(mod)
    assert (K["MAXF"], K["FSPILL"]) == (maxf, fspill)
    got, answers, untouched = h.run_filter(mod, ops)
    want, wanswers = h.replay(build, ops)
    assert untouched, "the slab outside the two spill tiers lost its sentinel"
    assert len(got) == len(want) > 0
    frozen = None      # tier 0's spill bytes while tier 1 is worked on
    for q, (g, (tier, lds, sp, over)) in enumerate(zip(got, want)):
        assert g["nfilt"] == len(lds) and g["nsp"] == (len(sp[0]), len(sp[1])) and g["over"] == over, \
            (q, g["nfilt"], g["nsp"], g["over"], len(lds), len(sp[0]), len(sp[1]), over)
        assert np.array_equal(_bits(g["fth"][:len(lds)]), _bits([e[0] for e in lds])), (q, "fth")
        assert np.array_equal(_bits(g["fph"][:len(lds)]), _bits([e[1] for e in lds])), (q, "fph")
        for t in (0, 1):
            assert np.array_equal(_bits(g["spill"][t, 0, :len(sp[t])]), _bits([e[0] for e in sp[t]])), (q, t, "theta")
            assert np.array_equal(_bits(g["spill"][t, 1, :len(sp[t])]), _bits([e[1] for e in sp[t]])), (q, t, "phi")
        if tier % 2 == 1:     # every byte of tier 0 stays as it is while tier 1 is worked on
            if frozen is None or frozen[0] != tier:
                frozen = (tier, _bits(g["spill"][0]).copy())
            assert np.array_equal(_bits(g["spill"][0]), frozen[1]), (q, "tier 0 written while tier 1 is current")
    assert answers == wanswers, {i: (answers[i], wanswers[i]) for i in answers if answers[i] != wanswers[i]}
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("seq", list(SEQUENCES))
@pytest.mark.parametrize("build", BUILDS)
def test_filter_lists(build, seq, modules):
    got = check_filter(build, ops_of(build, seq), modules(build))
    if seq == "overflow":
        maxf, fspill = h.FILTER_PARTS[build]
        assert got[-1]["over"] == 70 and got[-1]["nfilt"] == maxf and got[-1]["nsp"][0] == fspill
    print(f"filter {build} {seq}: {len(got)} snapshots, final nfilt {got[-1]['nfilt']}, nsp {got[-1]['nsp']}, "
          f"dropped {got[-1]['over']}")
