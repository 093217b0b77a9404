"""bench.py ``--dump-outputs`` (CPU): the arrays of the last timed step are written as float64
``.npy`` files, one ``mpcx_stats`` field per ``stats`` column, and a fleet past the size limit is
cut to the same seeded rows of every array on every run."""

import numpy as np
import torch

import bench
from agentlib_mpc_amd.runtime.native import _STATS_DOUBLES, _STATS_INTS, STATS_BYTES, stats_array


def _fleet(n, nw=7, ng=5, seed=3):
    rng = np.random.default_rng(seed)
    w = torch.from_numpy(rng.normal(size=(n, nw)))
    lam = torch.from_numpy(rng.normal(size=(n, ng)))
    rec = np.zeros(n, dtype=stats_array(np.zeros(STATS_BYTES, np.uint8)).dtype)
    rec["obj"] = rng.normal(size=n)
    rec["iter_count"] = rng.integers(0, 100, n)
    rec["status"] = rng.integers(0, 3, n)
    return w, lam, rec


def test_dump_outputs_writes_float64_arrays(tmp_path):
    w, lam, rec = _fleet(33)
    bench.dump_outputs(str(tmp_path / "out"), 0, w, lam, rec.view(np.uint8))
    got = {p.name: np.load(p) for p in sorted((tmp_path / "out").iterdir())}
    assert sorted(got) == ["lam_g.npy", "stats.npy", "w.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["w.npy"], w.numpy())
    assert np.array_equal(got["lam_g.npy"], lam.numpy())
    names = _STATS_DOUBLES + _STATS_INTS
    assert got["stats.npy"].shape == (33, len(names))
    for col in ("obj", "iter_count", "status"):
        assert np.array_equal(got["stats.npy"][:, names.index(col)], rec[col].astype(np.float64))


def test_dump_outputs_of_other_ranks_do_not_collide(tmp_path):
    w, lam, rec = _fleet(4)
    bench.dump_outputs(str(tmp_path), 0, w, lam, rec.view(np.uint8))
    bench.dump_outputs(str(tmp_path), 2, w, lam, rec.view(np.uint8))
    assert sorted(p.name for p in tmp_path.iterdir()) == [
        "lam_g.npy", "lam_g.rank2.npy", "stats.npy", "stats.rank2.npy", "w.npy", "w.rank2.npy"]


def test_dump_outputs_samples_a_fleet_past_the_limit(tmp_path, monkeypatch):
    n = 200
    w, lam, rec = _fleet(n)
    row_bytes = 8 * (w.shape[1] + lam.shape[1] + len(rec.dtype.names))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 50 * row_bytes + 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, w, lam, rec.view(np.uint8))
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("w", "lam_g", "stats")}
    b = {k: np.load(tmp_path / "b" / f"{k}.npy") for k in ("w", "lam_g", "stats")}
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert all(len(v) == 50 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 50 * row_bytes + 3
    # the same agents in every array, in fleet order
    rows = [int(np.flatnonzero((w.numpy() == r).all(axis=1))[0]) for r in a["w"]]
    assert rows == sorted(rows) and len(set(rows)) == 50
    assert np.array_equal(a["lam_g"], lam.numpy()[rows])
    assert np.array_equal(a["stats"][:, 0], rec["obj"][rows])

