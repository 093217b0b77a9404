"""Generate tests/golden/cia_room.json: the CIA backend's three steps on the cooler room, done on
the CPU with the oracle (oracle/ipm.py on the hand-written NLP of tests/cia_cases.py) and the numpy
restatement of the rounding.

    python tests/golden/make_cia_goldens.py

Per case and call it records the inputs, the relaxed optimum with status and iteration count, the
relaxed binary controls, eta and the next-best eta over all assignments, the rounded controls, and
the fixed optimum with status and iteration count.  The second call of a case starts from the first
call's fixed optimum with a new measured temperature, the way the backend warm-starts.

A case is written only if it can serve as a parity case (checked here, on the oracle alone): both
solves of every call end ``Solve_Succeeded``, and the next-best eta is at least 1e-3 intervals away,
so that a 1e-5 difference in the relaxed controls cannot change the rounding.  At least one case
must have two or more relaxed controls strictly inside (0.05, 0.95).
"""

from __future__ import annotations

import dataclasses
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for _p in (ROOT, ROOT / "agentlib-mpc_amd"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

from oracle import ipm  # noqa: E402
from tests import cia_cases as cc  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent / "cia_room.json"
TS = 300.0
#: the oracle's own defaults, written out in full so that the backend under test gets every one of
#: them.  (With the reference's solver settings -- tol 1e-4, acceptable_tol 0.1 after 5 iterations --
#: the fixed solve of the example ends Solved_To_Acceptable_Level after 31 iterations: not a case.)
ORACLE_DEFAULTS = dict(tol=1e-8, max_iter=3000, acceptable_tol=1e-6, acceptable_iter=15,
                       acceptable_constr_viol_tol=1e-2, acceptable_compl_inf_tol=1e-2)
#: (name, N, model values, solver options, measured temperature of each call)
CASES = [
    ("n4_heavy_slack", 4, dict(s_T=30.0), dict(ORACLE_DEFAULTS, acceptable_iter=0), [298.16, 297.6]),
    ("n10_example", 10, dict(), dict(ORACLE_DEFAULTS), [298.16, 297.9]),
]
MIN_GAP = 1e-3


def _solve(prob, p, w0, lbw, ubw, opts):
    r = ipm.solve(prob.functions(p), w0, lbw, ubw, prob.lbg(p), prob.ubg(p), ipm.IPMOptions(**opts))
    return r, {"status": r.status, "iterations": int(r.iterations), "f": float(r.f), "x": r.x.tolist(),
               "n_resto": int(r.n_resto)}


def run_case(name, N, values, opts, temperatures):
    prob = cc.cooler_room(N=N, ts=TS)
    pos = cc.cooler_room_binary_positions(prob)[0]
    calls, w_start = [], None
    for T0 in temperatures:
        p, lbw, ubw, w0 = cc.cooler_room_inputs(prob, N=N, T0=T0, **values)
        if w_start is not None:  # the previous call's fixed optimum, the initial state from its parameter
            w0 = w_start.copy()
            w0[0] = T0
        rel, rel_rec = _solve(prob, p, w0, lbw, ubw, opts)
        b_rel = rel.x[pos]
        rd = cc.round_batch(b_rel[None, None, :], TS)
        b, bad = cc.modes(b_rel[None, None, :])
        etas = cc.enumerate_eta(b[0], n_best=2)
        if rd["status"][0] != cc.OK or rd["eta"][0] != TS * etas[0]:
            return None, f"rounding failed ({rd['status'][0]})"
        B = rd["b_bin"][0, 0]
        lfix, ufix = lbw.copy(), ubw.copy()
        lfix[pos] = ufix[pos] = B
        fix, fix_rec = _solve(prob, p, rel.x.copy(), lfix, ufix, opts)
        calls.append({"T0": T0, "p": p.tolist(), "lbw": lbw.tolist(), "ubw": ubw.tolist(), "w0": w0.tolist(),
                      "relaxed": rel_rec, "b_rel": b_rel.tolist(), "eta": float(rd["eta"][0]),
                      "eta_intervals": etas[0], "eta_next_intervals": etas[1] if len(etas) > 1 else None,
                      "b_bin": B.tolist(), "fixed": fix_rec})
        print(f"  {name} T0={T0}: relaxed {rel.status} {rel.iterations} it, b_rel {np.round(b_rel, 3)}, "
              f"eta {etas[0]:.4f} (next {etas[1] if len(etas) > 1 else None}), B {B.astype(int)}, "
              f"fixed {fix.status} {fix.iterations} it")
        if rel.status != "Solve_Succeeded" or fix.status != "Solve_Succeeded":
            return None, "a solve did not end Solve_Succeeded"
        if len(etas) > 1 and etas[1] - etas[0] < MIN_GAP:
            return None, f"next-best eta only {etas[1] - etas[0]:.2e} intervals away"
        w_start = fix.x
    return {"name": name, "N": N, "time_step": TS, "values": values, "options": opts, "calls": calls}, None


def main():
    kept = []
    for case in CASES:
        rec, why = run_case(*case)
        if rec is None:
            print(f"dropped {case[0]}: {why}")
        else:
            kept.append(rec)
    inner = [sum(0.05 < v < 0.95 for v in c["b_rel"]) for rec in kept for c in rec["calls"]]
    assert kept and max(inner) >= 2, "no case with two relaxed controls strictly inside (0.05, 0.95)"
    OUT.write_text(json.dumps({"cases": kept}, indent=1) + "\n")
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(kept)} cases)")


if __name__ == "__main__":
    main()
