"""Measurement (GPU): the three legs of one CIA backend step for a fleet of cooler rooms
(``benchmarks.one_room_cia``, N = 10, the reference's solver settings), and what the rounding would
cost through the host.  One process, inputs uploaded once, HIP events on the launch stream:

* the relaxed solve (``mpcx_batch_solve``),
* the rounding launch (``mpcx_cia_round``),
* the fixed solve, started from the relaxed optimum,
* for comparison the same rounding done through the host: the solutions copied to the host, the
  numpy restatement of the rounding (tests/cia_cases.round_batch, the fastest host statement this
  tree has: vectorised over the agents), the fixed bounds copied back -- a host clock around work
  that ends in a device synchronise.

``python scripts/cia_leg.py [--agents 4096] [--repeats 10]`` prints one JSON line (medians, ms)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "agentlib-mpc_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--horizon", type=int, default=10)
    args = ap.parse_args()

    import torch

    from agentlib_mpc_amd import benchmarks as bm
    from agentlib_mpc_amd.runtime import native as nat
    from tests import cia_cases as cc

    assert torch.cuda.is_available(), "cia_leg.py measures on the GPU"
    dev = torch.device("cuda")
    n, N = args.agents, args.horizon
    be, cv = bm.one_room_cia(N=N, solver_options=bm.REFERENCE)
    prob, native = be.problem, be._native()
    temps = np.linspace(294.0, 299.0, n)
    p, lbw, ubw, w0 = prob.marshal.inputs([dict(cv, T=bm.V("T", float(t), 288.15, 303.15)) for t in temps], 0.0)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    tp, tl, tu, tw0 = T(p), T(lbw), T(ubw), T(w0)
    slot = T(be._slot)
    n_bin = be.binary_positions.shape[0]
    dt = float(be.config.discretization_options.time_step)
    pos = be.binary_positions.reshape(-1)
    native.reserve(n)
    tw = torch.empty_like(tw0)
    lam_g = torch.empty((n, prob.nlp.kernel_ng), dtype=torch.float64, device=dev)
    st_rel = torch.zeros(n * nat.STATS_BYTES, dtype=torch.uint8, device=dev)
    st_fix = torch.zeros(n * nat.STATS_BYTES, dtype=torch.uint8, device=dev)
    rd = None
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    legs = {"relaxed_solve_ms": [], "rounding_launch_ms": [], "fixed_solve_ms": [], "host_rounding_ms": []}
    for rep in range(args.repeats + 1):  # the first pass warms up (code objects, allocator)
        tw.copy_(tw0)
        e = [ev() for _ in range(4)]
        torch.cuda.synchronize()
        e[0].record()
        native.solve(tp, tl, tu, tw, lam_g=lam_g, stats=st_rel)
        e[1].record()
        rd = nat.cia_round(tw, tl, tu, slot, n_bin, N, dt, out=rd)
        e[2].record()
        w_rel = tw.clone()
        e_fix = (ev(), ev())
        e_fix[0].record()
        native.solve(tp, rd.lbw, rd.ubw, tw, lam_g=lam_g, stats=st_fix)
        e_fix[1].record()
        torch.cuda.synchronize()
        # the same rounding through the host
        t0 = time.perf_counter()
        w_host = w_rel.cpu().numpy()
        ref = cc.round_batch(w_host[:, pos].reshape(n, n_bin, N), dt)
        lf, uf = lbw.copy(), ubw.copy()
        ok = np.flatnonzero(ref["status"] == cc.OK)
        lf[np.ix_(ok, pos)] = uf[np.ix_(ok, pos)] = ref["b_bin"][ok].reshape(len(ok), -1)
        hl, hu = T(lf), T(uf)
        torch.cuda.synchronize()
        host_ms = 1e3 * (time.perf_counter() - t0)
        if rep == 0:
            continue
        legs["relaxed_solve_ms"].append(e[0].elapsed_time(e[1]))
        legs["rounding_launch_ms"].append(e[1].elapsed_time(e[2]))
        legs["fixed_solve_ms"].append(e_fix[0].elapsed_time(e_fix[1]))
        legs["host_rounding_ms"].append(host_ms)
    # both routes give the same bounds and the same deviation
    assert torch.equal(hl, rd.lbw) and torch.equal(hu, rd.ubw)
    assert np.array_equal(rd.eta.cpu().numpy(), ref["eta"], equal_nan=True)
    rel, fix = nat.stats_array(st_rel.cpu().numpy()), nat.stats_array(st_fix.cpu().numpy())
    status = rd.status.cpu().numpy()
    out = {"agents": n, "horizon": N, "repeats": args.repeats,
           **{k: round(float(np.median(v)), 4) for k, v in legs.items()},
           **{k.replace("_ms", "_min_max_ms"): [round(float(min(v)), 4), round(float(max(v)), 4)] for k, v in legs.items()},
           "relaxed_success": int(np.isin(rel["status"], (0, 1)).sum()), "fixed_success": int(np.isin(fix["status"], (0, 1)).sum()),
           "relaxed_iters_mean": round(float(rel["iter_count"].mean()), 2),
           "fixed_iters_mean": round(float(fix["iter_count"].mean()), 2),
           "relaxed_iters_max": int(rel["iter_count"].max()), "fixed_iters_max": int(fix["iter_count"].max()),
           "fixed_restorations": int(fix["n_restorations"].sum()),
           "rounding_ok": int((status == nat.CIA_OK).sum()),
           "agents_switched_on": int((rd.b_bin.cpu().numpy()[status == nat.CIA_OK].sum(axis=1) > 0).sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
