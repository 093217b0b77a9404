"""Diagnostic (GPU): kernel time of each code object of a structure (lds / mid / main) over fleet
sizes -- the measurement behind mpcx_batch_solve's choice of build by agents per CU.

usage: MODEL=one_room SIZES=1,256,512,1024,2048,4096 python scripts/build_scan.py
Every build solves the same fleet (bench.py C3 inputs for one_room, the template's values
otherwise) at the reference's IPOPT settings; statuses / iteration counts are compared with the
first build that ran.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "agentlib-mpc_amd")]


def main():
    import numpy as np
    import torch

    import bench
    from agentlib_mpc_amd import benchmarks as bm
    from agentlib_mpc_amd.optimization_backends.problem import fleet_nlp_inputs
    from agentlib_mpc_amd.runtime.native import STATS_BYTES, NativeError, stats_array

    model = os.environ.get("MODEL", "one_room")
    sizes = [int(v) for v in os.environ.get("SIZES", "1,256,512,1024,2048,4096").split(",")]
    builds = os.environ.get("BUILDS", "lds,mid,main").split(",")
    reps = int(os.environ.get("REPS", "5"))
    be, cv = getattr(bm, model)(solver_options=bm.REFERENCE)
    prob = be.problem
    native = be._native()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    dev = torch.device("cuda")
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    for n in sizes:
        if model == "one_room":
            vals = bench.fleet_values(n, 20261015 + 2)
        else:
            first = next(k for q in prob.system.parameters for k in q.ref_names if k in cv)
            vals = {first: np.full(n, cv[first].value, float)}
        p, lbw, ubw, w0 = prob.to_kernel(*fleet_nlp_inputs(prob, cv, vals))
        tp, tl, tu, tw0 = T(p), T(lbw), T(ubw), T(w0)
        native.reserve(n)
        ref = None
        for b in builds:
            try:
                native.select_build(b)
            except NativeError:  # no such build for this structure
                continue
            tw = tw0.clone()
            st = torch.zeros(n * STATS_BYTES, dtype=torch.uint8, device=dev)
            s = torch.cuda.current_stream()
            for _ in range(2):
                tw.copy_(tw0)
                native.solve(tp, tl, tu, tw, stats=st, stream=s.cuda_stream)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                tw.copy_(tw0)
                native.solve(tp, tl, tu, tw, stats=st, stream=s.cuda_stream)
            e1.record(s)
            torch.cuda.synchronize()
            arr = stats_array(st.cpu().numpy())
            key = (arr["status"].tolist(), arr["iter_count"].tolist())
            same = None if ref is None else key == ref
            ref = ref or key
            print(json.dumps({"model": model, "agents": n, "agents_per_cu": n / cus, "build": b,
                              "kernel_ms": e0.elapsed_time(e1) / reps, "mean_iter": float(arr["iter_count"].mean()),
                              "same_status_iters_as_first": same}), flush=True)
        native.select_build(None)


if __name__ == "__main__":
    main()
