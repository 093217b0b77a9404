"""The mixed-integer backend by combinatorial integral approximation (CIA).

``MI355XCIABackend`` <- ``CasADiCIABackend`` (type ``"casadi_cia"``, `casadi_/minlp_cia.py:60-225`)
on the ``CasadiMINLPSystem`` and its transcriptions (`casadi_/minlp.py`).  One step is three device
launches with nothing crossing to the host in between:

1. the NLP with the binary controls relaxed to their [0, 1] bounds (``mpcx_batch_solve``);
2. the rounding of the relaxed controls (``mpcx_cia_round``: where the reference calls
   pycombina's branch and bound on the host, an exact dynamic programme in a HIP kernel that
   reads the relaxed solution where the first solve left it and writes the bounds of the second);
3. the NLP again with the binary controls fixed through their bounds, started from the relaxed
   optimum (the reference remembers it between the two calls, `core/discretization.py:198-207`).

The rounding problem has no switch or dwell limits (`minlp_cia.py:131-143` sets none) and lives on
the backend's uniform grid (`minlp_cia.py:128-129`).  The results of the fixed solve are what
``solve`` returns, saves and warm-starts the next call from; the relaxed results go to
``relaxed_<results file>`` and stay on the backend as ``last_relaxed``, the rounding's outputs as
``last_cia``.
"""

from __future__ import annotations

import os
import time
from typing import NamedTuple, Optional, Sequence

import numpy as np
import pydantic

from agentlib_mpc_amd.data_structures.mpc_datamodels import (
    DiscretizationMethod, MINLPVariableReference, cia_relaxed_results_path, stats_path,
)
from agentlib_mpc_amd.optimization_backends import discretization as disc
from agentlib_mpc_amd.optimization_backends.mi355x import MI355XBackend, MI355XBackendConfig
from agentlib_mpc_amd.optimization_backends.results import Results
from agentlib_mpc_amd.optimization_backends.system import MINLPSystem


class MI355XCIABackendConfig(MI355XBackendConfig):
    @pydantic.field_validator("overwrite_result_file")
    @classmethod
    def check_overwrite(cls, overwrite, info):
        """`minlp_cia.py:33-57`: the base class's check, with the relaxed solve's files removed
        along with the main ones."""
        res_file = info.data.get("results_file")
        if res_file and info.data.get("save_results"):
            if overwrite:
                relaxed = cia_relaxed_results_path(res_file)
                for f in (res_file, stats_path(res_file), relaxed, stats_path(relaxed)):
                    try:
                        os.remove(f)
                    except FileNotFoundError:
                        pass
            elif os.path.isfile(res_file):
                raise FileExistsError(
                    f"Results file {res_file} already exists and will not be overwritten "
                    "automatically. Set 'overwrite_result_file' to True to enable automatic "
                    "overwrite it.")
        return overwrite


class CIARoundingResults(NamedTuple):
    """What the rounding did, per agent of the last call (host arrays)."""
    eta: np.ndarray      # [n] integral deviation of B from the relaxed controls, seconds (NaN: not OK)
    b_bin: np.ndarray    # [n, n_bin, N] the binary controls (NaN: not OK)
    status: np.ndarray   # [n] int32: native.CIA_OK / CIA_BAD_INPUT / CIA_BAND_OVERFLOW

    @property
    def ok(self) -> np.ndarray:
        return self.status == 0


class MI355XCIABackend(MI355XBackend):
    """Backend ``"casadi_cia"`` replacement."""

    system_type = MINLPSystem
    discretization_types = {
        DiscretizationMethod.collocation: disc.MINLPCollocation,
        DiscretizationMethod.multiple_shooting: disc.MINLPMultipleShooting,
    }
    config_type = MI355XCIABackendConfig
    var_ref: MINLPVariableReference

    def __init__(self, config: dict):
        super().__init__(config)
        self._created_rel_file = False
        self.last_relaxed = None                          # FleetResults of the relaxed solve
        self.last_cia: Optional[CIARoundingResults] = None
        self._slot = None        # host slot table of mpcx_cia_round
        self._slot_dev = None    # ... on the device
        self._rounding = None    # the rounding's device buffers, reused while the batch size stays

    def setup_optimization(self, var_ref):
        from agentlib_mpc_amd.runtime import native

        super().setup_optimization(var_ref)
        nlp = self.problem.nlp
        if nlp.lift is not None:  # the transcriptions add no change penalties: never lifted
            raise NotImplementedError("the CIA backend needs the kernel's layout to be the reference's")
        lay = nlp.var_groups[self.system.binary_controls.name]
        n_bin, N = lay.dim, len(lay.grid)
        if not 1 <= n_bin <= native.CIA_MAX_MODES:
            raise ValueError(f"the CIA backend rounds 1 to {native.CIA_MAX_MODES} binary controls, got {n_bin}")
        if not 1 <= N <= native.CIA_MAX_INTERVALS:
            raise ValueError(f"the CIA backend rounds horizons of 1 to {native.CIA_MAX_INTERVALS} intervals, got {N}")
        ts = float(self.config.discretization_options.time_step)
        if not np.allclose(lay.grid, ts * np.arange(N), rtol=0.0, atol=1e-9 * max(ts, 1.0)):
            raise NotImplementedError("the CIA backend rounds on a uniform grid only")
        self.binary_positions = lay.index            # [n_bin, N] positions in w
        self._slot = native.cia_slot_table(lay.index, nlp.nw)
        self._slot_dev = self._rounding = None
        self.last_relaxed = self.last_cia = None

    # -- solve (`minlp_cia.py:75-95`) -------------------------------------------------
    def solve(self, now: float, current_vars: dict) -> Results:
        from agentlib_mpc_amd.runtime import native

        res = self.solve_batch(now, [current_vars])
        status = int(self.last_cia.status[0])
        if status != native.CIA_OK:
            raise ValueError("the relaxed binary controls could not be rounded "
                             f"({native.CIA_STATUS_NAMES.get(status, status)}); relaxed solve: "
                             f"{self.last_relaxed.stats[0]['return_status']}")
        return res[0]

    def solve_batch(self, now, batch_vars: Sequence[dict], agent_ids: Optional[Sequence] = None):
        """Relaxed solve, rounding and fixed solve of every entry of ``batch_vars`` in three
        launches.  Returns the fixed solve's :class:`FleetResults`, which are also the next call's
        warm start (``agent_ids`` as in :meth:`MI355XBackend.solve_batch`).  An agent whose
        rounding status (``last_cia.status``) is not OK solved the relaxed problem twice."""
        if self.problem is None:
            raise RuntimeError("setup_optimization() must be called before solve()")
        n = len(batch_vars)
        w_prev = self._remembered_optima(n, self._previous_slots(n, agent_ids))
        p, lbw, ubw, w0, sampled = self.problem.marshal.inputs(batch_vars, now, w_prev, return_sampled_bounds=True)
        res = self.solve_arrays(p, lbw, ubw, w0, result_bounds=sampled)
        self._remembered = res.w.copy()
        if self.config.save_results:
            for i in range(n):
                self.save_rel_result_df(self.last_relaxed[i], now)
                self.save_result_df(res[i], now)
        return res

    def solve_arrays(self, p, lbw, ubw, w0, lbg=None, ubg=None, result_bounds=None):
        """The three launches on reference-layout NLP inputs [n, .] (host arrays): one upload, the
        relaxed solve, the rounding, the fixed solve from the relaxed optimum, one read-back.
        Returns the fixed solve's :class:`FleetResults` (its lower / upper columns show the
        binary controls' fixed bounds); sets ``last_relaxed`` and ``last_cia``."""
        import torch

        from agentlib_mpc_amd.optimization_backends.problem import FleetResults
        from agentlib_mpc_amd.runtime import native as nat

        prob = self.problem
        native = self._native()
        dev = torch.device("cuda")
        t0 = time.perf_counter()
        n = p.shape[0]
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev, non_blocking=True)  # noqa
        tp, tl, tu, tw = T(p), T(lbw), T(ubw), T(w0)
        tg = tug = None
        if lbg is not None:
            tg, tug = T(lbg), T(ubg)
        if self._slot_dev is None:
            self._slot_dev = torch.from_numpy(self._slot).to(dev)
        if self._rounding is not None and self._rounding.eta.shape[0] != n:
            self._rounding = None
        lam_g = torch.empty((n, prob.nlp.kernel_ng), dtype=torch.float64, device=dev)
        st_rel = torch.zeros(n * nat.STATS_BYTES, dtype=torch.uint8, device=dev)
        st_fix = torch.zeros(n * nat.STATS_BYTES, dtype=torch.uint8, device=dev)
        n_bin, N = self.binary_positions.shape
        native.solve(tp, tl, tu, tw, lbg=tg, ubg=tug, lam_g=lam_g, stats=st_rel)
        w_rel = tw.clone()  # the second solve continues in tw
        rd = self._rounding = nat.cia_round(tw, tl, tu, self._slot_dev, n_bin, N,
                                            float(self.config.discretization_options.time_step), out=self._rounding)
        native.solve(tp, rd.lbw, rd.ubw, tw, lbg=tg, ubg=tug, lam_g=lam_g, stats=st_fix)
        w_fix, w_relaxed = tw.cpu().numpy(), w_rel.cpu().numpy()
        raw_fix, raw_rel = st_fix.cpu().numpy(), st_rel.cpu().numpy()
        cia = CIARoundingResults(eta=rd.eta.cpu().numpy(), b_bin=rd.b_bin.cpu().numpy().reshape(n, n_bin, N),
                                 status=rd.status.cpu().numpy())
        wall = {"t_wall_total": time.perf_counter() - t0}
        rlb, rub = result_bounds if result_bounds is not None else (lbw, ubw)
        flb, fub = np.array(rlb, copy=True), np.array(rub, copy=True)
        pos = self.binary_positions.reshape(-1)
        ok = np.flatnonzero(cia.ok)
        flb[np.ix_(ok, pos)] = fub[np.ix_(ok, pos)] = cia.b_bin[ok].reshape(len(ok), -1)
        self.last_relaxed = FleetResults(prob, prob.marshal, p, rlb, rub, w_relaxed,
                                         nat.StatsView(nat.stats_array(raw_rel), wall))
        self.last_cia = cia
        return FleetResults(prob, prob.marshal, p, flb, fub, w_fix, nat.StatsView(nat.stats_array(raw_fix), wall))

    # -- the relaxed solve's results file (`minlp_cia.py:173-225`) -------------------------
    def save_rel_result_df(self, results: Results, now: float = 0):
        """Rows of the relaxed solve and its stats line into ``relaxed_<results file>`` and its
        stats file, with the same writers and columns as the main files' rows."""
        if not self.config.save_results:
            return
        res_file = cia_relaxed_results_path(self.config.results_file)
        if not self.rel_results_file_exists():
            results.write_columns(res_file)
            results.write_stats_columns(stats_path(res_file))
        df = results.df
        df.index = [str((now, x)) for x in df.index]
        df.to_csv(res_file, mode="a", header=False)
        with open(stats_path(res_file), "a") as f:
            f.writelines(results.stats_line(str(now)))

    def rel_results_file_exists(self) -> bool:
        """Like :meth:`results_folder_exists`, for the relaxed file: looked up once."""
        if self._created_rel_file:
            return True
        res_file = cia_relaxed_results_path(self.config.results_file)
        if res_file.is_file():
            self._created_rel_file = True
            return True
        res_file.parent.mkdir(parents=True, exist_ok=True)
        self._created_rel_file = True
        return False
