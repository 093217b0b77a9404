// mpcx_builds.h — the optional builds of a problem structure and the rule that picks one for a
// launch.  Host only, no HIP: mpcx_runtime.cpp includes it, generated sources do not (it is not
// part of the code-object key), and tests/test_native_abi.py compiles the rule alone.
#pragma once

namespace mpcx_builds {

// in routing order; the main build serves whatever no optional build takes
enum Slot {
  SMALL = 0,  // workspace in LDS (mpcx_problem_small_fleet): batches of at most `limit` agents
  MID,        // one wave per SIMD (mpcx_problem_mid_fleet): batches of at most `limit` agents
  WIDE,       // more agents per CU (mpcx_problem_wide_fleet): batches of at least `limit`, 0 none
  N_SLOTS,
  MAIN = N_SLOTS
};

// The choice goes by the workgroups launched: a mapped launch of a few unfrozen agents runs the
// small-fleet build however large the fleet is.
inline int route(const int limit[N_SLOTS], const bool loaded[N_SLOTS], int n_launch) {
  if (loaded[SMALL] && n_launch <= limit[SMALL]) return SMALL;
  if (loaded[MID] && n_launch <= limit[MID]) return MID;
  if (loaded[WIDE] && limit[WIDE] > 0 && n_launch >= limit[WIDE]) return WIDE;
  return MAIN;
}

}  // namespace mpcx_builds
