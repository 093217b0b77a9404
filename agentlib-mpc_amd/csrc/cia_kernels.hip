// cia_kernels.hip — rounding of relaxed binary controls by combinatorial integral approximation
// (mpcx_cia_round, include/mpcx.h), between the relaxed and the fixed solve of the CIA backend.
//
// Reference semantics: CasADiCIABackend.do_pycombina (agentlib_mpc/optimization_backends/casadi_/
// minlp_cia.py:99-171): clip the relaxed controls, add the dummy mode of a single control, solve
// the CIA problem on the backend's uniform grid with no switch or dwell limits.  The reference
// calls pycombina's branch and bound; here the exact dynamic programme over count vectors that the
// header states, restricted to the band that sum-up rounding's deviation allows.
//
// Mapping: one wave per agent, WAVES_PER_GROUP waves per workgroup, no workgroup barrier (a wave
// without an agent leaves at once).  Lane s of a level holds the state whose counts of the modes
// 0 .. nc-2 are lo_k(i) + digit_k(s) (digit 0 most significant: the smallest lane that attains the
// minimum is the lexicographically smallest count vector); the last mode's count follows from the
// sum.  F of the previous level stays in a register and is read across lanes (ds_bpermute); the
// predecessor bytes [N][64], the windows' starts [N][4] and the clipped controls [4][N] are the
// wave's LDS.  Every loop runs over nw, N, nc or the 64 lanes.  Every global address is
// agent * row length + an index below the row length: the slot table's values only index LDS, and
// are range-checked before they do.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mpcx.h"

namespace {

constexpr int WAVE = 64;
constexpr int WAVES_PER_GROUP = 4;
constexpr int MAX_NC = MPCX_CIA_MAX_MODES;
constexpr int CAP = MPCX_CIA_MAX_STATES;
constexpr double CLIP_TOL = 1e-5;  // minlp_cia.py:105-112
constexpr double COL_TOL = 1e-6;
static_assert(CAP == WAVE, "one lane per state");
static_assert(MAX_NC == 4, "the windows' starts are stored four to a level");

// LDS bytes of one wave: controls [4][N] fp64, window starts [N][4] int16, predecessors [N][64]
// bytes, chosen modes [N] bytes (rounded up to keep the next wave's doubles aligned)
__host__ __device__ constexpr int lds_per_wave(int N) { return N * (32 + 8 + 64) + ((N + 7) & ~7); }
static_assert(WAVES_PER_GROUP * lds_per_wave(MPCX_CIA_MAX_INTERVALS) <= 64 * 1024, "LDS of a workgroup");

// hand-off between the lanes of one wave through LDS: the LDS runs a wave's instructions in issue
// order, only the compiler has to keep it
__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(WAVE* WAVES_PER_GROUP)
k_cia_round(int n_agents, int nw, int n_bin, int N, double dt, const int* __restrict__ slot,
            const double* __restrict__ w, const double* lbw, const double* ubw, double* lbw_fix, double* ubw_fix,
            double* __restrict__ b_bin, double* __restrict__ eta_out, int* __restrict__ status,
            const int* __restrict__ active) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const int a = blockIdx.x * WAVES_PER_GROUP + wv;
  if (a >= n_agents) return;  // wave-uniform
  if (active != nullptr && active[a] == 0) return;
  const int nc = n_bin == 1 ? 2 : n_bin, nm = nc - 1, ne = n_bin * N;
  unsigned char* base = lds + wv * lds_per_wave(N);
  double* b = (double*)base;                   // [MAX_NC][N], mode-major
  short* los = (short*)(base + N * 32);        // [N][4]
  unsigned char* pred = base + N * 40;         // [N][64]
  unsigned char* mode = base + N * 104;        // [N]
  const long row = (long)a * nw;

  // the relaxed controls, clipped; a (j, i) that no slot names stays NaN and is bad input
  for (int e = lane; e < MAX_NC * N; e += WAVE) b[e] = NAN;
  wsync();
  for (int k = lane; k < nw; k += WAVE) {
    const int e = slot[k];
    if (e >= 0 && e < ne) {
      double v = w[row + k];
      if (v > -CLIP_TOL && v < 0.0) v = 0.0;
      if (v > 1.0 && v < 1.0 + CLIP_TOL) v = 1.0;
      b[e] = v;
    }
  }
  wsync();
  bool bad = false;
  for (int i = lane; i < N; i += WAVE) {
    double s = 0.0;
    for (int r = 0; r < n_bin; ++r) {
      const double v = b[r * N + i];
      if (!(v >= 0.0 && v <= 1.0)) bad = true;  // NaN and infinities too
      s = r == 0 ? v : s + v;
    }
    if (n_bin >= 2 && !(fabs(s - 1.0) <= COL_TOL)) bad = true;
    if (n_bin == 1) b[N + i] = fmax(0.0, 1.0 - b[i]);
  }
  bad = __any(bad) != 0;
  wsync();

  bool overflow = false;
  double fmin_all = INFINITY;
  if (!bad) {
    // sum-up rounding: the incumbent's deviation (every lane computes the same)
    double acc[MAX_NC] = {0.0, 0.0, 0.0, 0.0};
    int cs[MAX_NC] = {0, 0, 0, 0};
    double eta = 0.0;
    for (int i = 0; i < N; ++i) {
      int js = 0;
      double most = 0.0;
#pragma unroll
      for (int j = 0; j < MAX_NC; ++j)
        if (j < nc) {
          acc[j] += b[j * N + i];
          const double d = acc[j] - (double)cs[j];
          if (j == 0 || d > most) { most = d; js = j; }
        }
#pragma unroll
      for (int j = 0; j < MAX_NC; ++j)
        if (j < nc) {
          cs[j] += (j == js) ? 1 : 0;
          eta = fmax(eta, fabs(acc[j] - (double)cs[j]));
        }
    }
    // the band: W counts per mode, W^(nc-1) states
    const double w2 = floor(2.0 * eta);
    const int W = w2 < (double)CAP ? (int)w2 + 2 : CAP + 1;
    int slots = 1;
    if (W > CAP) overflow = true;
    else
      for (int k = 0; k < nm; ++k) slots *= W;
    if (slots > CAP) overflow = true;
    if (!overflow) {
      int str[MAX_NC - 1], dig[MAX_NC - 1], lo_prev[MAX_NC - 1] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < MAX_NC - 1; ++k) {
        int s = 1;
        for (int q = k + 1; q < nm; ++q) s *= W;
        str[k] = k < nm ? s : 0;
        dig[k] = k < nm ? (lane / s) % W : 0;
      }
      double fprev = lane == 0 ? 0.0 : INFINITY;  // F(-1, 0) = 0
#pragma unroll
      for (int j = 0; j < MAX_NC; ++j) acc[j] = 0.0;
      for (int i = 0; i < N; ++i) {
        int lo[MAX_NC - 1] = {0, 0, 0};
        int c[MAX_NC] = {0, 0, 0, 0};
        int rest = i + 1;
        bool valid = lane < slots;
#pragma unroll
        for (int j = 0; j < MAX_NC; ++j)
          if (j < nc) acc[j] += b[j * N + i];
#pragma unroll
        for (int k = 0; k < MAX_NC - 1; ++k)
          if (k < nm) {
            lo[k] = (int)ceil(acc[k] - eta) - 1;
            // the count above the window must not be within the band
            if (fabs(acc[k] - (double)(lo[k] + W)) <= eta) overflow = true;
            c[k] = lo[k] + dig[k];
            rest -= c[k];
            valid = valid && c[k] >= 0;
          }
#pragma unroll
        for (int j = 0; j < MAX_NC; ++j)
          if (j == nm) c[j] = rest;
        valid = valid && rest >= 0;
        double dev = 0.0;
#pragma unroll
        for (int j = 0; j < MAX_NC; ++j)
          if (j < nc) dev = fmax(dev, fabs(acc[j] - (double)c[j]));
        const bool live = valid && dev <= eta;
        double best = INFINITY;
        int bj = 0;
#pragma unroll
        for (int j = 0; j < MAX_NC; ++j)
          if (j < nc) {  // wave-uniform: every lane takes part in the exchange
            bool ok = c[j] >= 1;
            int sp = 0;
#pragma unroll
            for (int k = 0; k < MAX_NC - 1; ++k)
              if (k < nm) {
                const int dp = c[k] - (k == j ? 1 : 0) - lo_prev[k];
                ok = ok && dp >= 0 && dp < W;
                sp += dp * str[k];
              }
            const double v = __shfl(fprev, ok ? sp : 0, WAVE);
            if (ok && v < best) { best = v; bj = j; }
          }
        pred[i * WAVE + lane] = (unsigned char)bj;
        if (lane < MAX_NC - 1) los[i * 4 + lane] = (short)(lane == 0 ? lo[0] : lane == 1 ? lo[1] : lo[2]);
        fprev = live ? fmax(dev, best) : INFINITY;
#pragma unroll
        for (int k = 0; k < MAX_NC - 1; ++k) lo_prev[k] = lo[k];
      }
      // the best final state, the smallest lane on ties
      fmin_all = fprev;
#pragma unroll
      for (int o = WAVE / 2; o > 0; o >>= 1) fmin_all = fmin(fmin_all, __shfl_xor(fmin_all, o, WAVE));
      const unsigned long long at = __ballot(fprev == fmin_all);
      if (!(fmin_all < INFINITY) || at == 0ull) overflow = true;  // no state left: never with a live incumbent
      wsync();
      if (!overflow) {
        // walk the predecessors back (every lane the same walk)
        int s = __ffsll((long long)at) - 1;
        int c[MAX_NC - 1] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < MAX_NC - 1; ++k)
          if (k < nm) c[k] = lo_prev[k] + (s / str[k]) % W;
        for (int i = N - 1; i >= 0; --i) {
          const int j = pred[i * WAVE + (s & (WAVE - 1))];
          if (lane == 0) mode[i] = (unsigned char)j;
          s = 0;
#pragma unroll
          for (int k = 0; k < MAX_NC - 1; ++k)
            if (k < nm) {
              c[k] -= (k == j) ? 1 : 0;
              s += (c[k] - (i > 0 ? (int)los[(i - 1) * 4 + k] : 0)) * str[k];
            }
        }
        wsync();
      }
    }
  }

  // the fixed rows: the relaxed rows, and B at the binary positions of an agent that is OK
  const bool okay = !bad && !overflow;
  for (int k = lane; k < nw; k += WAVE) {
    double l = lbw[row + k], u = ubw[row + k];
    const int e = slot[k];
    if (e >= 0 && e < ne) {
      double v = NAN;
      if (okay) {
        const int r = e / N, i = e - r * N;
        v = mode[i] == r ? 1.0 : 0.0;
        l = v;
        u = v;
      }
      if (b_bin != nullptr) b_bin[(long)a * ne + e] = v;
    }
    lbw_fix[row + k] = l;
    ubw_fix[row + k] = u;
  }
  if (lane == 0) {
    eta_out[a] = okay ? dt * fmin_all : NAN;
    status[a] = bad ? MPCX_CIA_BAD_INPUT : overflow ? MPCX_CIA_BAND_OVERFLOW : MPCX_CIA_OK;
  }
}

}  // namespace

extern "C" int mpcx_cia_round(int32_t n_agents, int32_t nw, int32_t n_bin, int32_t n_intervals, double dt,
                              const int32_t* slot, const double* w, const double* lbw, const double* ubw,
                              double* lbw_fix, double* ubw_fix, double* b_bin, double* eta, int32_t* status,
                              const int32_t* active, void* stream) {
  if (n_agents < 0 || nw < 1 || n_bin < 1 || n_bin > MPCX_CIA_MAX_MODES || n_intervals < 1 ||
      n_intervals > MPCX_CIA_MAX_INTERVALS || (int64_t)n_bin * n_intervals > nw || !(dt > 0.0) || !(dt < INFINITY))
    return MPCX_ERR_ARG;
  if (!slot || !w || !lbw || !ubw || !lbw_fix || !ubw_fix || !eta || !status) return MPCX_ERR_ARG;
  if (n_agents == 0) return MPCX_OK;
  const unsigned groups = (unsigned)(((long)n_agents + WAVES_PER_GROUP - 1) / WAVES_PER_GROUP);
  hipLaunchKernelGGL(k_cia_round, dim3(groups), dim3(WAVE * WAVES_PER_GROUP), WAVES_PER_GROUP * lds_per_wave(n_intervals),
                     (hipStream_t)stream, n_agents, nw, n_bin, n_intervals, dt, slot, w, lbw, ubw, lbw_fix, ubw_fix,
                     b_bin, eta, status, active);
  if (hipGetLastError() != hipSuccess) return MPCX_ERR_HIP;
  return MPCX_OK;
}
