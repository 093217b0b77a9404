// ipm/wave.h -- wavefront layer: the wave size, address-space pointer types, DPP / readlane exchanges, wave and
// lane-group reductions, wsync, lane_now, MPCX_PIN, isfin / absn.  Model-free: needs no MPCX_*
// dimension and no other header of ipm/.
#pragma once
namespace mpcx_kernel {

constexpr int WAVE = 64;

// address-space qualified pointers: global_* / ds_* addressing inside the
// noinline phases (generic pointers compile to flat_*, which drain both
// counters and block load/store reordering)
typedef __attribute__((address_space(1))) double gdbl;
typedef __attribute__((address_space(1))) int gint;
typedef __attribute__((address_space(3))) double ldsd;
typedef __attribute__((address_space(3))) int ldsi;
#define LDSP(x) ((ldsd*)(x))
#define LDSI(x) ((ldsi*)(x))

// wave-uniform 64-bit value into SGPRs
__device__ __forceinline__ unsigned long long uni64(unsigned long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// ---------------------------------------------------------------------------
// wave and lane-group helpers
// ---------------------------------------------------------------------------
// DPP lane exchange inside aligned groups (quad_perm xor1 / xor2, half-row and
// row mirrors): register-speed, no LDS round trip
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, false);
}
// broadcast lane `l` (compile-time in unrolled loops) of a double: two v_readlane
__device__ __forceinline__ double rl_f64(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}
// Wave reductions (all 64 lanes active): DPP steps inside each row of 16 lanes (VALU
// latency), then the four row results read into SGPRs and combined -- instead of six
// LDS-permute (ds_bpermute) round trips.  MPCX_SHFL_REDUCE: the butterfly over __shfl_xor.
#ifndef MPCX_SHFL_REDUCE
__device__ __forceinline__ double wsum(double v) {
  v += dpp_f64<0xB1>(v);   // quad_perm xor 1
  v += dpp_f64<0x4E>(v);   // quad_perm xor 2
  v += dpp_f64<0x141>(v);  // row_half_mirror: the other quad of the half-row
  v += dpp_f64<0x140>(v);  // row_mirror: the other half of the row
  return (rl_f64(v, 0) + rl_f64(v, 16)) + (rl_f64(v, 32) + rl_f64(v, 48));
}
__device__ __forceinline__ double wmax(double v) {
  v = fmax(v, dpp_f64<0xB1>(v));
  v = fmax(v, dpp_f64<0x4E>(v));
  v = fmax(v, dpp_f64<0x141>(v));
  v = fmax(v, dpp_f64<0x140>(v));
  return fmax(fmax(rl_f64(v, 0), rl_f64(v, 16)), fmax(rl_f64(v, 32), rl_f64(v, 48)));
}
__device__ __forceinline__ double wmin(double v) {
  v = fmin(v, dpp_f64<0xB1>(v));
  v = fmin(v, dpp_f64<0x4E>(v));
  v = fmin(v, dpp_f64<0x141>(v));
  v = fmin(v, dpp_f64<0x140>(v));
  return fmin(fmin(rl_f64(v, 0), rl_f64(v, 16)), fmin(rl_f64(v, 32), rl_f64(v, 48)));
}
__device__ __forceinline__ int wsumi(int v) {
  v += dpp_i32<0xB1>(v);
  v += dpp_i32<0x4E>(v);
  v += dpp_i32<0x141>(v);
  v += dpp_i32<0x140>(v);
  return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
         (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}
#else
__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}
__device__ __forceinline__ double wmax(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, WAVE));
  return v;
}
__device__ __forceinline__ double wmin(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, WAVE));
  return v;
}
__device__ __forceinline__ int wsumi(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}
#endif
// argmax with smallest index on ties
__device__ __forceinline__ void wargmax(double& v, int& idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    double ov = __shfl_xor(v, o, WAVE);
    int oi = __shfl_xor(idx, o, WAVE);
    if (ov > v || (ov == v && oi >= 0 && (idx < 0 || oi < idx))) { v = ov; idx = oi; }
  }
}
__device__ __forceinline__ void sync() { __syncthreads(); }
// Wavefront-scope sync for LDS-only hand-offs between lanes: a workgroup is one
// wavefront and the LDS executes one wave's DS instructions in issue order, so
// only compiler ordering is needed (no s_barrier, no vmcnt drain).
__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lane id that the compiler can neither hoist nor keep live across calls: non-leaf phase
// functions recompute lane-derived values after each call instead of parking them in
// callee-saved VGPRs (saved to scratch on every call)
__device__ __forceinline__ int lane_now() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l & (WAVE - 1);  // the range for the compiler: lane-derived offsets are known non-negative
}

// Pin a loaded operand: the empty asm "uses" it here, so the compiler issues the load before this
// point instead of sinking it into the branch that uses it -- a load waited for inside a branch
// drains every older load (vmcnt counts in issue order), one memory round trip per such load.  A
// phase loads all its operands, pins them, then computes: one round trip for the batch.
#ifndef MPCX_NO_PIN
#define MPCX_PIN(x) asm volatile("" ::"v"(x))
#else  // diagnostics (A/B): the compiler places the loads
#define MPCX_PIN(x) (void)0
#endif
// The iteration head (inlined into the kernel body) is left to the compiler's placement: pinned as
// one batch it measured no faster at 4096 C3 agents and 0.5-1.5 % slower on C1 and MHE (r06/s6);
// MPCX_PIN_HEAD_BATCH pins it (A/B)
#ifdef MPCX_PIN_HEAD_BATCH
#define MPCX_PIN_HEAD(x) MPCX_PIN(x)
#else
#define MPCX_PIN_HEAD(x) (void)0
#endif

template <int GG>
__device__ __forceinline__ double gmax(double v) {
  if constexpr (GG >= 2) v = fmax(v, dpp_f64<0xB1>(v));
  if constexpr (GG >= 4) v = fmax(v, dpp_f64<0x4E>(v));
  if constexpr (GG >= 8) v = fmax(v, dpp_f64<0x141>(v));
  if constexpr (GG >= 16) v = fmax(v, dpp_f64<0x140>(v));
  if constexpr (GG >= 32) v = fmax(v, __shfl_xor(v, 16, WAVE));
  if constexpr (GG >= 64) v = fmax(v, __shfl_xor(v, 32, WAVE));
  return v;
}
__device__ __forceinline__ void amax_merge(double& v, int& idx, double ov, int oi) {
  if (ov > v || (ov == v && oi >= 0 && (idx < 0 || oi < idx))) { v = ov; idx = oi; }
}
template <int GG>
__device__ __forceinline__ void gargmax(double& v, int& idx) {
  if constexpr (GG >= 2) amax_merge(v, idx, dpp_f64<0xB1>(v), dpp_i32<0xB1>(idx));
  if constexpr (GG >= 4) amax_merge(v, idx, dpp_f64<0x4E>(v), dpp_i32<0x4E>(idx));
  if constexpr (GG >= 8) amax_merge(v, idx, dpp_f64<0x141>(v), dpp_i32<0x141>(idx));
  if constexpr (GG >= 16) amax_merge(v, idx, dpp_f64<0x140>(v), dpp_i32<0x140>(idx));
  if constexpr (GG >= 32) amax_merge(v, idx, __shfl_xor(v, 16, WAVE), __shfl_xor(idx, 16, WAVE));
  if constexpr (GG >= 64) amax_merge(v, idx, __shfl_xor(v, 32, WAVE), __shfl_xor(idx, 32, WAVE));
}

__device__ __forceinline__ bool isfin(double v) { return fabs(v) < INFINITY; }
__device__ __forceinline__ double absn(double v) {  // |v| with NaN -> +inf (total order for pivoting)
  const double t = fabs(v);
  return t == t ? t : INFINITY;
}

}  // namespace mpcx_kernel
