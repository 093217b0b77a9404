// ipm/bk.h -- dense Bunch-Kaufman in LDS: Inertia, bk_factor, bk_inverse, bk_sweep, bk_sweep2.  Model-free: needs
// wave.h and a MPCX_RCP(x) reciprocal (the generated source defines it), no MPCX_* dimension.
#pragma once
namespace mpcx_kernel {

// ---------------------------------------------------------------------------
// dense Bunch-Kaufman LDL^T in LDS (full symmetric storage, wave-wide):
// block-chain fallback and the nx x nx state-chain pivots
// ---------------------------------------------------------------------------
struct Inertia {
  int pos, neg, zero;
};

// zero pivots: absolute threshold (same constant as oracle/ipm.py ZERO_PIVOT);
// the barrier terms make the block norm unbounded near active bounds, so a
// norm-relative test would misclassify legitimate -delta_c pivots
constexpr double ZERO_PIVOT = 1e-20;
constexpr double BK_ALPHA = 0.6403882032022076;  // (1 + sqrt(17)) / 8

template <int NN, int LD>
__device__ __noinline__ Inertia bk_factor(ldsd* A, ldsi* perm, ldsi* piv, int lane) {
  constexpr int NN2 = NN * NN;
  Inertia in{0, 0, 0};
  for (int i = lane; i < NN; i += WAVE) perm[i] = i;
  wsync();
  int k = 0;
#pragma unroll 1
  while (k < NN) {
    const double akk = fabs(A[k * LD + k]);
    double lam = -1.0;
    int r = -1;
    for (int i = k + 1 + lane; i < NN; i += WAVE) {
      const double t = fabs(A[i * LD + k]);
      if (t > lam) { lam = t; r = i; }
    }
    if constexpr (NN <= 9) {  // candidates in lanes 0..7: DPP reduction inside the lane octet
      gargmax<8>(lam, r);
      lam = rl_f64(lam, 0);
      r = __builtin_amdgcn_readfirstlane(r);
    } else {
      wargmax(lam, r);
    }
    if (r < 0) lam = 0.0;
    int size = 1, kp = k;
    if (fmax(akk, lam) == 0.0 || akk >= BK_ALPHA * lam) {
      size = 1; kp = k;
    } else {
      double sg = 0.0;
      for (int j = k + lane; j < NN; j += WAVE)
        if (j != r) sg = fmax(sg, fabs(A[r * LD + j]));
      double sigma;
      if constexpr (NN <= 8) sigma = rl_f64(gmax<8>(sg), 0);
      else sigma = wmax(sg);
      if (akk * sigma >= BK_ALPHA * lam * lam) {
        size = 1; kp = k;
      } else if (fabs(A[r * LD + r]) >= BK_ALPHA * sigma) {
        size = 1; kp = r;
      } else {
        size = 2; kp = r;
      }
    }
    const int kk = k + size - 1;
    if (kp != kk) {
      for (int j = lane; j < NN; j += WAVE) {
        const double t = A[kp * LD + j]; A[kp * LD + j] = A[kk * LD + j]; A[kk * LD + j] = t;
      }
      wsync();
      for (int i = lane; i < NN; i += WAVE) {
        const double t = A[i * LD + kp]; A[i * LD + kp] = A[i * LD + kk]; A[i * LD + kk] = t;
      }
      if (lane == 0) { const int t = perm[kp]; perm[kp] = perm[kk]; perm[kk] = t; }
      wsync();
    }
    if (size == 1) {
      const double d = A[k * LD + k];
      if (fabs(d) <= ZERO_PIVOT) {
        in.zero++;
        for (int i = k + 1 + lane; i < NN; i += WAVE) A[i * LD + k] = 0.0;
      } else {
        if (d > 0) in.pos++; else in.neg++;
        const double rd = MPCX_RCP(d);
        for (int t = lane; t < NN2; t += WAVE) {
          const int i = t / NN, j = t % NN;
          if (i > k && j > k) A[i * LD + j] -= A[i * LD + k] * A[j * LD + k] * rd;
        }
        wsync();
        for (int i = k + 1 + lane; i < NN; i += WAVE) A[i * LD + k] *= rd;
      }
      if (lane == 0) piv[k] = 1;
    } else {
      const double a11 = A[k * LD + k], a21 = A[(k + 1) * LD + k], a22 = A[(k + 1) * LD + k + 1];
      const double det = a11 * a22 - a21 * a21;
      if (fabs(det) <= ZERO_PIVOT * ZERO_PIVOT) {
        in.zero += 2;
      } else {
        if (det < 0) { in.pos++; in.neg++; }
        else if (a11 + a22 > 0) in.pos += 2;
        else in.neg += 2;
      }
      const double rdet = MPCX_RCP(det);
      for (int t = lane; t < NN2; t += WAVE) {
        const int i = t / NN, j = t % NN;
        if (i > k + 1 && j > k + 1) {
          const double ai1 = A[i * LD + k], ai2 = A[i * LD + k + 1];
          const double l1 = (ai1 * a22 - ai2 * a21) * rdet, l2 = (ai2 * a11 - ai1 * a21) * rdet;
          A[i * LD + j] -= l1 * A[j * LD + k] + l2 * A[j * LD + k + 1];
        }
      }
      wsync();
      for (int i = k + 2 + lane; i < NN; i += WAVE) {
        const double ai1 = A[i * LD + k], ai2 = A[i * LD + k + 1];
        A[i * LD + k] = (ai1 * a22 - ai2 * a21) * rdet;
        A[i * LD + k + 1] = (ai2 * a11 - ai1 * a21) * rdet;
      }
      if (lane == 0) { piv[k] = 2; piv[k + 1] = 0; }
    }
    wsync();
    k += size;
  }
  return in;
}

// Explicit inverse of a factored block, A^{-1} = P^T L^{-T} D^{-1} L^{-1} P,
// written in the ORIGINAL index order to `out` (ld LD).  W, Y: scratch (LDS for the chain
// pivots, the workspace for the block-chain fallback).
template <int NN, int LD, typename OutT, typename WT>
__device__ __noinline__ void bk_inverse(const ldsd* A, const ldsi* perm, const ldsi* piv, WT* W,
                                        WT* Y, OutT* out, int lane) {
  constexpr int NN2 = NN * NN;
  for (int t = lane; t < NN2; t += WAVE) {
    const int i = t / NN, j = t % NN;
    W[i * LD + j] = (i == j) ? 1.0 : 0.0;
  }
  wsync();
  int k = 0;
#pragma unroll 1
  while (k < NN) {
    const int sz = piv[k];
    for (int t = lane; t < NN2; t += WAVE) {
      const int i = t / NN, j = t % NN;
      if (i >= k + sz && j <= k + sz - 1) {
        double v = A[i * LD + k] * W[k * LD + j];
        if (sz == 2) v += A[i * LD + k + 1] * W[(k + 1) * LD + j];
        W[i * LD + j] -= v;
      }
    }
    wsync();
    k += sz;
  }
  for (int t = lane; t < NN2; t += WAVE) {
    const int i = t / NN, j = t % NN;
    const int sz = piv[i];
    if (sz == 1) {
      const double d = A[i * LD + i];
      Y[i * LD + j] = (d != 0.0) ? W[i * LD + j] / d : 0.0;
    } else if (sz == 2) {
      const double a11 = A[i * LD + i], a21 = A[(i + 1) * LD + i], a22 = A[(i + 1) * LD + i + 1];
      const double det = a11 * a22 - a21 * a21;
      const double w0 = W[i * LD + j], w1 = W[(i + 1) * LD + j];
      Y[i * LD + j] = (a22 * w0 - a21 * w1) / det;
      Y[(i + 1) * LD + j] = (a11 * w1 - a21 * w0) / det;
    }
  }
  wsync();
  for (int t = lane; t < NN2; t += WAVE) {
    const int i = t / NN, j = t % NN;
    double acc = 0.0;
    const int mx = i > j ? i : j;
    for (int m = (mx > 0 ? mx - 1 : 0); m < NN; ++m) acc += W[m * LD + i] * Y[m * LD + j];
    out[perm[i] * LD + perm[j]] = acc;
  }
  wsync();
}

// Inverse AND inertia of a small symmetric indefinite block in one pass (state-chain
// pivots, NN*NN <= 64): the symmetric sweep operator (Goodnight) with Bunch-Kaufman pivot
// choices.  Lane (i, j) owns entry (i, j) of the LDS image; each pivot step is one pivot
// search (DPP reductions in the first lane octet) plus ONE read-modify-write of the whole
// block -- the swept rows/columns become the inverse as the sweep goes, so there are no
// row swaps, no separate L^{-1} sweep and no final product (bk_factor + bk_inverse take
// ~3x the dependent LDS round trips).  Pivots are the Schur-complement pivots of a
// symmetric elimination in the chosen order, so the inertia is the same (Sylvester); a
// zero pivot is counted and its row/column left out of the inverse, as the LDL^T path
// does.  A is destroyed; out receives A^{-1} (ld LD).
template <int NN, int LD, typename OutT>
__device__ __noinline__ Inertia bk_sweep(ldsd* A, OutT* out, int lane) {
  static_assert(NN * NN <= WAVE && NN <= 8, "one lane per entry; pivot candidates in one lane octet");
  constexpr unsigned FULL = (1u << NN) - 1u;
  Inertia in{0, 0, 0};
  const int ti = lane / NN, tj = lane % NN;
  const bool own = lane < NN * NN;
  unsigned done = 0u, zero = 0u;
#pragma unroll 1
  while (done != FULL) {
    const int k = __builtin_ctz(~done);
    const bool cand = lane < NN && !((done >> lane) & 1u);
    double lam = -1.0;
    int r = -1;
    if (cand && lane != k) { lam = fabs(A[lane * LD + k]); r = lane; }
    gargmax<8>(lam, r);
    lam = rl_f64(lam, 0);
    r = __builtin_amdgcn_readfirstlane(r);
    if (r < 0) lam = 0.0;
    const double akk = fabs(A[k * LD + k]);
    int p = k, q = -1;  // 1x1 pivot p, or 2x2 pivot {k, q}
    if (!(fmax(akk, lam) == 0.0 || akk >= BK_ALPHA * lam)) {
      double sg = 0.0;
      if (cand && lane != r) sg = fabs(A[r * LD + lane]);
      const double sigma = rl_f64(gmax<8>(sg), 0);
      if (akk * sigma >= BK_ALPHA * lam * lam) p = k;
      else if (fabs(A[r * LD + r]) >= BK_ALPHA * sigma) p = r;
      else q = r;
    }
    if (q < 0) {
      const double d = A[p * LD + p];
      done |= 1u << p;
      if (fabs(d) <= ZERO_PIVOT) { in.zero++; zero |= 1u << p; continue; }
      if (d > 0) in.pos++; else in.neg++;
      const double rd = MPCX_RCP(d);
      if (own) {
        const double aip = A[ti * LD + p], apj = A[p * LD + tj], aij = A[ti * LD + tj];
        A[ti * LD + tj] = (ti == p) ? ((tj == p) ? -rd : apj * rd) : (tj == p) ? aip * rd : aij - aip * apj * rd;
      }
    } else {
      const double a11 = A[k * LD + k], a21 = A[q * LD + k], a22 = A[q * LD + q];
      const double det = a11 * a22 - a21 * a21;
      done |= (1u << k) | (1u << q);
      if (fabs(det) <= ZERO_PIVOT * ZERO_PIVOT) { in.zero += 2; zero |= (1u << k) | (1u << q); continue; }
      if (det < 0) { in.pos++; in.neg++; }
      else if (a11 + a22 > 0) in.pos += 2;
      else in.neg += 2;
      const double rdet = MPCX_RCP(det);
      const double p11 = a22 * rdet, p12 = -a21 * rdet, p22 = a11 * rdet;  // pivot-block inverse
      if (own) {
        const double aik = A[ti * LD + k], aiq = A[ti * LD + q], akj = A[k * LD + tj], aqj = A[q * LD + tj];
        const double aij = A[ti * LD + tj];
        const double xk = aik * p11 + aiq * p12, xq = aik * p12 + aiq * p22;  // row i times P^{-1}
        const double yk = p11 * akj + p12 * aqj, yq = p12 * akj + p22 * aqj;  // P^{-1} times column j
        const bool ip = ti == k || ti == q, jp = tj == k || tj == q;
        double v;
        if (ip && jp) v = -((ti == k) ? ((tj == k) ? p11 : p12) : ((tj == k) ? p12 : p22));
        else if (ip) v = (ti == k) ? yk : yq;
        else if (jp) v = (tj == k) ? xk : xq;
        else v = aij - (xk * akj + xq * aqj);
        A[ti * LD + tj] = v;
      }
    }
    wsync();
  }
  wsync();
  if (own) out[ti * LD + tj] = (((zero >> ti) | (zero >> tj)) & 1u) ? 0.0 : -A[ti * LD + tj];
  wsync();
  return in;
}

// Two independent blocks swept at once (the twisted chain's forward and backward pivots, r04):
// bk_sweep's arithmetic and pivot choices for each block -- lanes 0-7 search block A's pivot
// candidates and lanes 8-15 block B's, each octet with its own DPP reduction, and every owning
// lane updates its entry of both blocks -- so one pass costs the dependent latency of one.
// In place (each block receives its own inverse); twob false sweeps A alone.
template <int NN, int LD>
__device__ __noinline__ Inertia bk_sweep2(ldsd* A, ldsd* B, bool twob, int lane) {
  static_assert(NN * NN <= WAVE && NN <= 8, "one lane per entry; pivot candidates in one lane octet");
  constexpr unsigned FULL = (1u << NN) - 1u;
  Inertia in{0, 0, 0};
  const int ti = lane / NN, tj = lane % NN;
  const bool own = lane < NN * NN;
  const int oc = lane >> 3, ol = lane & 7;  // octet 0 searches A, octet 1 searches B
  ldsd* const M = oc == 0 ? A : B;
  unsigned dA = 0u, zA = 0u, dB = twob ? 0u : FULL, zB = 0u;
#pragma unroll 1
  while (dA != FULL || dB != FULL) {
    const bool goA = dA != FULL, goB = dB != FULL;
    const int kA = goA ? __builtin_ctz(~dA) : 0, kB = goB ? __builtin_ctz(~dB) : 0;
    const int k = oc == 0 ? kA : kB;
    const bool cand = oc < 2 && ol < NN && (oc == 0 ? goA : goB) && !(((oc == 0 ? dA : dB) >> ol) & 1u);
    double lam = -1.0;
    int r = -1;
    if (cand && ol != k) { lam = fabs(M[ol * LD + k]); r = ol; }
    gargmax<8>(lam, r);
    double lamA = rl_f64(lam, 0), lamB = rl_f64(lam, 8);
    const int rA = __builtin_amdgcn_readlane(r, 0), rB = __builtin_amdgcn_readlane(r, 8);
    if (rA < 0) lamA = 0.0;
    if (rB < 0) lamB = 0.0;
    const double akkA = fabs(A[kA * LD + kA]), akkB = fabs(B[kB * LD + kB]);
    const bool needA = goA && !(fmax(akkA, lamA) == 0.0 || akkA >= BK_ALPHA * lamA);
    const bool needB = goB && !(fmax(akkB, lamB) == 0.0 || akkB >= BK_ALPHA * lamB);
    int pA = kA, qA = -1, pB = kB, qB = -1;
    if (needA || needB) {
      const int ro = oc == 0 ? rA : rB;
      double sg = 0.0;
      if (cand && ol != ro && (oc == 0 ? needA : needB)) sg = fabs(M[ro * LD + ol]);
      const double g8 = gmax<8>(sg);
      const double sigA = rl_f64(g8, 0), sigB = rl_f64(g8, 8);
      if (needA) {
        if (akkA * sigA >= BK_ALPHA * lamA * lamA) pA = kA;
        else if (fabs(A[rA * LD + rA]) >= BK_ALPHA * sigA) pA = rA;
        else qA = rA;
      }
      if (needB) {
        if (akkB * sigB >= BK_ALPHA * lamB * lamB) pB = kB;
        else if (fabs(B[rB * LD + rB]) >= BK_ALPHA * sigB) pB = rB;
        else qB = rB;
      }
    }
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      if (blk == 0 ? !goA : !goB) continue;
      ldsd* const X = blk == 0 ? A : B;
      unsigned& done = blk == 0 ? dA : dB;
      unsigned& zero = blk == 0 ? zA : zB;
      const int kk = blk == 0 ? kA : kB, p = blk == 0 ? pA : pB, q = blk == 0 ? qA : qB;
      if (q < 0) {
        const double d = X[p * LD + p];
        done |= 1u << p;
        if (fabs(d) <= ZERO_PIVOT) { in.zero++; zero |= 1u << p; continue; }
        if (d > 0) in.pos++; else in.neg++;
        const double rd = MPCX_RCP(d);
        if (own) {
          const double aip = X[ti * LD + p], apj = X[p * LD + tj], aij = X[ti * LD + tj];
          X[ti * LD + tj] = (ti == p) ? ((tj == p) ? -rd : apj * rd) : (tj == p) ? aip * rd : aij - aip * apj * rd;
        }
      } else {
        const double a11 = X[kk * LD + kk], a21 = X[q * LD + kk], a22 = X[q * LD + q];
        const double det = a11 * a22 - a21 * a21;
        done |= (1u << kk) | (1u << q);
        if (fabs(det) <= ZERO_PIVOT * ZERO_PIVOT) { in.zero += 2; zero |= (1u << kk) | (1u << q); continue; }
        if (det < 0) { in.pos++; in.neg++; }
        else if (a11 + a22 > 0) in.pos += 2;
        else in.neg += 2;
        const double rdet = MPCX_RCP(det);
        const double p11 = a22 * rdet, p12 = -a21 * rdet, p22 = a11 * rdet;
        if (own) {
          const double aik = X[ti * LD + kk], aiq = X[ti * LD + q], akj = X[kk * LD + tj], aqj = X[q * LD + tj];
          const double aij = X[ti * LD + tj];
          const double xk = aik * p11 + aiq * p12, xq = aik * p12 + aiq * p22;
          const double yk = p11 * akj + p12 * aqj, yq = p12 * akj + p22 * aqj;
          const bool ip = ti == kk || ti == q, jp = tj == kk || tj == q;
          double v;
          if (ip && jp) v = -((ti == kk) ? ((tj == kk) ? p11 : p12) : ((tj == kk) ? p12 : p22));
          else if (ip) v = (ti == kk) ? yk : yq;
          else if (jp) v = (tj == kk) ? xk : xq;
          else v = aij - (xk * akj + xq * aqj);
          X[ti * LD + tj] = v;
        }
      }
    }
    wsync();
  }
  if (own) {
    A[ti * LD + tj] = (((zA >> ti) | (zA >> tj)) & 1u) ? 0.0 : -A[ti * LD + tj];
    if (twob) B[ti * LD + tj] = (((zB >> ti) | (zB >> tj)) & 1u) ? 0.0 : -B[ti * LD + tj];
  }
  wsync();
  return in;
}

}  // namespace mpcx_kernel
