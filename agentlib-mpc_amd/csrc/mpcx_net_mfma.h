// mpcx_net_mfma.h — wave-level evaluation of the NARX networks on the FP64 matrix cores.
//
// Included by generated model sources that contain network nodes (runtime/codegen.py,
// device-only section).  What it replaces: the CasADi evaluation of the reference's
// serialized ANN (agentlib_mpc/models/casadi_predictor.py:306-336, one dense hidden layer,
// topology from modules/ml_model_training/ml_model_trainer.py:617-626) inside every IPOPT
// callback.  The per-stage generated code evaluates each network once per stage in a
// loop over the hidden units, one stage per lane (12 of 64 lanes busy for a C5 zone);
// here all evaluations of one network in the agent (stages x call sites, R rows) are one
// batched product per wavefront:
//
//   A^T = W1^T X^T + b1          [H x R]   (v_mfma_f64_16x16x4_f64, K = inputs)
//   v   = w2 . act(A) + b2       [R]       (row sums of the accumulator tile)
//   g^T = W1_D (w2 o act'(A))    [ND1 x R] (K = hidden units)
//   h^T = P_D  (w2 o act''(A))   [ND2 x R] (P_D[p][j] = W1[a_p][j] W1[b_p][j])
//
// Orientation: the first product is computed transposed (hidden unit on the accumulator
// row, evaluation on the lane), so its accumulator register r of lane l holds hidden
// unit 4r + (l >> 4) of evaluation l & 15 -- exactly the B operand of the k-step over
// hidden units 4r .. 4r + 3 of the two derivative products: no LDS round trip and no
// lane movement between the three products.
//
// eval_rbf below is the same pass for the second network kind (Gaussian-process means), eval2
// for the third (two hidden layers).
//
// f64 MFMA lane maps (CDNA4): A[m = l & 15][k = l >> 4], B[k = l >> 4][n = l & 15],
// D lane l register r: [m = (l >> 4) + 4 r][n = l & 15].
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace mpcx_net {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) double ldsd;

// activation codes follow symbolic._ACTS: sigmoid, tanh, linear, softplus, exponential, gaussian
template <int ACT>
__device__ __forceinline__ void act(double a, double& s0, double& s1, double& s2) {
  if constexpr (ACT == 0) {
    s0 = 1.0 / (1.0 + exp(-a)); s1 = s0 * (1.0 - s0); s2 = s1 * (1.0 - 2.0 * s0);
  } else if constexpr (ACT == 1) {
    s0 = tanh(a); s1 = 1.0 - s0 * s0; s2 = -2.0 * s0 * s1;
  } else if constexpr (ACT == 2) {
    s0 = a; s1 = 1.0; s2 = 0.0;
  } else if constexpr (ACT == 3) {
    const double sg = 1.0 / (1.0 + exp(-a));
    s0 = log(1.0 + exp(a)); s1 = sg; s2 = sg * (1.0 - sg);
  } else if constexpr (ACT == 4) {
    s0 = exp(a); s1 = s0; s2 = s0;
  } else {
    s0 = exp(-a * a); s1 = -2.0 * a * s0; s2 = (4.0 * a * a - 2.0) * s0;
  }
}

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// R evaluations of one network (inputs X[R][NIN], LDS) -> V[R] (if WV), G[R][ND1]
// (d/d inputs D1[]), Hd[R][ND2] (d2 / d inputs of pair p, table PW[ND2][H]).  Called by
// all 64 lanes of the wave; every lane takes part in every product.
template <int R, int NIN, int H, int ACT, bool WV, int ND1, int ND2>
__device__ __forceinline__ void eval(const ldsd* X, ldsd* V, ldsd* Gd, ldsd* Hd, const double* W1T,
                                     const double* B1, const double* W2, double b2, const int* D1,
                                     const double* PW, int lane) {
  constexpr int JT = (H + 15) / 16;   // hidden-unit tiles
  constexpr int KS = (NIN + 3) / 4;   // k-steps over the inputs
  constexpr bool W1D = ND1 > 0, W2D = ND2 > 0;
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll 1
  for (int rt = 0; rt < (R + 15) / 16; ++rt) {
    const int row = rt * 16 + lr;
    d4 acc[JT];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jt * 16 + lk + 4 * r;
        acc[jt][r] = j < H ? B1[j] : 0.0;
      }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int i = ks * 4 + lk;
      const double bx = (row < R && i < NIN) ? X[row * NIN + i] : 0.0;
#pragma unroll
      for (int jt = 0; jt < JT; ++jt) {
        const int jj = jt * 16 + lr;
        const double aw = (jj < H && i < NIN) ? W1T[jj * NIN + i] : 0.0;
        acc[jt] = mfma(aw, bx, acc[jt]);
      }
    }
    // activations, weighted by the output layer; registers keep the accumulator layout
    double c0[JT][4], c1[JT][4], c2[JT][4];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jt * 16 + lk + 4 * r;
        const double w = j < H ? W2[j] : 0.0;
        double s0, s1, s2;
        act<ACT>(acc[jt][r], s0, s1, s2);
        c0[jt][r] = w * s0; c1[jt][r] = w * s1; c2[jt][r] = w * s2;
      }
    if constexpr (WV) {
      double v = 0.0;
#pragma unroll
      for (int jt = 0; jt < JT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) v += c0[jt][r];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (lk == 0 && row < R) V[row] = v + b2;
    }
    if constexpr (W1D) {
#pragma unroll
      for (int it = 0; it < (ND1 + 15) / 16; ++it) {
        const int ii = it * 16 + lr;
        const int col = ii < ND1 ? D1[ii] : 0;
        d4 g = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = jt * 16 + 4 * r + lk;
            const double aw = (ii < ND1 && j < H) ? W1T[j * NIN + col] : 0.0;
            g = mfma(aw, c1[jt][r], g);
          }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = it * 16 + lk + 4 * r;
          if (o < ND1 && row < R) Gd[row * ND1 + o] = g[r];
        }
      }
    }
    if constexpr (W2D) {
#pragma unroll
      for (int pt = 0; pt < (ND2 + 15) / 16; ++pt) {
        const int pp = pt * 16 + lr;
        d4 h = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = jt * 16 + 4 * r + lk;
            const double aw = (pp < ND2 && j < H) ? PW[pp * H + j] : 0.0;
            h = mfma(aw, c2[jt][r], h);
          }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = pt * 16 + lk + 4 * r;
          if (o < ND2 && row < R) Hd[row * ND2 + o] = h[r];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// RBF networks (the mean of a Gaussian process, symbolic.RBFNetwork): R evaluations of
//
//   y(x) = sum_j a_j exp(-1/2 |z - T_j|^2),   z = s o x + t
//
// Replaces the CasADi graph of the reference's CasadiGPR (casadi_predictor.py:126-174).  With
// w_j = a_j exp(TT_j + z.T_j - 1/2 |z|^2), TT_j = -1/2 |T_j|^2 (the reference's expanded
// distance) and the moments S0 = sum w_j, S1_i = sum w_j T_ji, S2_ik = sum w_j T_ji T_jk:
//
//   y = S0,  dy/dx_i = -s_i (z_i S0 - S1_i),
//   d2y/dx_i dx_k = s_i s_k (z_i z_k S0 - z_i S1_k - z_k S1_i + S2_ik - delta_ik S0)
//
// The first product is transposed as in eval (training point on the accumulator row,
// evaluation on the lane; accumulators start from TT in the role of B1, B = z formed from the
// LDS inputs), so register r of lane l holds the weight of training point 4r + (l >> 4) of
// the tile for evaluation l & 15: the B operand of the moment products.  The training points
// are streamed in tiles of 16: per tile the value and the moment accumulators are updated and
// the weights dropped, so register use does not depend on NT.  A Hessian entry (a, b) needs
// S1_a and S1_b whether or not the gradient list holds them: every pair tile carries three
// accumulators (S2_ab, S1_a, S1_b; A operands T_ja T_jb from two table reads, T_ja, T_jb),
// which land in the lane and register of the entry they belong to.  Rows of the last tile
// past NT get the weight 0 exactly (a is read as 0 there; exp of their finite exponent is
// finite).  The exponent is <= 0 up to rounding: no overflow guard; far from the data the
// weights underflow to 0 and every output is 0.
//
// X[R][NIN] (LDS) -> V[R] (if WV), Gd[R][ND1] (inputs D1[]), Hd[R][ND2] (pairs P2[ND2][2]).
// T[NT][NIN], TT[NT], A[NT], S[NIN], SH[NIN]: tables of the network.
template <int R, int NIN, int NT, bool WV, int ND1, int ND2>
__device__ __forceinline__ void eval_rbf(const ldsd* X, ldsd* V, ldsd* Gd, ldsd* Hd, const double* T,
                                         const double* TT, const double* A, const double* S,
                                         const double* SH, const int* D1, const int* P2, int lane) {
  constexpr int JT = (NT + 15) / 16;   // training-point tiles
  constexpr int KS = (NIN + 3) / 4;    // k-steps over the inputs
  constexpr int GT = (ND1 + 15) / 16, PT = (ND2 + 15) / 16;
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll 1
  for (int rt = 0; rt < (R + 15) / 16; ++rt) {
    const int row = rt * 16 + lr;
    // B operand of the first product and |z|^2 of the row (partial sums over the lane's inputs)
    double bz[KS];
    double zz = 0.0;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int i = ks * 4 + lk;
      bz[ks] = (row < R && i < NIN) ? X[row * NIN + i] * S[i] + SH[i] : 0.0;
      zz += bz[ks] * bz[ks];
    }
    zz += __shfl_xor(zz, 16, 64);
    zz += __shfl_xor(zz, 32, 64);
    const double hz = 0.5 * zz;
    double v = 0.0;
    d4 g[GT > 0 ? GT : 1], h2[PT > 0 ? PT : 1], ha[PT > 0 ? PT : 1], hb[PT > 0 ? PT : 1];
    int gcol[GT > 0 ? GT : 1], pa[PT > 0 ? PT : 1], pb[PT > 0 ? PT : 1];
#pragma unroll
    for (int it = 0; it < GT; ++it) {
      g[it] = d4{0.0, 0.0, 0.0, 0.0};
      gcol[it] = it * 16 + lr < ND1 ? D1[it * 16 + lr] : 0;
    }
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      h2[pt] = ha[pt] = hb[pt] = d4{0.0, 0.0, 0.0, 0.0};
      const int pp = pt * 16 + lr;
      pa[pt] = pp < ND2 ? P2[2 * pp] : 0;
      pb[pt] = pp < ND2 ? P2[2 * pp + 1] : 0;
    }
#pragma unroll 1
    for (int jt = 0; jt < JT; ++jt) {
      d4 acc;
      double w[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jt * 16 + lk + 4 * r;
        acc[r] = j < NT ? TT[j] : 0.0;
      }
      const int jj = jt * 16 + lr;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int i = ks * 4 + lk;
        const double aw = (jj < NT && i < NIN) ? T[jj * NIN + i] : 0.0;
        acc = mfma(aw, bz[ks], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jt * 16 + lk + 4 * r;
        w[r] = (j < NT ? A[j] : 0.0) * exp(acc[r] - hz);
        v += w[r];
      }
#pragma unroll
      for (int it = 0; it < GT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = jt * 16 + 4 * r + lk;
          const double aw = (it * 16 + lr < ND1 && j < NT) ? T[j * NIN + gcol[it]] : 0.0;
          g[it] = mfma(aw, w[r], g[it]);
        }
#pragma unroll
      for (int pt = 0; pt < PT; ++pt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = jt * 16 + 4 * r + lk;
          const bool on = pt * 16 + lr < ND2 && j < NT;
          const double ta = on ? T[j * NIN + pa[pt]] : 0.0;
          const double tb = on ? T[j * NIN + pb[pt]] : 0.0;
          h2[pt] = mfma(ta * tb, w[r], h2[pt]);
          ha[pt] = mfma(ta, w[r], ha[pt]);
          hb[pt] = mfma(tb, w[r], hb[pt]);
        }
    }
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);   // S0 of the row, in its four lanes
    if constexpr (WV)
      if (lk == 0 && row < R) V[row] = v;
#pragma unroll
    for (int it = 0; it < GT; ++it)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = it * 16 + lk + 4 * r;
        if (o < ND1 && row < R) {
          const int i = D1[o];
          const double zi = X[row * NIN + i] * S[i] + SH[i];
          // the product rounded on its own (no fma): on a model's only training point the
          // gradient is exactly 0, as in the fp64 evaluation
          double zv;
          {
#pragma clang fp contract(off)
            zv = zi * v;
          }
          Gd[row * ND1 + o] = -S[i] * (zv - g[it][r]);
        }
      }
#pragma unroll
    for (int pt = 0; pt < PT; ++pt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = pt * 16 + lk + 4 * r;
        if (o < ND2 && row < R) {
          const int a = P2[2 * o], b = P2[2 * o + 1];
          const double za = X[row * NIN + a] * S[a] + SH[a];
          const double zb = X[row * NIN + b] * S[b] + SH[b];
          const double m = za * zb * v - za * hb[pt][r] - zb * ha[pt][r] + h2[pt][r] - (a == b ? v : 0.0);
          Hd[row * ND2 + o] = S[a] * S[b] * m;
        }
      }
  }
}

// ---------------------------------------------------------------------------------------------
// Two hidden layers (symbolic.DeepNetwork): R evaluations of
//
//   y(x) = b3 + w3 . act2(a2),   a2 = W2^T act1(a1) + b2,   a1 = W1^T x + b1
//
// Replaces the layer-by-layer expansion of a Dense -> Dense -> Dense(linear) model of the
// reference's trainer (ml_model_trainer.py:592-626) into the stage graph.  With
// c1 = w3 o act2'(a2), c2 = w3 o act2''(a2) and u = W2 c1:
//
//   dy/dx_i       = sum_k W1[i,k] act1'(a1_k) u_k
//   d2y/dx_a dx_b = sum_k W1[a,k] W1[b,k] act1''(a1_k) u_k + sum_j c2_j J[j,a] J[j,b],
//   J[:,i] = W2^T (act1'(a1) o W1[i,:])
//
// Layout.  The layer-1 accumulator is eval's (hidden-1 unit 4r + (l >> 4) of the tile in
// register r, evaluation l & 15 on the lane): after act1 it is the B operand of a k-step over
// hidden-1 units, so a2^T = W2^T s1 (A operand W2 read as [k = hidden-1][m = hidden-2]) lands in
// the same layout over the hidden-2 units.  c1 there is the B operand of a k-step over
// hidden-2 units, and u^T = W2 c1 (A operand W2 read as [m = hidden-1][k = hidden-2]: the same
// table with the two strides exchanged) lands in the layer-1 layout again, where act1' and
// act1'' sit.  The gradient and the first Hessian term are then eval's products on act1' o u
// and act1'' o u.  A Jacobian column J[:,i] is one more product of the first kind with the B
// operand act1' o W1[i,:].
//
// Second Hessian term.  The pairs are walked in table order (sorted: equal first index a
// adjacent).  J[:,a] stays in registers while a repeats; J[:,b] is recomputed per pair unless
// b = a: about half the products of forming both columns for every pair, and two resident
// columns instead of one per input.  The contraction over the hidden-2 units is a sum over the
// lane's registers and the four lanes of the evaluation; the result is added to the register
// of the first term's accumulator tile that holds the pair, so Hd is written once.
//
// Pad rows: act(0) != 0 for four of the activations, so a padded hidden-1 unit meets a zero W2
// operand in every product that sums over it (and gives u = 0), a padded hidden-2 unit a zero
// w3 (c1 = c2 = 0) and a zero W2 operand; rows of the last tile past R write nothing.
//
// X[R][NIN] (LDS) -> V[R] (if WV), Gd[R][ND1] (inputs D1[]), Hd[R][ND2] (pairs P2[ND2][2], table
// PW[ND2][H1] of W1[a,k] W1[b,k]).  W1T[H1][NIN], B1[H1], W2[H1][H2], B2[H2], W3[H2].  No LDS
// besides X and the outputs.
template <int R, int NIN, int H1, int H2, int ACT1, int ACT2, bool WV, int ND1, int ND2>
__device__ __forceinline__ void eval2(const ldsd* X, ldsd* V, ldsd* Gd, ldsd* Hd, const double* W1T,
                                      const double* B1, const double* W2, const double* B2,
                                      const double* W3, double b3, const int* D1, const double* PW,
                                      const int* P2, int lane) {
  constexpr int JT = (H1 + 15) / 16;   // hidden-1 tiles
  constexpr int KT = (H2 + 15) / 16;   // hidden-2 tiles
  constexpr int KS = (NIN + 3) / 4;    // k-steps over the inputs
  constexpr bool W1D = ND1 > 0, W2D = ND2 > 0;
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll 1
  for (int rt = 0; rt < (R + 15) / 16; ++rt) {
    const int row = rt * 16 + lr;
    // layer 1: as eval
    d4 acc[JT];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jt * 16 + lk + 4 * r;
        acc[jt][r] = j < H1 ? B1[j] : 0.0;
      }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int i = ks * 4 + lk;
      const double bx = (row < R && i < NIN) ? X[row * NIN + i] : 0.0;
#pragma unroll
      for (int jt = 0; jt < JT; ++jt) {
        const int jj = jt * 16 + lr;
        const double aw = (jj < H1 && i < NIN) ? W1T[jj * NIN + i] : 0.0;
        acc[jt] = mfma(aw, bx, acc[jt]);
      }
    }
    double s0[JT][4], s1[JT][4], s2[JT][4];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) act<ACT1>(acc[jt][r], s0[jt][r], s1[jt][r], s2[jt][r]);
    // layer 2: a2^T = W2^T s0 + b2, hidden-2 unit on the accumulator row
    d4 acc2[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = kt * 16 + lk + 4 * r;
        acc2[kt][r] = k < H2 ? B2[k] : 0.0;
      }
      const int kk = kt * 16 + lr;
#pragma unroll
      for (int jt = 0; jt < JT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = jt * 16 + 4 * r + lk;
          const double aw = (j < H1 && kk < H2) ? W2[j * H2 + kk] : 0.0;
          acc2[kt] = mfma(aw, s0[jt][r], acc2[kt]);
        }
    }
    double c1[KT][4], c2[KT][4];
    double v = 0.0;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = kt * 16 + lk + 4 * r;
        const double w = k < H2 ? W3[k] : 0.0;
        double t0, t1, t2;
        act<ACT2>(acc2[kt][r], t0, t1, t2);
        v += w * t0; c1[kt][r] = w * t1; c2[kt][r] = w * t2;
      }
    if constexpr (WV) {
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (lk == 0 && row < R) V[row] = v + b3;
    }
    if constexpr (W1D || W2D) {
      // u^T = W2 c1 in the layer-1 layout; e1 = act1' o u, e2 = act1'' o u
      double e1[JT][4], e2[JT][4];
#pragma unroll
      for (int jt = 0; jt < JT; ++jt) {
        const int jj = jt * 16 + lr;
        d4 u = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = kt * 16 + 4 * r + lk;
            const double aw = (jj < H1 && k < H2) ? W2[jj * H2 + k] : 0.0;
            u = mfma(aw, c1[kt][r], u);
          }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          e1[jt][r] = s1[jt][r] * u[r];
          e2[jt][r] = s2[jt][r] * u[r];
        }
      }
      if constexpr (W1D) {
#pragma unroll
        for (int it = 0; it < (ND1 + 15) / 16; ++it) {
          const int ii = it * 16 + lr;
          const int col = ii < ND1 ? D1[ii] : 0;
          d4 g = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int jt = 0; jt < JT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int j = jt * 16 + 4 * r + lk;
              const double aw = (ii < ND1 && j < H1) ? W1T[j * NIN + col] : 0.0;
              g = mfma(aw, e1[jt][r], g);
            }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = it * 16 + lk + 4 * r;
            if (o < ND1 && row < R) Gd[row * ND1 + o] = g[r];
          }
        }
      }
      if constexpr (W2D) {
        // J[:, i] in the layer-2 layout
        auto jcol = [&](const int i, d4 (&J)[KT]) __attribute__((always_inline)) {
          double b[JT][4];
#pragma unroll
          for (int jt = 0; jt < JT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int j = jt * 16 + lk + 4 * r;
              b[jt][r] = s1[jt][r] * (j < H1 ? W1T[j * NIN + i] : 0.0);
            }
#pragma unroll
          for (int kt = 0; kt < KT; ++kt) {
            const int kk = kt * 16 + lr;
            J[kt] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int jt = 0; jt < JT; ++jt)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int j = jt * 16 + 4 * r + lk;
                const double aw = (j < H1 && kk < H2) ? W2[j * H2 + kk] : 0.0;
                J[kt] = mfma(aw, b[jt][r], J[kt]);
              }
          }
        };
        d4 Ja[KT], Jb[KT];
        int ca = -1;   // input of the resident column
#pragma unroll 1
        for (int pt = 0; pt < (ND2 + 15) / 16; ++pt) {
          d4 h = {0.0, 0.0, 0.0, 0.0};
          const int pend = (pt * 16 + 16 < ND2) ? pt * 16 + 16 : ND2;
#pragma unroll 1
          for (int p = pt * 16; p < pend; ++p) {
            const int a = P2[2 * p], b = P2[2 * p + 1];
            if (a != ca) {
              jcol(a, Ja);
              ca = a;
            }
            if (b != a) jcol(b, Jb);
            double t = 0.0;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                t += c2[kt][r] * Ja[kt][r] * (b != a ? Jb[kt][r] : Ja[kt][r]);
            t += __shfl_xor(t, 16, 64);
            t += __shfl_xor(t, 32, 64);
            // pair p is row p - 16 pt of the tile: register (p >> 2) & 3 of lane quarter p & 3
#pragma unroll
            for (int r = 0; r < 4; ++r)
              h[r] += (lk == (p & 3) && r == ((p >> 2) & 3)) ? t : 0.0;
          }
          const int pp = pt * 16 + lr;
#pragma unroll
          for (int jt = 0; jt < JT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int j = jt * 16 + 4 * r + lk;
              const double aw = (pp < ND2 && j < H1) ? PW[pp * H1 + j] : 0.0;
              h = mfma(aw, e2[jt][r], h);
            }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = pt * 16 + lk + 4 * r;
            if (o < ND2 && row < R) Hd[row * ND2 + o] = h[r];
          }
        }
      }
    }
  }
}

}  // namespace mpcx_net
