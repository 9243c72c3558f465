// hmpc_sens_common.h -- device helpers the two kernels that differentiate the
// solve share (hmpc_sens.hip: forward mode, hmpc_vjp_kernel.h: reverse mode): the
// stage record, the projector Pi_k onto the free input directions, the 6 x 6
// factor of G~_k on reciprocal pivots and Bd_k' times a costate
// (DESIGN.md 4.8).  Device code only; internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include "hmpc_model.h"

namespace hmpc {

namespace {

constexpr int kRec = 29;   // doubles per stage record
constexpr int R_CS = 0;    // cos, sin of the linearisation yaw
constexpr int R_BW = 2;    // rows 9..11 of Bd_k, [3][6]
constexpr int R_PI = 20;   // force projector, symmetric: xx xy xz yy yz zz
constexpr int R_TM = 26;   // torque mask (1: free), contiguous with R_PI
constexpr int kKst = 72;   // K_k, [6][12]
constexpr int kCst = 21;   // factor of G~_k: 15 strict-lower entries, 6 reciprocal diagonals
constexpr double kPivotFloor = 1e-11;   // relative to the row's own diagonal

// active-mask bits of the force rows
constexpr int A_FXP = 1, A_FXM = 2, A_FYP = 4, A_FYM = 8, A_FZU = 16;

__device__ __forceinline__ constexpr int li(int i, int j) { return i * (i - 1) / 2 + j; }   // i > j

// I - Q Q' for the active force rows of a regular stance stage (modified
// Gram-Schmidt; at most one of +-fx - mu fz, one of +-fy - mu fz -- 2f: the
// fixed fy -- and fz <= f_max: always independent)
template <int VAR>
__device__ __forceinline__ void force_projector(int mask, double mu, double (&pi)[6]) {
  const bool px = (mask & (A_FXP | A_FXM)) != 0;
  const bool py = VAR == 2 ? true : (mask & (A_FYP | A_FYM)) != 0;
  const bool pz = (mask & A_FZU) != 0;
  const double sx = (mask & A_FXP) ? 1.0 : -1.0;
  const double sy = (mask & A_FYP) ? 1.0 : -1.0;
  double a[3][3] = {{px ? sx : 0.0, 0.0, px ? -mu : 0.0},
                    {0.0, py ? (VAR == 2 ? 1.0 : sy) : 0.0, (py && VAR != 2) ? -mu : 0.0},
                    {0.0, 0.0, pz ? 1.0 : 0.0}};
  const bool pres[3] = {px, py, pz};
  pi[0] = 1.0; pi[1] = 0.0; pi[2] = 0.0; pi[3] = 1.0; pi[4] = 0.0; pi[5] = 1.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < i; ++j) {
      const double r = a[j][0] * a[i][0] + a[j][1] * a[i][1] + a[j][2] * a[i][2];
#pragma unroll
      for (int c = 0; c < 3; ++c) a[i][c] = fma(-r, a[j][c], a[i][c]);
    }
    const double n2 = a[i][0] * a[i][0] + a[i][1] * a[i][1] + a[i][2] * a[i][2];
    const double ri = (pres[i] && n2 > 0.0) ? 1.0 / sqrt(n2) : 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) a[i][c] *= ri;
    pi[0] = fma(-a[i][0], a[i][0], pi[0]);
    pi[1] = fma(-a[i][0], a[i][1], pi[1]);
    pi[2] = fma(-a[i][0], a[i][2], pi[2]);
    pi[3] = fma(-a[i][1], a[i][1], pi[3]);
    pi[4] = fma(-a[i][1], a[i][2], pi[4]);
    pi[5] = fma(-a[i][2], a[i][2], pi[5]);
  }
}

// v <- Pi v: pr = the record's projector (6) and torque mask (3)
__device__ __forceinline__ void pi_apply(const double* pr, double (&v)[6]) {
  const double f0 = pr[0] * v[0] + pr[1] * v[1] + pr[2] * v[2];
  const double f1 = pr[1] * v[0] + pr[3] * v[1] + pr[4] * v[2];
  const double f2 = pr[2] * v[0] + pr[4] * v[1] + pr[5] * v[2];
  v[0] = f0; v[1] = f1; v[2] = f2;
#pragma unroll
  for (int c = 0; c < 3; ++c) v[3 + c] *= pr[6 + c];
}

// G~ = C C' on reciprocal pivots (lower triangle of A read)
__device__ __forceinline__ void chol6(const double (&A)[6][6], double (&cf)[kCst]) {
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int p = 0; p < j; ++p) d = fma(-cf[li(j, p)], cf[li(j, p)], d);
    cf[15 + j] = rsq_nr(d);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int p = 0; p < j; ++p) s = fma(-cf[li(i, p)], cf[li(j, p)], s);
      cf[li(i, j)] = s * cf[15 + j];
    }
  }
}
// y <- C^-1 y
__device__ __forceinline__ void chol_fwd(const double* cf, double (&y)[6]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = y[i];
#pragma unroll
    for (int p = 0; p < i; ++p) s = fma(-cf[li(i, p)], y[p], s);
    y[i] = s * cf[15 + i];
  }
}
// w <- C'^-1 w
__device__ __forceinline__ void chol_bwd(const double* cf, double (&w)[6]) {
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = w[i];
#pragma unroll
    for (int p = i + 1; p < 6; ++p) s = fma(-cf[li(p, i)], w[p], s);
    w[i] = s * cf[15 + i];
  }
}

// m = Bd_k' P (rows 6..8: bv(); rows 9..11: the record's bw)
template <int VAR>
__device__ __forceinline__ void bdt_times(const double (&P)[12], const double* rec, double dtm, double (&m)[6]) {
  const double cp = rec[R_CS], sp = rec[R_CS + 1];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double acc = 0.0;
    if (c < 3) {
      if constexpr (VAR == 3) {
        acc = dtm * P[6 + c];
      } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) acc = fma(bv<VAR>(r, c, dtm, cp, sp), P[6 + r], acc);
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) acc = fma(rec[R_BW + 6 * r + c], P[9 + r], acc);
    m[c] = acc;
  }
}

}  // namespace

}  // namespace hmpc
