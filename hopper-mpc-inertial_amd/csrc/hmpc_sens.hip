// hmpc_sens.hip -- first-order sensitivity of the optimum to the measured
// state, S[b,k,c,i] = d u*_k[c] / d x_in[i], at the active set of a given
// primal point (x, u) of the reference's QP (3f :96-153, 2f :96-151).  With
// every active row held as an equality, S is the minimiser of an
// equality-constrained LQR in (dx, du) started at dx_0 = e_i.
// A post-processing kernel like hmpc_kkt.hip: it touches no solve kernel.
//
// One wavefront per instance, grid-stride over B, fp64:
//
//   pass 0  lane k < N takes stage k: dynamics, slacks, stage class, active
//           mask and the projector Pi_k onto the free input directions; stage
//           records go to LDS.  The active z rows are balloted onto lanes 0..q-1.
//   pass 1  projected Riccati recursion, serial over k = N-1 .. 0.  Lane j < 12
//           holds column j of P (12 registers).  Bd'P is per lane; Bd'P Ad and
//           P Ad are lane-parallel (adt_lane: a row shift by 6 and the three-
//           lane cos/sin combination); G = 2 lambda R + Bd'P Bd, G~ = Pi G Pi +
//           (I - Pi) and its 6 x 6 Cholesky factor (reciprocal pivots) are
//           formed by every lane from a broadcast tile; lane j then solves for
//           column j of K_k = -Pi G~^-1 Pi Bd'P Ad.  K_k and the factor stay in LDS.
//   pass 2  (q > 0) lane j < q carries the costate of a unit load on its z row,
//           p_k = (Ad + Bd K)' p_{k+1} + e_2 [k = k_j].  y = C^-1 Pi Bd' p_{k+1}
//           goes to an LDS tile; each lane accumulates its row of the
//           compliance matrix W = sum_k y y' from broadcast reads.  p_0 is the
//           z response to the twelve dx_0 columns: the right-hand sides.  No
//           forward pass is needed.  W nu = p_0 by row-per-lane elimination,
//           the pivot row by readlane; a pivot below the floor drops the row.
//   pass 3  lane i < 12: the same backward recursion with the combined loads
//           nu[., i] gives the feed-forward v_k, parked in S itself (the lane
//           reads back what it wrote); then the forward roll-out
//           du_k = K_k dx_k + v_k overwrites S[k] for k < n_stages.
//
// No MFMA: the dense products are 6 x 12 x 6 and sit outside the dependent
// chain that bounds pass 1.
#include <hip/hip_runtime.h>

#include "hmpc_internal.h"
#include "hmpc_model.h"
#include "hmpc_sens_common.h"

namespace hmpc {

namespace {

// The backward step the sweeps share: g = Bd_k' p, y = C_k^-1 Pi_k g, then
// p <- Ad_k' p + K_k' g (= (Ad + Bd K)' p).  The caller adds the stage's load.
template <int VAR>
__device__ __forceinline__ void sweep_step(const double* rec, const double* cf, const double* Kk, double dt,
                                           double dtm, double (&P)[12], double (&y)[6]) {
  double g[6];
  bdt_times<VAR>(P, rec[R_CS], rec[R_CS + 1], rec + R_BW, dtm, g);
#pragma unroll
  for (int c = 0; c < 6; ++c) y[c] = g[c];
  pi_apply(rec + R_PI, y);
  chol_fwd(cf, y);
  adt_times(P, dt, rec[R_CS], rec[R_CS + 1]);
#pragma unroll
  for (int r = 0; r < 12; ++r) {
    double acc = P[r];
#pragma unroll
    for (int c = 0; c < 6; ++c) acc = fma(Kk[12 * c + r], g[c], acc);
    P[r] = acc;
  }
}

struct SensShared : RiccatiShared {
  double nu[65 * 12];        // load on stage k's z row for dx_0 column i, [k][i]
  int zidx[65];
};

template <int VAR>
__global__ void __launch_bounds__(64) sens_kernel(SensArgs a) {
  __shared__ __attribute__((aligned(16))) SensShared sh;
  const int lane = threadIdx.x;
  const int N = a.N, ns = a.n_stages;
  const double dt = a.dt, dtm = a.dt / a.m;
  const bool colane = lane < 12;     // this lane owns a column of P / of S
  const int col = colane ? lane : 0;

  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    const double mu = a.mu ? a.mu[b] : a.mu_default;
    // ------------------------------------------------------------ pass 0
    int nq;
    const int zstage = stage_records<VAR>(a, sh, sh.zidx, b, mu, [&] {
#pragma unroll
      for (int i = 0; i < 12; ++i) sh.nu[12 * lane + i] = 0.0;
    }, nq);
    // ------------------------------------------------------------ pass 1
    // riccati_pass (hmpc_sens_common.h) written out: called as a function, which
    // reaches the LDS block through a generic reference, this kernel takes one
    // more VGPR spill (74, 300 B scratch against 73, 296 B) in every form tried
    // (DESIGN.md 4.8).  Keep the two texts equal.
    double P[12];
#pragma unroll
    for (int r = 0; r < 12; ++r) P[r] = lane == r ? 2.0 * kTermQ * kQ[r] : 0.0;
    double* tW = sh.tile;
    double* tH = sh.tile + 72;
#pragma unroll 1
    for (int kk = N - 1; kk >= 0; --kk) {
      const double* rec = sh.rec + kRec * kk;
      const double cp = rec[R_CS], sp = rec[R_CS + 1];
      double W[6], H[6];
      bdt_times<VAR>(P, rec[R_CS], rec[R_CS + 1], rec + R_BW, dtm, W);   // column `lane` of Bd'P
#pragma unroll
      for (int c = 0; c < 6; ++c) H[c] = adt_lane(W[c], dt, cp, sp);   // ... of Bd'P Ad
      {
        const int slot = colane ? 6 * lane : 144;   // idle lanes: spare slots past both tiles
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          tW[slot + c] = W[c];
          tH[slot + c] = H[c];
        }
      }
      __syncthreads();
      // G = 2 lambda R + Bd'P Bd (rows 6..11 of Bd), then G~ = Pi G Pi + (I - Pi)
      double Gm[6][6];
      const double r2 = kk == N - 1 ? 0.0 : 2.0 * kRdiag;
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int d = 0; d <= c; ++d) {
          double acc = c == d ? r2 : 0.0;
          if (d < 3) {
#pragma unroll
            for (int r = 0; r < 3; ++r) acc = fma(tW[6 * (6 + r) + c], bv<VAR>(r, d, dtm, cp, sp), acc);
          }
#pragma unroll
          for (int r = 0; r < 3; ++r) acc = fma(tW[6 * (9 + r) + c], rec[R_BW + 6 * r + d], acc);
          Gm[c][d] = acc;
          Gm[d][c] = acc;
        }
#pragma unroll
      for (int r = 0; r < 6; ++r) pi_apply(rec + R_PI, Gm[r]);   // rows of G Pi (G is symmetric)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double v[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) v[r] = Gm[r][c];
        pi_apply(rec + R_PI, v);
#pragma unroll
        for (int r = 0; r < 6; ++r) Gm[r][c] = v[r];
      }
      Gm[0][0] += 1.0 - rec[R_PI + 0];
      Gm[1][0] -= rec[R_PI + 1];
      Gm[2][0] -= rec[R_PI + 2];
      Gm[1][1] += 1.0 - rec[R_PI + 3];
      Gm[2][1] -= rec[R_PI + 4];
      Gm[2][2] += 1.0 - rec[R_PI + 5];
#pragma unroll
      for (int c = 0; c < 3; ++c) Gm[3 + c][3 + c] += 1.0 - rec[R_TM + c];
      double cf[kCst];
      chol6(Gm, cf);
#pragma unroll
      for (int i = 0; i < kCst; ++i) sh.cf[kCst * kk + i] = cf[i];   // every lane, the same values
      // column `lane` of K = -Pi G~^-1 Pi (Bd'P Ad)
      double Kc[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) Kc[c] = H[c];
      pi_apply(rec + R_PI, Kc);
      chol_fwd(cf, Kc);
      chol_bwd(cf, Kc);
      pi_apply(rec + R_PI, Kc);
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        Kc[c] = -Kc[c];
        sh.K[colane ? kKst * kk + 12 * c + lane : 64 * kKst + c] = Kc[c];   // idle lanes: the spare slots
      }
      // P <- 2 Q + Ad'P Ad + (Bd'P Ad)' K
      if (kk > 0) {
#pragma unroll
        for (int r = 0; r < 12; ++r) P[r] = adt_lane(P[r], dt, cp, sp);   // P Ad
        adt_times(P, dt, cp, sp);
#pragma unroll
        for (int r = 0; r < 12; ++r) {
          double acc = P[r];
#pragma unroll
          for (int c = 0; c < 6; ++c) acc = fma(tH[6 * r + c], Kc[c], acc);
          P[r] = acc + (lane == r ? 2.0 * kQ[r] : 0.0);
        }
      }
      __syncthreads();
    }

    // ------------------------------------------------------------ pass 2
    int singular = 0;
    if (nq > 0) {
      double G[64], y[6];
#pragma unroll
      for (int j = 0; j < 64; ++j) G[j] = 0.0;
#pragma unroll
      for (int r = 0; r < 12; ++r) P[r] = 0.0;
      double D0 = 0.0;
#pragma unroll 1
      for (int kk = N - 1; kk >= 0; --kk) {
        sweep_step<VAR>(sh.rec + kRec * kk, sh.cf + kCst * kk, sh.K + kKst * kk, dt, dtm, P, y);
        P[2] += zstage == kk ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          sh.tile[6 * lane + c] = y[c];
          D0 = fma(y[c], y[c], D0);
        }
        __syncthreads();
        gram_row(G, y, sh.tile, nq);   // own row of W
        __syncthreads();
      }
      // W nu = p_0, twelve right-hand sides (the registers of P).  A pivot
      // below the floor: the row is dependent given the pinned inputs (the
      // stage-1 row always is) -- flag it, drop it, its nu stays 0.
      solve_rows<12, 0>(G, P, D0, nq, lane, singular);
#pragma unroll
      for (int i = 0; i < 12; ++i) sh.nu[12 * (zstage >= 0 ? zstage : 64) + i] = P[i];   // row 64: spare
      __syncthreads();
    }

    // ------------------------------------------------------------ pass 3
    double* Sb = a.S + b * ns * 72 + col;   // S[b][k][c][col] = Sb[72 k + 12 c]
    if (nq > 0) {
      double y[6];
#pragma unroll
      for (int r = 0; r < 12; ++r) P[r] = 0.0;
#pragma unroll 1
      for (int kk = N - 1; kk >= 0; --kk) {
        const double* rec = sh.rec + kRec * kk;
        const double* cf = sh.cf + kCst * kk;
        sweep_step<VAR>(rec, cf, sh.K + kKst * kk, dt, dtm, P, y);
        P[2] += sh.nu[12 * kk + col];
        // v_k = -Pi C'^-1 y, parked in S[k] until the roll-out below
        chol_bwd(cf, y);
        pi_apply(rec + R_PI, y);
        if (colane && kk < ns) {
#pragma unroll
          for (int c = 0; c < 6; ++c) Sb[72 * kk + 12 * c] = -y[c];
        }
      }
    }
    {
      double x[12];
#pragma unroll
      for (int r = 0; r < 12; ++r) x[r] = col == r ? 1.0 : 0.0;
#pragma unroll 1
      for (int kk = 0; kk < ns; ++kk) {
        const double* rec = sh.rec + kRec * kk;
        const double* Kk = sh.K + kKst * kk;
        double du[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          double acc = (nq > 0 && colane) ? Sb[72 * kk + 12 * c] : 0.0;
#pragma unroll
          for (int r = 0; r < 12; ++r) acc = fma(Kk[12 * c + r], x[r], acc);
          du[c] = acc;
        }
        if (colane) {
#pragma unroll
          for (int c = 0; c < 6; ++c) Sb[72 * kk + 12 * c] = du[c];
        }
        // dx <- Ad dx + Bd du
        const double cp = rec[R_CS], sp = rec[R_CS + 1];
        ad_times(x, dt, cp, sp);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          double acc = x[6 + r];
#pragma unroll
          for (int c = 0; c < 3; ++c) acc = fma(bv<VAR>(r, c, dtm, cp, sp), du[c], acc);
          x[6 + r] = acc;
          acc = x[9 + r];
#pragma unroll
          for (int c = 0; c < 6; ++c) acc = fma(rec[R_BW + 6 * r + c], du[c], acc);
          x[9 + r] = acc;
        }
      }
    }
    if (a.flags && lane == 0) a.flags[b] = singular;   // HMPC_SENS_SINGULAR
  }
}

}  // namespace

void launch_sens(int variant, const SensArgs& a, hipStream_t s) {
  if (a.B <= 0) return;
  // one wave per workgroup, grid-stride; the LDS block allows two workgroups
  // per CU, so 1024 workgroups are two rounds of the chip
  const unsigned grid = (unsigned)(a.B < 1024 ? a.B : 1024);
  if (variant == 2) hipLaunchKernelGGL(sens_kernel<2>, dim3(grid), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(sens_kernel<3>, dim3(grid), dim3(64), 0, s, a);
}

}  // namespace hmpc
