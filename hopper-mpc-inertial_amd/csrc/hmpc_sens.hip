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

#include <utility>

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
  bdt_times<VAR>(P, rec, dtm, g);
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

// Step C of the elimination of W nu = p_0, row per lane: the pivot row comes
// from lane C by readlane (every register index is a template constant, so
// the rows stay in registers), W's columns in blocks of eight up to nq.
template <int C>
__device__ __forceinline__ void eliminate_step(double (&G)[64], double (&P)[12], double D0, int nq, int lane,
                                               int& singular, double& rinv_own) {
  if (C >= nq) return;
  const double piv = rdlane(G[C], C);
  const double d0 = rdlane(D0, C);
  const bool ok = piv > kPivotFloor * d0 && piv > 0.0;
  const double rinv = ok ? 1.0 / piv : 0.0;
  singular |= ok ? 0 : 1;
  rinv_own = lane == C ? rinv : rinv_own;
  const double f = lane > C ? G[C] * rinv : 0.0;
#pragma unroll
  for (int i = 0; i < 12; ++i) P[i] = fma(-f, rdlane(P[i], C), P[i]);
#pragma unroll
  for (int jb = 0; jb < 64; jb += 8) {
    if (jb + 7 > C && jb < nq) {
#pragma unroll
      for (int j = jb; j < jb + 8; ++j)
        if (j > C) G[j] = fma(-f, rdlane(G[j], C), G[j]);
    }
  }
}
template <int... Cs>
__device__ __forceinline__ void eliminate(std::integer_sequence<int, Cs...>, double (&G)[64], double (&P)[12],
                                          double D0, int nq, int lane, int& singular, double& rinv_own) {
  (eliminate_step<Cs>(G, P, D0, nq, lane, singular, rinv_own), ...);
}
// nu_C = rhs_C / pivot_C stays in lane C (0 for a dropped row); the rows above take it out
template <int C>
__device__ __forceinline__ void back_step_nu(const double (&G)[64], double (&P)[12], int nq, int lane,
                                             double rinv_own) {
  if (C >= nq) return;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const double nc = rdlane(P[i] * rinv_own, C);
    P[i] = lane == C ? nc : (lane < C ? fma(-G[C], nc, P[i]) : P[i]);
  }
}
template <int... Cs>
__device__ __forceinline__ void back_substitute(std::integer_sequence<int, Cs...>, const double (&G)[64],
                                                double (&P)[12], int nq, int lane, double rinv_own) {
  (back_step_nu<63 - Cs>(G, P, nq, lane, rinv_own), ...);
}

struct SensShared {
  double rec[65 * kRec];     // one spare record / row / slot for the idle lanes
  double K[64 * kKst + 8];
  double cf[64 * kCst];
  double tile[64 * 6];       // pass 1: Bd'P | Bd'P Ad, [12][6] each; pass 2: y, [64][6]
  double nu[65 * 12];        // load on stage k's z row for dx_0 column i, [k][i]
  int zidx[65];
};

template <int VAR>
__global__ void __launch_bounds__(64) sens_kernel(SensArgs a) {
  __shared__ __attribute__((aligned(16))) SensShared sh;
  const int lane = threadIdx.x;
  const int N = a.N, ns = a.n_stages;
  const double dt = a.dt, dtm = a.dt / a.m;
  const bool st = lane < N;          // this lane owns a stage
  const int k = st ? lane : N - 1;   // clamped: loads stay in bounds
  const bool colane = lane < 12;     // this lane owns a column of P / of S
  const int col = colane ? lane : 0;

  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    const double mu = a.mu ? a.mu[b] : a.mu_default;
    const double tol = a.act_tol;
    // ------------------------------------------------------------ pass 0
    const double* xl = a.x_lin + (b * (N + 1) + k) * 12;
    const double* pfp = a.pf + (b * N + k) * 3;
    double u[6], cs[2], bw[18];
#pragma unroll
    for (int c = 0; c < 6; ++c) u[c] = a.u[(b * N + k) * 6 + c];
    const bool stance = a.C[b * N + k] != 0.0;
    {
      const double p[3] = {xl[0], xl[1], xl[2]};
      const double pfk[3] = {pfp[0], pfp[1], pfp[2]};
      stage_dynamics_vals<VAR, double>(0, xl[5], p, pfk, a.Jinv, a.rh, dt, cs, bw);
    }
    // z row of this stage (stage 0 sits on the fixed x_0)
    const double zslack = a.x[(b * (N + 1) + k) * 12 + 2] - kZmin;
    const bool zact = st && lane >= 1 && zslack <= tol * (1.0 + kZmin);
    double tm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double lim = tau_lim(3 + c);
      const bool pin = lim - u[3 + c] <= tol * (1.0 + lim) || u[3 + c] + lim <= tol * (1.0 + lim);
      tm[c] = pin ? 0.0 : 1.0;
    }
    // forces: stage class, active rows and projector, branch-free (selects).
    // Swing, and stance with fz = 0 (five dependent rows of rank 3): pinned.
    const bool reg = stance && !(u[2] <= tol);
    double pi[6];
    {
      const double s0 = mu * u[2] - u[0], s1 = mu * u[2] + u[0];
      const double s2 = mu * u[2] - u[1], s3 = mu * u[2] + u[1];
      const bool a3 = s0 <= tol, a4 = s1 <= tol, a5 = s2 <= tol, a6 = s3 <= tol;
      const bool xp = a3 && (!a4 || s0 <= s1);
      const bool yp = a5 && (!a6 || s2 <= s3);
      int fm = xp ? A_FXP : (a4 ? A_FXM : 0);
      if (VAR == 3) fm |= yp ? A_FYP : (a6 ? A_FYM : 0);
      fm |= (kFzMax - u[2] <= tol * (1.0 + kFzMax)) ? A_FZU : 0;
      // both signs of a pair active while fz > tol (mu < 1, fz <= tol / mu): the pair
      // spans (e_axis, e_z), which the kept row and a pinned fz span as well
      fm |= ((a3 && a4) || (VAR == 3 && a5 && a6)) ? A_FZU : 0;
      force_projector<VAR>(reg ? fm : 0, mu, pi);
#pragma unroll
      for (int i = 0; i < 6; ++i) pi[i] = reg ? pi[i] : 0.0;
    }
    __syncthreads();   // the previous instance's reads of the shared block are done
    {
      double* rec = sh.rec + kRec * (st ? lane : 64);   // idle lanes write a spare record
      rec[R_CS] = cs[0];
      rec[R_CS + 1] = cs[1];
#pragma unroll
      for (int i = 0; i < 18; ++i) rec[R_BW + i] = bw[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) rec[R_PI + i] = pi[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) rec[R_TM + c] = tm[c];
#pragma unroll
      for (int i = 0; i < 12; ++i) sh.nu[12 * lane + i] = 0.0;
    }
    // active z rows -> lanes 0..nq-1, in stage order (nq <= N - 1 <= 63: every row has a lane)
    const unsigned long long zb = __ballot(zact);
    const int nq = __popcll(zb);
    sh.zidx[zact ? __popcll(zb & ((1ull << lane) - 1ull)) : 64] = lane;   // slot 64: spare
    __syncthreads();
    const int zi = sh.zidx[lane];   // (unassigned lanes read a stale slot: selected away)
    const int zstage = lane < nq ? zi : -1;

    // ------------------------------------------------------------ pass 1
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
      bdt_times<VAR>(P, rec, dtm, W);          // column `lane` of Bd'P
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
        // own row of W from broadcast reads of the tile, eight columns a block
#pragma unroll
        for (int jb = 0; jb < 64; jb += 8) {
          if (jb < nq) {
#pragma unroll
            for (int j = jb; j < jb + 8; ++j) {
              const double* t = sh.tile + 6 * j;
              double acc = G[j];
#pragma unroll
              for (int c = 0; c < 6; ++c) acc = fma(y[c], t[c], acc);
              G[j] = acc;
            }
          }
        }
        __syncthreads();
      }
      // W nu = p_0, twelve right-hand sides (the registers of P).  A pivot
      // below the floor: the row is dependent given the pinned inputs (the
      // stage-1 row always is) -- flag it, drop it, its nu stays 0.
      double rinv_own = 0.0;
      eliminate(std::make_integer_sequence<int, 64>(), G, P, D0, nq, lane, singular, rinv_own);
      back_substitute(std::make_integer_sequence<int, 64>(), G, P, nq, lane, rinv_own);
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
