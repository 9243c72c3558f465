// hmpc_sens_common.h -- the one home of what the post-solve kernels share
// (hmpc_kkt.hip: multipliers, hmpc_sens.hip: forward mode, hmpc_vjp_kernel.h:
// reverse mode): the active-set rule of a stage, the
// Gram-Schmidt of its force rows and the projector Pi_k, Bd_k' times a costate,
// the 6 x 6 factor of G~_k on reciprocal pivots, the row-per-lane elimination,
// and passes 0 and 1 of the two kernels that differentiate the solve.
// Device code only; internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "hmpc_internal.h"
#include "hmpc_model.h"

namespace hmpc {

namespace {

// the stage record of sens / vjp (kkt keeps a longer one of its own)
constexpr int kRec = 29;   // doubles per stage record
constexpr int R_CS = 0;    // cos, sin of the linearisation yaw
constexpr int R_BW = 2;    // rows 9..11 of Bd_k, [3][6]
constexpr int R_PI = 20;   // force projector, symmetric: xx xy xz yy yz zz
constexpr int R_TM = 26;   // torque mask (1: free), contiguous with R_PI
constexpr int kKst = 72;   // K_k, [6][12]
constexpr int kCst = 21;   // factor of G~_k: 15 strict-lower entries, 6 reciprocal diagonals
constexpr double kPivotFloor = 1e-11;   // relative to the row's own diagonal

// active-mask bits: the force rows, and the torque bounds (<< c for torque c)
constexpr int A_FXP = 1, A_FXM = 2, A_FYP = 4, A_FYM = 8, A_FZU = 16;
constexpr int A_TUP = 32, A_TLO = 256;

__device__ __forceinline__ constexpr int li(int i, int j) { return i * (i - 1) / 2 + j; }   // i > j

// ---------------------------------------------------------------- active set
// The active-set rule of one stage: a row is active when its slack is at most
// tol (1 + |bound|).  Every post-solve kernel reads the rule from here.
struct StageClass {
  bool stance, apex, reg;   // apex: stance with fz = 0 (five dependent rows of rank 3); reg: the other stance stages
  double zslack;            // x_k[2] - z_min
  bool zact;                // the z row is active (the caller leaves out stage 0, which sits on the fixed x_0)
  int tmask;                // A_TUP << c / A_TLO << c: torque c sits on its upper / lower bound
  double fs[4];             // slacks of the friction rows, slots 3..6: mu fz - fx, + fx, - fy, + fy
  bool a3, a4, a5, a6;      // those rows are active
  bool xp, yp;              // the row kept of a pair is the + row (the nearer one when both are active)
  int fm;                   // the force rows held at a regular stage: one of each pair (3f), fz <= f_max
};

template <int VAR>
__device__ __forceinline__ StageClass classify_stage(const double (&u)[6], double xz, bool stance, double mu,
                                                     double tol) {
  StageClass s;
  s.stance = stance;
  s.apex = stance && u[2] <= tol;
  s.reg = stance && !s.apex;
  s.zslack = xz - kZmin;
  s.zact = s.zslack <= tol * (1.0 + kZmin);
  s.tmask = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double lim = tau_lim(3 + c);
    const bool up = lim - u[3 + c] <= tol * (1.0 + lim);
    const bool lo = !up && u[3 + c] + lim <= tol * (1.0 + lim);
    s.tmask |= up ? (A_TUP << c) : 0;
    s.tmask |= lo ? (A_TLO << c) : 0;
  }
  s.fs[0] = mu * u[2] - u[0];
  s.fs[1] = mu * u[2] + u[0];
  s.fs[2] = mu * u[2] - u[1];
  s.fs[3] = mu * u[2] + u[1];
  s.a3 = s.fs[0] <= tol;
  s.a4 = s.fs[1] <= tol;
  s.a5 = s.fs[2] <= tol;
  s.a6 = s.fs[3] <= tol;
  s.xp = s.a3 && (!s.a4 || s.fs[0] <= s.fs[1]);
  s.yp = s.a5 && (!s.a6 || s.fs[2] <= s.fs[3]);
  s.fm = s.xp ? A_FXP : (s.a4 ? A_FXM : 0);
  if (VAR == 3) s.fm |= s.yp ? A_FYP : (s.a6 ? A_FYM : 0);
  s.fm |= (kFzMax - u[2] <= tol * (1.0 + kFzMax)) ? A_FZU : 0;
  return s;
}

// 1: torque c is free, 0: pinned at a bound
__device__ __forceinline__ double torque_free(const StageClass& s, int c) {
  return (s.tmask & ((A_TUP | A_TLO) << c)) ? 0.0 : 1.0;
}

// sens / vjp hold every active row as an equality, so both signs of a friction
// pair active while fz > tol (mu < 1, fz <= tol / mu) count: the pair spans
// (e_axis, e_z), which the kept row and a pinned fz span as well.  kkt's mask
// names the rows that receive a multiplier, and fz <= f_max is not active
// there: it keeps the nearer row alone and does not apply this.
template <int VAR>
__device__ __forceinline__ bool both_signs(const StageClass& s) {
  return (s.a3 && s.a4) || (VAR == 3 && s.a5 && s.a6);
}

// ---------------------------------------------------------------- force rows
// Orthonormal basis (modified Gram-Schmidt) of the active force rows of a
// regular stance stage: at most one of +-fx - mu fz, one of +-fy - mu fz (2f:
// the fixed fy) and fz <= f_max; always independent.  ri holds the
// reciprocal norms (0 for an absent row).
struct StageQr {
  double q[3][3];
  double r01, r02, r12;
  double ri[3];
};
template <int VAR>
__device__ __forceinline__ void stage_qr(int mask, double mu, StageQr& s) {
  const bool px = (mask & (A_FXP | A_FXM)) != 0;
  const bool py = VAR == 2 ? true : (mask & (A_FYP | A_FYM)) != 0;
  const bool pz = (mask & A_FZU) != 0;
  const double sx = (mask & A_FXP) ? 1.0 : -1.0;
  const double sy = (mask & A_FYP) ? 1.0 : -1.0;
  double a[3][3] = {{px ? sx : 0.0, 0.0, px ? -mu : 0.0},
                    {0.0, py ? (VAR == 2 ? 1.0 : sy) : 0.0, (py && VAR != 2) ? -mu : 0.0},
                    {0.0, 0.0, pz ? 1.0 : 0.0}};
  const bool pres[3] = {px, py, pz};
  double r[3][3] = {};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < i; ++j) {
      r[j][i] = s.q[j][0] * a[i][0] + s.q[j][1] * a[i][1] + s.q[j][2] * a[i][2];
#pragma unroll
      for (int c = 0; c < 3; ++c) a[i][c] = fma(-r[j][i], s.q[j][c], a[i][c]);
    }
    const double n2 = a[i][0] * a[i][0] + a[i][1] * a[i][1] + a[i][2] * a[i][2];
    s.ri[i] = (pres[i] && n2 > 0.0) ? 1.0 / sqrt(n2) : 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) s.q[i][c] = a[i][c] * s.ri[i];
  }
  s.r01 = r[0][1]; s.r02 = r[0][2]; s.r12 = r[1][2];
}

// I - Q Q' for those rows
template <int VAR>
__device__ __forceinline__ void force_projector(int mask, double mu, double (&pi)[6]) {
  StageQr s;
  stage_qr<VAR>(mask, mu, s);
  pi[0] = 1.0; pi[1] = 0.0; pi[2] = 0.0; pi[3] = 1.0; pi[4] = 0.0; pi[5] = 1.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    pi[0] = fma(-s.q[i][0], s.q[i][0], pi[0]);
    pi[1] = fma(-s.q[i][0], s.q[i][1], pi[1]);
    pi[2] = fma(-s.q[i][0], s.q[i][2], pi[2]);
    pi[3] = fma(-s.q[i][1], s.q[i][1], pi[3]);
    pi[4] = fma(-s.q[i][1], s.q[i][2], pi[4]);
    pi[5] = fma(-s.q[i][2], s.q[i][2], pi[5]);
  }
}

// v <- Pi v: pr = a record's projector (6) and torque mask (3)
__device__ __forceinline__ void pi_apply(const double* pr, double (&v)[6]) {
  const double f0 = pr[0] * v[0] + pr[1] * v[1] + pr[2] * v[2];
  const double f1 = pr[1] * v[0] + pr[3] * v[1] + pr[4] * v[2];
  const double f2 = pr[2] * v[0] + pr[4] * v[1] + pr[5] * v[2];
  v[0] = f0; v[1] = f1; v[2] = f2;
#pragma unroll
  for (int c = 0; c < 3; ++c) v[3 + c] *= pr[6 + c];
}

// ---------------------------------------------------------------- 6 x 6 factor
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

// m = Bd_k' P (rows 6..8: bv() at the yaw cp, sp; rows 9..11: bw, [3][6])
template <int VAR>
__device__ __forceinline__ void bdt_times(const double (&P)[12], double cp, double sp, const double* bw, double dtm,
                                          double (&m)[6]) {
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
    for (int r = 0; r < 3; ++r) acc = fma(bw[6 * r + c], P[9 + r], acc);
    m[c] = acc;
  }
}

// ---------------------------------------------------------------- normal equations, row per lane
// Own Gram row from broadcast reads of the tile ([64][6], row j written by lane
// j), eight columns a block up to ncols
__device__ __forceinline__ void gram_row(double (&G)[64], const double (&y)[6], const double* tile, int ncols) {
#pragma unroll
  for (int jb = 0; jb < 64; jb += 8) {
    if (jb < ncols) {
#pragma unroll
      for (int j = jb; j < jb + 8; ++j) {
        const double* t = tile + 6 * j;
        double acc = G[j];
#pragma unroll
        for (int c = 0; c < 6; ++c) acc = fma(y[c], t[c], acc);
        G[j] = acc;
      }
    }
  }
}

// Step C of the elimination of G nu = rhs over rows R0 .. R0 + nq - 1, NR
// right-hand sides: the pivot row comes from lane C by readlane (every register
// index is a template constant, so the rows stay in registers), G's columns in
// blocks of eight.  A pivot below the floor (relative to D0, the row's own
// diagonal before the elimination) drops the row: flagged, its nu stays 0.
template <int NR, int R0, int C>
__device__ __forceinline__ void eliminate_step(double (&G)[64], double (&rhs)[NR], double D0, int nq, int lane,
                                               int& singular, double& rinv_own) {
  if (C >= nq + R0) return;
  const double piv = rdlane(G[C], C);
  const double d0 = rdlane(D0, C);
  const bool ok = piv > kPivotFloor * d0 && piv > 0.0;
  const double rinv = ok ? 1.0 / piv : 0.0;
  singular |= ok ? 0 : 1;
  rinv_own = lane == C ? rinv : rinv_own;
  const double f = lane > C ? G[C] * rinv : 0.0;
#pragma unroll
  for (int i = 0; i < NR; ++i) rhs[i] = fma(-f, rdlane(rhs[i], C), rhs[i]);
#pragma unroll
  for (int jb = 0; jb < 64; jb += 8) {
    if (jb + 7 > C && jb < nq + R0) {
#pragma unroll
      for (int j = jb; j < jb + 8; ++j)
        if (j > C) G[j] = fma(-f, rdlane(G[j], C), G[j]);
    }
  }
}
// nu_C = rhs_C / pivot_C stays in lane C (0 for a dropped row); the rows above take it out
template <int NR, int R0, int C>
__device__ __forceinline__ void back_step_nu(const double (&G)[64], double (&rhs)[NR], int nq, int lane,
                                             double rinv_own) {
  if (C >= nq + R0) return;
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const double nc = rdlane(rhs[i] * rinv_own, C);
    rhs[i] = lane == C ? nc : (lane < C ? fma(-G[C], nc, rhs[i]) : rhs[i]);
  }
}
template <int NR, int R0, int... Cs>
__device__ __forceinline__ void solve_rows(std::integer_sequence<int, Cs...>, double (&G)[64], double (&rhs)[NR],
                                           double D0, int nq, int lane, int& singular) {
  double rinv_own = 0.0;
  (eliminate_step<NR, R0, R0 + Cs>(G, rhs, D0, nq, lane, singular, rinv_own), ...);
  (back_step_nu<NR, R0, 63 - Cs>(G, rhs, nq, lane, rinv_own), ...);
}
// G nu = rhs: lane C in R0 .. R0 + nq - 1 leaves with its nu in rhs
template <int NR, int R0>
__device__ __forceinline__ void solve_rows(double (&G)[64], double (&rhs)[NR], double D0, int nq, int lane,
                                           int& singular) {
  solve_rows<NR, R0>(std::make_integer_sequence<int, 64 - R0>(), G, rhs, D0, nq, lane, singular);
}

// ---------------------------------------------------------------- passes 0 and 1 of sens / vjp
// the LDS block SensShared and VjpShared begin with
struct RiccatiShared {
  double rec[65 * kRec];     // one spare record / row / slot for the idle lanes
  double K[64 * kKst + 8];
  double cf[64 * kCst];
  double tile[64 * 6];       // pass 1: Bd'P | Bd'P Ad, [12][6] each; pass 2: y, [64][6]
};

// Pass 0, lane k < N takes stage k: dynamics, stage class, active rows and the
// projector Pi_k onto the free input directions, branch-free (selects); the
// records go to LDS, the active z rows are balloted onto lanes 0..nq-1 in stage
// order (nq <= N - 1 <= 63).  fill() writes the kernel's own LDS tables between
// the two barriers.  Returns this lane's z stage (-1: none).
template <int VAR, class Args, class Fill>
__device__ __forceinline__ int stage_records(const Args& a, RiccatiShared& sh, int* zidx, int64_t b, double mu,
                                             Fill&& fill, int& nq) {
  const int lane = threadIdx.x;
  const int N = a.N;
  const bool st = lane < N;          // this lane owns a stage
  const int k = st ? lane : N - 1;   // clamped: loads stay in bounds
  const double* xl = a.x_lin + (b * (N + 1) + k) * 12;
  const double* pfp = a.pf + (b * N + k) * 3;
  double u[6], cs[2], bw[18];
#pragma unroll
  for (int c = 0; c < 6; ++c) u[c] = a.u[(b * N + k) * 6 + c];
  const bool stance = a.C[b * N + k] != 0.0;
  {
    const double p[3] = {xl[0], xl[1], xl[2]};
    const double pfk[3] = {pfp[0], pfp[1], pfp[2]};
    stage_dynamics_vals<VAR, double>(0, xl[5], p, pfk, a.Jinv, a.rh, a.dt, cs, bw);
  }
  const StageClass sc = classify_stage<VAR>(u, a.x[(b * (N + 1) + k) * 12 + 2], stance, mu, a.act_tol);
  const bool zact = st && lane >= 1 && sc.zact;
  // Swing, and stance with fz = 0: every force component is pinned
  double pi[6];
  force_projector<VAR>(sc.reg ? (sc.fm | (both_signs<VAR>(sc) ? A_FZU : 0)) : 0, mu, pi);
#pragma unroll
  for (int i = 0; i < 6; ++i) pi[i] = sc.reg ? pi[i] : 0.0;
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
    for (int c = 0; c < 3; ++c) rec[R_TM + c] = torque_free(sc, c);
  }
  fill();
  const unsigned long long zb = __ballot(zact);
  nq = __popcll(zb);
  zidx[zact ? __popcll(zb & ((1ull << lane) - 1ull)) : 64] = lane;   // slot 64: spare
  __syncthreads();
  const int zi = zidx[lane];   // (unassigned lanes read a stale slot: selected away)
  return lane < nq ? zi : -1;
}

// Pass 1, the projected Riccati recursion, serial over k = N-1 .. 0.  Lane j <
// 12 holds column j of P (12 registers).  Bd'P is per lane; Bd'P Ad and P Ad
// are lane-parallel (adt_lane); G = 2 lambda R + Bd'P Bd, G~ = Pi G Pi +
// (I - Pi) and its factor are formed by every lane from a broadcast tile; lane
// j then solves for column j of K_k = -Pi G~^-1 Pi Bd'P Ad.  K_k and the factor
// stay in LDS.
template <int VAR>
__device__ __forceinline__ void riccati_pass(RiccatiShared& sh, int N, double dt, double dtm) {
  const int lane = threadIdx.x;
  const bool colane = lane < 12;     // this lane owns a column of P
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
    bdt_times<VAR>(P, cp, sp, rec + R_BW, dtm, W);   // column `lane` of Bd'P
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
}

}  // namespace

}  // namespace hmpc
