// hmpc_vjp_lin.hip -- hmpc_vjp_lin_batch: the adjoint kernel of hmpc_vjp_kernel.h
// with a second lane = stage epilogue for the gradients in the linearisation
// point and the friction coefficient.  For any parameter of
// Ad_k, Bd_k,
//   grad = sum_k p_{k+1}'(dAd_k dx_k + dBd_k du_k) + pt_{k+1}'(dAd_k x*_k + dBd_k u*_k)
// with p the original problem's dynamics costate and pt the adjoint's.
//
//   position  x_lin[k][0:3] enters through pf[k] - x_lin[k][0:3] alone: -grad_pf[k].
//   yaw       x_lin[k][5] turns Ad[3:6, 9:12] = dt rz, rows 9..11 of Bd_k and (2f)
//             Bd[6:9, 0:3] = dt/m rz'.  d rz / d psi has a zero third row and
//             column, so of the costates only components 3..5, 9..11 and (2f) 6, 7
//             are needed, and 6, 7 follow from 0, 1: none of them sees a z-row
//             multiplier (those sit in components 2 and 8).  All are suffix
//             sums over the horizon (the DPP scan of the first epilogue).
//   mu        only the friction rows s f - mu fz <= 0 depend on it, d row / d mu =
//             -e_fz: per held row -lam du_k[fz] + b fz*_k, b the adjoint's
//             multiplier of the row.  The held force rows are triangular in
//             (fx | fy | fz), so b = s rho[axis] with rho = 2 lambda R du_k + g_u_k +
//             Bd_k' pt_{k+1}, the adjoint's input stationarity residual.
//
// Lane k holds stage k throughout; d Bd_k / d psi is the product rule along
// stage_dynamics_vals in registers.  grad_x_lin is staged in the K table (dead
// after the roll-out) and leaves flat and coalesced; grad_mu is one wave sum.
#include "hmpc_vjp_kernel.h"

namespace hmpc {

namespace {

// The costate components at x_{k+1}, lane k, from the cost gradients c at x_{k+1}
// (components 3 4 5 | 9 10 11 | 0 1 | 6 7; 0 past the horizon): th = 3..5,
// w = 9..11 (costate_w's recursion), v = 6, 7 (v_i = c + v_{i+1} + dt p[0:2]_{i+1}).
// cn, sn: the yaw of stage k + 1.
__device__ __forceinline__ void costate_lin(const double (&c)[10], double cn, double sn, double dt, int lane,
                                            double (&th)[3], double (&w)[3], double (&v)[2]) {
  double tn[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    th[j] = suffix_scan(c[j], lane);
    tn[j] = th[j] - c[j];   // theta_{k+2}
  }
  w[0] = suffix_scan(c[3] + dt * (cn * tn[0] - sn * tn[1]), lane);
  w[1] = suffix_scan(c[4] + dt * (sn * tn[0] + cn * tn[1]), lane);
  w[2] = suffix_scan(fma(dt, tn[2], c[5]), lane);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const double pn = suffix_scan(c[6 + j], lane) - c[6 + j];
    v[j] = suffix_scan(fma(dt, pn, c[8 + j]), lane);
  }
}

// d/d psi of rows 9..11 of Bd_k, [3][6]: the product rule along
// stage_dynamics_vals (hmpc_model.h).  d = pf_k - x_lin[k][0:3].
template <int VAR>
__device__ __forceinline__ void dbw_dpsi(double cp, double sp, const double (&d)[3], const double (&Jinv)[9],
                                         const double (&rh)[3], double dt, double (&dbw)[18]) {
  const double Rz[3][3] = {{cp, sp, 0.0}, {-sp, cp, 0.0}, {0.0, 0.0, 1.0}};
  const double dR[3][3] = {{-sp, cp, 0.0}, {-cp, -sp, 0.0}, {0.0, 0.0, 0.0}};
  double rf[3], drf[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    rf[i] = rh[i] + (Rz[i][0] * d[0] + Rz[i][1] * d[1] + Rz[i][2] * d[2]);
    drf[i] = dR[i][0] * d[0] + dR[i][1] * d[1];
  }
  double T[3][3], dT[3][3], Jw[3][3], dJw[3][3], Bt[3][3], dBt[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      T[i][j] = Rz[i][0] * Jinv[j] + Rz[i][1] * Jinv[3 + j] + Rz[i][2] * Jinv[6 + j];
      dT[i][j] = dR[i][0] * Jinv[j] + dR[i][1] * Jinv[3 + j];
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {   // Jw = T Rz'
      Jw[i][j] = T[i][0] * Rz[j][0] + T[i][1] * Rz[j][1] + T[i][2] * Rz[j][2];
      dJw[i][j] = (dT[i][0] * Rz[j][0] + dT[i][1] * Rz[j][1] + dT[i][2] * Rz[j][2]) +
                  (T[i][0] * dR[j][0] + T[i][1] * dR[j][1]);
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {   // B[9:12, 3:6] = Jw Rz'
      Bt[i][j] = Jw[i][0] * Rz[j][0] + Jw[i][1] * Rz[j][1] + Jw[i][2] * Rz[j][2];
      dBt[i][j] = (dJw[i][0] * Rz[j][0] + dJw[i][1] * Rz[j][1] + dJw[i][2] * Rz[j][2]) +
                  (Jw[i][0] * dR[j][0] + Jw[i][1] * dR[j][1]);
    }
  double w[3], dw[3];
  if constexpr (VAR == 3) {   // hat(Rz' rf)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      w[i] = Rz[0][i] * rf[0] + Rz[1][i] * rf[1] + Rz[2][i] * rf[2];
      dw[i] = (dR[0][i] * rf[0] + dR[1][i] * rf[1]) + (Rz[0][i] * drf[0] + Rz[1][i] * drf[1] + Rz[2][i] * drf[2]);
    }
  } else {                    // hat(rf)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      w[i] = rf[i];
      dw[i] = drf[i];
    }
  }
  const double hw[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
  const double hd[3][3] = {{0.0, -dw[2], dw[1]}, {dw[2], 0.0, -dw[0]}, {-dw[1], dw[0], 0.0}};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double f = 0.0;
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        if constexpr (VAR == 3) f += dJw[i][l] * hw[l][j] + Jw[i][l] * hd[l][j];
        else f += dBt[i][l] * hw[l][j] + Bt[i][l] * hd[l][j];
      }
      dbw[6 * i + j] = f * dt;
      dbw[6 * i + 3 + j] = dBt[i][j] * dt;
    }
}

struct LinEpilogue {
  template <int VAR>
  static __device__ __forceinline__ void run(const VjpLinArgs& a, VjpShared& sh, int64_t b, double mu) {
    if (!a.grad_x_lin && !a.grad_mu) return;
    const int lane = threadIdx.x;
    const int N = a.N;
    const double dt = a.dt, dtm = a.dt / a.m, tol = a.act_tol;
    const bool st = lane < N;
    const int k = st ? lane : N - 1;
    // lane k: the cost gradients at x_{k+1} of the original problem and of the adjoint
    const double kap2 = st ? (k == N - 1 ? 2.0 * kTermQ : 2.0) : 0.0;
    const double sel = st ? 1.0 : 0.0;
    constexpr int kComp[10] = {3, 4, 5, 9, 10, 11, 0, 1, 6, 7};
    double c0[10], c1[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const int comp = kComp[j];
      const int64_t xi = (b * (N + 1) + k + 1) * 12 + comp;
      c0[j] = kap2 * kQ[comp] * (a.x[xi] - a.x_ref[(b * N + k) * 12 + comp]);
      c1[j] = fma(kap2 * kQ[comp], sh.gx[12 * (k + 1) + comp], a.g_x ? sel * a.g_x[xi] : 0.0);
    }
    const double* recn = sh.rec + kRec * (k + 1 < N ? k + 1 : k);   // the yaw of stage k + 1 (last lane: times 0)
    double th0[3], w0[3], v0[2], th1[3], w1[3], v1[2];
    costate_lin(c0, recn[R_CS], recn[R_CS + 1], dt, lane, th0, w0, v0);
    costate_lin(c1, recn[R_CS], recn[R_CS + 1], dt, lane, th1, w1, v1);

    const double* rec = sh.rec + kRec * k;
    const double cp = rec[R_CS], sp = rec[R_CS + 1];
    double u[6], du[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      u[c] = a.u[(b * N + k) * 6 + c];
      du[c] = sh.gu[6 * k + c];
    }
    if (a.grad_x_lin) {
      // position: -grad_pf[k], the first epilogue's two cross products
      double m0[3], m1[3], g[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        m0[j] = rec[R_BW + 3 + j] * w0[0] + rec[R_BW + 9 + j] * w0[1] + rec[R_BW + 15 + j] * w0[2];
        m1[j] = rec[R_BW + 3 + j] * w1[0] + rec[R_BW + 9 + j] * w1[1] + rec[R_BW + 15 + j] * w1[2];
      }
      if constexpr (VAR == 3) {
        const double r0[3] = {cp * m0[0] - sp * m0[1], sp * m0[0] + cp * m0[1], m0[2]};
        const double r1[3] = {cp * m1[0] - sp * m1[1], sp * m1[0] + cp * m1[1], m1[2]};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
          g[j] = (u[j1] * r1[j2] - u[j2] * r1[j1]) + (du[j1] * r0[j2] - du[j2] * r0[j1]);
        }
      } else {
        double t[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
          t[j] = (u[j1] * m1[j2] - u[j2] * m1[j1]) + (du[j1] * m0[j2] - du[j2] * m0[j1]);
        }
        g[0] = cp * t[0] - sp * t[1];
        g[1] = sp * t[0] + cp * t[1];
        g[2] = t[2];
      }
      // yaw.  Rows 9..11 of Bd_k: sum_rc dBw[r][c] (p_w[r] du[c] + pt_w[r] u*[c])
      double gy = 0.0;
      {
        const double* xl = a.x_lin + (b * (N + 1) + k) * 12;
        const double* pfp = a.pf + (b * N + k) * 3;
        const double d[3] = {pfp[0] - xl[0], pfp[1] - xl[1], pfp[2] - xl[2]};
        double dbw[18];
        dbw_dpsi<VAR>(cp, sp, d, a.Jinv, a.rh, dt, dbw);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 6; ++c) gy = fma(dbw[6 * r + c], fma(w0[r], du[c], w1[r] * u[c]), gy);
      }
      // d rz / d psi = [[-s, c], [-c, -s]] in the leading 2 x 2 block, 0 elsewhere
      if constexpr (VAR == 2) {   // Bd[6:9, 0:3] = dt/m rz': its derivative is the transpose of the block
        const double e00 = fma(v0[0], du[0], v1[0] * u[0]), e01 = fma(v0[0], du[1], v1[0] * u[1]);
        const double e10 = fma(v0[1], du[0], v1[1] * u[0]), e11 = fma(v0[1], du[1], v1[1] * u[1]);
        gy = fma(dtm, -sp * (e00 + e11) + cp * (e10 - e01), gy);
      }
      {   // Ad[3:6, 9:12] = dt rz on (dx_k, x*_k)[9:11]; dx_0 = 0 (row 0 of the table still holds g_x[0])
        const double o0 = a.x[(b * (N + 1) + k) * 12 + 9], o1 = a.x[(b * (N + 1) + k) * 12 + 10];
        const double q0 = k >= 1 ? sh.gx[12 * k + 9] : 0.0, q1 = k >= 1 ? sh.gx[12 * k + 10] : 0.0;
        const double e00 = fma(th0[0], q0, th1[0] * o0), e01 = fma(th0[0], q1, th1[0] * o1);
        const double e10 = fma(th0[1], q0, th1[1] * o0), e11 = fma(th0[1], q1, th1[1] * o1);
        gy = fma(dt, -sp * (e00 + e11) + cp * (e01 - e10), gy);
      }
      // stage: row k of [N+1][12] in the K table, row N zero; idle lanes fill a spare row
      double* row = sh.K + 12 * (st ? lane : 65);
#pragma unroll
      for (int c = 0; c < 12; ++c) row[c] = c < 3 ? -g[c] : (c == 5 ? gy : 0.0);
      if (lane < 12) sh.K[12 * N + lane] = 0.0;
    }
    if (a.grad_mu) {
      // the stage class and the held friction rows: pass 0's
      const StageClass sc =
          classify_stage<VAR>(u, a.x[(b * (N + 1) + k) * 12 + 2], a.C[b * N + k] != 0.0, mu, tol);
      const bool live = st && sc.reg && !both_signs<VAR>(sc);   // both signs: fz pinned at ~0, nothing moves with mu
      const double r2 = k == N - 1 ? 0.0 : 2.0 * kRdiag;
      const double* lam = a.lam + (b * N + k) * 11;
      double acc = 0.0;
#pragma unroll
      for (int ax = 0; ax < (VAR == 3 ? 2 : 1); ++ax) {
        // rho[ax] = 2 lambda R du + g_u + (Bd_k' pt_{k+1})[ax]
        double rho = fma(r2, du[ax], a.g_u ? a.g_u[(b * N + k) * 6 + ax] : 0.0);
        if constexpr (VAR == 3) rho = fma(dtm, v1[ax], rho);
        else rho += bv<VAR>(0, ax, dtm, cp, sp) * v1[0] + bv<VAR>(1, ax, dtm, cp, sp) * v1[1];
#pragma unroll
        for (int r = 0; r < 3; ++r) rho = fma(rec[R_BW + 6 * r + ax], w1[r], rho);
        const bool plus = ax == 0 ? sc.xp : sc.yp, held = ax == 0 ? (sc.a3 || sc.a4) : (sc.a5 || sc.a6);
        const double lm = plus ? lam[3 + 2 * ax] : lam[4 + 2 * ax];
        const double sg = plus ? 1.0 : -1.0;
        acc += (live && held) ? fma(sg * rho, u[2], -lm * du[2]) : 0.0;
      }
      const double total = wave_sum(acc);
      if (lane == 0) a.grad_mu[b] = total;
    }
    if (a.grad_x_lin) {
      __syncthreads();
#pragma unroll 1
      for (int i0 = 0; i0 < 12 * (N + 1); i0 += 64) {
        const int i = i0 + lane;
        if (i < 12 * (N + 1)) a.grad_x_lin[b * (N + 1) * 12 + i] = sh.K[i];
      }
    }
  }
};

}  // namespace

void launch_vjp_lin(int variant, const VjpLinArgs& a, hipStream_t s) {
  launch_vjp_kernel<VjpLinArgs, LinEpilogue>(variant, a, s);
}

}  // namespace hmpc
