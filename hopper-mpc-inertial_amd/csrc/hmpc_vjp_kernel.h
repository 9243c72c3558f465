// hmpc_vjp_kernel.h -- the adjoint kernel behind hmpc_vjp_batch (hmpc_vjp.hip)
// and hmpc_vjp_lin_batch (hmpc_vjp_lin.hip, which adds an epilogue for x_lin and
// mu through the Epi hook): one body, one instantiation per translation unit.
// Device code only; internal linkage.
//
// Reverse-mode gradients of the solve: for cotangents g_u, g_x
// of a scalar loss L(u*, x*),
//   grad_theta = (d u*/d theta)' g_u + (d x*/d theta)' g_x,  theta = x_in, x_ref, pf,
// at the active set of a given primal point (x, u) of the reference's QP
// (3f :96-153, 2f :96-151) -- the solution map hmpc_sens.hip differentiates in
// forward mode.  One adjoint solve: d = (dx, du) minimises the QP's quadratic
// form plus g_x . dx + g_u . du over the linearised dynamics from dx_0 = 0 with
// every active row held.  A post-processing kernel like
// hmpc_sens.hip: it touches no solve kernel.
//
// One wavefront per instance, grid-stride over B, fp64.  Lane = load:
//
//   pass 0  lane k < N takes stage k (records to LDS as in hmpc_sens.hip); the
//           cotangents go to two LDS tables; the active z rows are balloted
//           onto lanes 0..q-1.
//   pass 1  the projected Riccati recursion of hmpc_sens.hip: K_k, C_k to LDS.
//   pass 2  (q > 0) one backward sweep for every load at once: lane j < q
//           carries the unit load of its z row, lane q (the base lane) the
//           affine load s_k = g_x_k + Ad' s_{k+1} + K_k' h_k, h_k = g_u_k +
//           Bd_k' s_{k+1}.  y = C^-1 Pi h goes to an LDS tile; each lane
//           accumulates its row of the Gram matrix W and its product with the
//           base lane's y: the right-hand side of W nu = -Y' y0.  Elimination
//           row per lane, one right-hand side.
//   pass 3  every lane alike: the backward sweep with the combined load (base +
//           nu on the z rows) leaves v_k = -Pi C'^-1 y_k in LDS and grad_x_in = s_0;
//           then the roll-out dx_{k+1} = Ad dx_k + Bd (K_k dx_k + v_k) with lane =
//           state component (ad_lane, row sums by DPP); dx and du go to LDS.
//   epilogue  lane = stage: the costate components that multiply d Bd / d pf
//           are suffix sums over the horizon -- of the original problem (from
//           2 kappa Q (x - r)) and of the adjoint (from g_x + 2 kappa Q dx) --
//           by a DPP suffix scan; grad_pf[k] is two cross products, grad_x_ref
//           a scaled copy of dx.
//
//   Epi::run  a further lane = stage epilogue on the tables the passes leave (dx
//           in gx rows >= 1, du in gu, the adjoint's z loads in nu, the records);
//           K, cf and tile are dead by then and free for staging.
//
// No MFMA: the blocks are 12 x 6 and smaller, as everywhere in this path.
#pragma once
#include <hip/hip_runtime.h>

#include "hmpc_internal.h"
#include "hmpc_model.h"
#include "hmpc_sens_common.h"

namespace hmpc {

namespace {

// Sum over each row of 16 lanes, left in every lane of the row
__device__ __forceinline__ double row_sum(double x) {
  x += dpp<kDppXor1>(x);
  x += dpp<kDppXor2>(x);
  x += dpp<kDppHalfMirror>(x);
  x += dpp<kDppMirror>(x);
  return x;
}

// Inclusive suffix sum over the wave, sum of x over lanes >= this one: four DPP
// row shifts (lanes past the row's end read 0), then the totals of the later
// rows, which sit in their first lanes
__device__ __forceinline__ double suffix_scan(double x, int lane) {
  x += row_shift<1>(x);
  x += row_shift<2>(x);
  x += row_shift<4>(x);
  x += row_shift<8>(x);
  const double t1 = rdlane(x, 16), t2 = rdlane(x, 32), t3 = rdlane(x, 48);
  const int row = lane >> 4;
  return x + (row == 0 ? t1 + (t2 + t3) : (row == 1 ? t2 + t3 : (row == 2 ? t3 : 0.0)));
}

// c = the cost gradient at x_i, components 3..5 | 9..11, in lane i - 1 (0 past
// the horizon): the costate's components 9..11 at x_i.  theta_i = c[0:3] +
// theta_{i+1} and w_i = c[3:6] + w_{i+1} + dt Rz_i' theta_{i+1}; nothing else of
// the costate reaches them (Ad' feeds 9..11 from 3..5 alone).  cn, sn: the yaw
// of stage i.
__device__ __forceinline__ void costate_w(const double (&c)[6], double cn, double sn, double dt, int lane,
                                          double (&w)[3]) {
  double th[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) th[j] = suffix_scan(c[j], lane) - c[j];   // theta_{i+1}
  w[0] = suffix_scan(c[3] + dt * (cn * th[0] - sn * th[1]), lane);
  w[1] = suffix_scan(c[4] + dt * (sn * th[0] + cn * th[1]), lane);
  w[2] = suffix_scan(fma(dt, th[2], c[5]), lane);
}

// The backward step of the loaded sweeps: h = Bd_k' s + w gu, y = C_k^-1 Pi_k h,
// then s <- Ad_k' s + K_k' h.  The caller adds the stage's state load.
template <int VAR>
__device__ __forceinline__ void load_step(const double* rec, const double* cf, const double* Kk, const double* gu,
                                          double w, double dt, double dtm, double (&s)[12], double (&y)[6]) {
  double h[6];
  bdt_times<VAR>(s, rec[R_CS], rec[R_CS + 1], rec + R_BW, dtm, h);
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    h[c] = fma(w, gu[c], h[c]);
    y[c] = h[c];
  }
  pi_apply(rec + R_PI, y);
  chol_fwd(cf, y);
  adt_times(s, dt, rec[R_CS], rec[R_CS + 1]);
#pragma unroll
  for (int r = 0; r < 12; ++r) {
    double acc = s[r];
#pragma unroll
    for (int c = 0; c < 6; ++c) acc = fma(Kk[12 * c + r], h[c], acc);
    s[r] = acc;
  }
}

struct VjpShared : RiccatiShared {
  double gx[66 * 12];        // g_x[k] until the roll-out, which leaves dx_k in row k >= 1
  double gu[65 * 6];         // g_u[k], then v_k (pass 3), then du_k (roll-out)
  double nu[65];             // load on stage k's z row
  int zidx[65];
};

struct NoEpilogue {
  template <int VAR, class Args>
  static __device__ __forceinline__ void run(const Args&, VjpShared&, int64_t, double) {}
};

template <int VAR, class Args, class Epi>
__global__ void __launch_bounds__(64) vjp_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) VjpShared sh;
  const int lane = threadIdx.x;
  const int N = a.N;
  const double dt = a.dt, dtm = a.dt / a.m;
  const bool st = lane < N;          // this lane owns a stage
  const int k = st ? lane : N - 1;   // clamped: loads stay in bounds
  const bool colane = lane < 12;     // this lane owns a column of P / a state component
  const int col = colane ? lane : 0;

  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    const double mu = a.mu ? a.mu[b] : a.mu_default;
    // ------------------------------------------------------------ pass 0
    int nq;
    const int zstage = stage_records<VAR>(a, sh, sh.zidx, b, mu, [&] {
      sh.nu[lane] = 0.0;
      // the cotangents, flat and coalesced (a NULL one is 0); lanes past the end fill a spare slot
#pragma unroll 1
      for (int i0 = 0; i0 < 12 * (N + 1); i0 += 64) {
        const int i = i0 + lane;
        const bool ok = i < 12 * (N + 1);
        sh.gx[ok ? i : 65 * 12] = a.g_x ? a.g_x[b * (N + 1) * 12 + (ok ? i : 0)] : 0.0;
      }
#pragma unroll 1
      for (int i0 = 0; i0 < 6 * N; i0 += 64) {
        const int i = i0 + lane;
        const bool ok = i < 6 * N;
        sh.gu[ok ? i : 64 * 6] = a.g_u ? a.g_u[b * N * 6 + (ok ? i : 0)] : 0.0;
      }
    }, nq);   // (nq <= N - 1 <= 63: the base lane nq exists)
    // ------------------------------------------------------------ pass 1
    riccati_pass<VAR>(sh, N, dt, dtm);
    double P[12];

    // ------------------------------------------------------------ pass 2
    // The loaded LQR's optimal value is -1/2 |y0 + Y nu|^2 summed over the stages
    // (y0: the base lane's y, Y: the unit loads'): its maximum over nu is
    // W nu = -Y'y0, W = Y'Y -- the base column of the (q+1) x (q+1) Gram matrix.
    int singular = 0;
    if (nq > 0) {
      double G[64], y[6];
#pragma unroll
      for (int j = 0; j < 64; ++j) G[j] = 0.0;
      const double base = lane == nq ? 1.0 : 0.0;
#pragma unroll
      for (int r = 0; r < 12; ++r) P[r] = base * sh.gx[12 * N + r];
      double D0 = 0.0, rhs[1] = {0.0};
#pragma unroll 1
      for (int kk = N - 1; kk >= 0; --kk) {
        load_step<VAR>(sh.rec + kRec * kk, sh.cf + kCst * kk, sh.K + kKst * kk, sh.gu + 6 * kk, base, dt, dtm, P, y);
#pragma unroll
        for (int r = 0; r < 12; ++r) P[r] = fma(base, sh.gx[12 * kk + r], P[r]);
        P[2] += zstage == kk ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          sh.tile[6 * lane + c] = y[c];
          D0 = fma(y[c], y[c], D0);
        }
        __syncthreads();
        gram_row(G, y, sh.tile, nq);   // own row of W
        {
          const double* t = sh.tile + 6 * nq;   // the base lane's y
#pragma unroll
          for (int c = 0; c < 6; ++c) rhs[0] = fma(y[c], t[c], rhs[0]);
        }
        __syncthreads();
      }
      // A pivot below the floor: the row is dependent given the pinned inputs
      // (the stage-1 row always is) -- flag it, drop it, its nu stays 0.
      rhs[0] = -rhs[0];
      solve_rows<1, 0>(G, rhs, D0, nq, lane, singular);
      sh.nu[zstage >= 0 ? zstage : 64] = rhs[0];   // slot 64: spare
      __syncthreads();
    }

    // ------------------------------------------------------------ pass 3
    // backward with the combined load, every lane the same stream and values
    {
      double y[6];
#pragma unroll
      for (int r = 0; r < 12; ++r) P[r] = sh.gx[12 * N + r];
#pragma unroll 1
      for (int kk = N - 1; kk >= 0; --kk) {
        const double* rec = sh.rec + kRec * kk;
        const double* cf = sh.cf + kCst * kk;
        load_step<VAR>(rec, cf, sh.K + kKst * kk, sh.gu + 6 * kk, 1.0, dt, dtm, P, y);
#pragma unroll
        for (int r = 0; r < 12; ++r) P[r] += sh.gx[12 * kk + r];
        P[2] += sh.nu[kk];
        // v_k = -Pi C'^-1 y over g_u[k], which this stage has consumed
        chol_bwd(cf, y);
        pi_apply(rec + R_PI, y);
#pragma unroll
        for (int c = 0; c < 6; ++c) sh.gu[6 * kk + c] = -y[c];
      }
      // the costate at stage 0 (dx_0 = 0: no P_0 dx_0 term) is the multiplier of x_0 = x_in
      double g0 = 0.0;
#pragma unroll
      for (int r = 0; r < 12; ++r) g0 = lane == r ? P[r] : g0;
      if (a.grad_x_in && colane) a.grad_x_in[b * 12 + lane] = g0;
    }
    __syncthreads();
    // roll-out, lane r < 12 = component r of dx (lanes >= 12 stay 0)
    {
      const bool wl = lane >= 9 && lane < 12, vl = lane >= 6 && lane < 9;
      const int rw = wl ? lane - 9 : 0, rv = lane - 6;
      const double isw = wl ? 1.0 : 0.0, isv = vl ? dtm : 0.0;
      double xr = 0.0;
#pragma unroll 1
      for (int kk = 0; kk < N; ++kk) {
        const double* rec = sh.rec + kRec * kk;
        const double* Kk = sh.K + kKst * kk;
        const double cp = rec[R_CS], sp = rec[R_CS + 1];
        double du[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) du[c] = row_sum(Kk[12 * c + col] * xr) + sh.gu[6 * kk + c];
        {
          double* dst = sh.gu + 6 * (lane == 0 ? kk : 64);   // the other lanes: the spare row
#pragma unroll
          for (int c = 0; c < 6; ++c) dst[c] = du[c];
        }
        // row `lane` of Bd_k (rows 6..8: bv(); rows 9..11: the record's bw)
        double brow[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) brow[c] = isw * rec[R_BW + 6 * rw + c];
        if constexpr (VAR == 3) {
#pragma unroll
          for (int c = 0; c < 3; ++c) brow[c] += rv == c ? isv : 0.0;
        } else {   // Rz' dt/m
          brow[0] += isv * (rv == 0 ? cp : (rv == 1 ? sp : 0.0));
          brow[1] += isv * (rv == 0 ? -sp : (rv == 1 ? cp : 0.0));
          brow[2] += rv == 2 ? isv : 0.0;
        }
        double acc = ad_lane(xr, dt, cp, sp, lane);
#pragma unroll
        for (int c = 0; c < 6; ++c) acc = fma(brow[c], du[c], acc);
        xr = acc;
        sh.gx[colane ? 12 * (kk + 1) + lane : 65 * 12] = xr;
      }
    }
    __syncthreads();

    // ------------------------------------------------------------ epilogue, lane = stage
    if (a.grad_x_ref) {   // grad_x_ref[k] = -2 kappa_k Q dx_{k+1}, flat and coalesced
#pragma unroll 1
      for (int i0 = 0; i0 < 12 * N; i0 += 64) {
        const int i = i0 + lane;
        const bool ok = i < 12 * N;
        const int ic = ok ? i : 0;
        const int kx = ic / 12, r = ic - 12 * kx;
        const double val = -2.0 * (kx == N - 1 ? kTermQ : 1.0) * qdiag(r) * sh.gx[12 + ic];
        if (ok) a.grad_x_ref[b * N * 12 + i] = val;
      }
    }
    if (a.grad_pf) {
      // lane k: the cost gradients at x_{k+1} of the original problem and of the adjoint
      const double kap2 = st ? (k == N - 1 ? 2.0 * kTermQ : 2.0) : 0.0;
      const double sel = st ? 1.0 : 0.0;
      double c0[6], c1[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const int comp = j < 3 ? 3 + j : 6 + j;
        const int64_t xi = (b * (N + 1) + k + 1) * 12 + comp;
        c0[j] = kap2 * kQ[comp] * (a.x[xi] - a.x_ref[(b * N + k) * 12 + comp]);
        c1[j] = fma(kap2 * kQ[comp], sh.gx[12 * (k + 1) + comp], a.g_x ? sel * a.g_x[xi] : 0.0);
      }
      const double* recn = sh.rec + kRec * (k + 1 < N ? k + 1 : k);   // the yaw of stage k + 1 (last lane: times 0)
      double w0[3], w1[3];
      costate_w(c0, recn[R_CS], recn[R_CS + 1], dt, lane, w0);
      costate_w(c1, recn[R_CS], recn[R_CS + 1], dt, lane, w1);
      // d Bd_k / d pf_k[j] sits in rows 9..11, columns 0..2: 3f dt Jw hat(e_j), 2f dt Jw Rz' hat(Rz e_j).
      // With m = (dt Jw Rz')' w (the record's torque block):
      //   3f  grad_pf[k] = f*_k x Rz' m(adjoint) + df_k x Rz' m(original)
      //   2f  grad_pf[k] = Rz' (f*_k x m(adjoint) + df_k x m(original))
      const double* rec = sh.rec + kRec * k;
      const double cp = rec[R_CS], sp = rec[R_CS + 1];
      double m0[3], m1[3], f[3], df[3], g[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        m0[j] = rec[R_BW + 3 + j] * w0[0] + rec[R_BW + 9 + j] * w0[1] + rec[R_BW + 15 + j] * w0[2];
        m1[j] = rec[R_BW + 3 + j] * w1[0] + rec[R_BW + 9 + j] * w1[1] + rec[R_BW + 15 + j] * w1[2];
        f[j] = a.u[(b * N + k) * 6 + j];
        df[j] = sh.gu[6 * k + j];
      }
      if constexpr (VAR == 3) {
        const double r0[3] = {cp * m0[0] - sp * m0[1], sp * m0[0] + cp * m0[1], m0[2]};
        const double r1[3] = {cp * m1[0] - sp * m1[1], sp * m1[0] + cp * m1[1], m1[2]};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
          g[j] = (f[j1] * r1[j2] - f[j2] * r1[j1]) + (df[j1] * r0[j2] - df[j2] * r0[j1]);
        }
      } else {
        double t[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
          t[j] = (f[j1] * m1[j2] - f[j2] * m1[j1]) + (df[j1] * m0[j2] - df[j2] * m0[j1]);
        }
        g[0] = cp * t[0] - sp * t[1];
        g[1] = sp * t[0] + cp * t[1];
        g[2] = t[2];
      }
      if (st) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a.grad_pf[(b * N + k) * 3 + j] = g[j];
      }
    }
    Epi::template run<VAR>(a, sh, b, mu);
    if (a.flags && lane == 0) a.flags[b] = singular;   // HMPC_VJP_SINGULAR
  }
}

// one wave per workgroup, grid-stride; the LDS block allows two workgroups
// per CU, so 1024 workgroups are two rounds of the chip
template <class Args, class Epi>
void launch_vjp_kernel(int variant, const Args& a, hipStream_t s) {
  if (a.B <= 0) return;
  const unsigned grid = (unsigned)(a.B < 1024 ? a.B : 1024);
  if (variant == 2) hipLaunchKernelGGL((vjp_kernel<2, Args, Epi>), dim3(grid), dim3(64), 0, s, a);
  else hipLaunchKernelGGL((vjp_kernel<3, Args, Epi>), dim3(grid), dim3(64), 0, s, a);
}

}  // namespace

}  // namespace hmpc
