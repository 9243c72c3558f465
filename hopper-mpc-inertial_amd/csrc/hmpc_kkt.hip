// hmpc_kkt.hip -- Lagrange multipliers and a KKT certificate for a given
// primal point (x, u) of the reference's QP (3f :96-153, 2f :96-151): what
// problem.solve() leaves in cvxpy's dual_value / OSQP's y
// (src/mpc_cvx_euler_3f.py:156-157).  A post-processing kernel: it touches no
// solve kernel and never forms the condensed Hessian.
//
// One wavefront per instance, grid-stride over B, fp64.  The work split is
// lane = right-hand side of the costate recursion, not lane = variable:
//
//   pass 0  lane k < N takes stage k: dynamics, slacks, stage class and active
//           mask, the projector onto the input directions whose gradient must
//           vanish, the primal residuals; stage records go to LDS.  The
//           active z rows are balloted and assigned to lanes 1..q.
//   pass 1  every lane steps k = N-1 .. 0 together: lane 0 carries the base
//           costate p0, lane j the unit response of its z row (12 registers
//           each); the stage's Ad, Bd and projector are wave-uniform LDS reads.
//           Each lane writes its projected input gradient to an LDS tile and
//           accumulates its own row of the Gram matrix from broadcast reads.
//   solve   the q x q normal equations, row per lane, reciprocal pivots.
//   pass 2  the same recursion once more: g_k = g0_k - sum_j nu_j m_j,k by six
//           wave sums per stage; lane k keeps stage k and recovers its
//           multipliers and its share of the certificate.
//
// No MFMA: the blocks are 12 x 6 and smaller.
#include <hip/hip_runtime.h>

#include "hmpc_internal.h"
#include "hmpc_model.h"
#include "hmpc_sens_common.h"

namespace hmpc {

namespace {

// the stage record (longer than the one sens / vjp share: it carries the cost gradients)
constexpr int kKktRec = 48;   // doubles per stage record
constexpr int KR_CS = 0;    // cos, sin of the linearisation yaw
constexpr int KR_BW = 2;    // rows 9..11 of Bd_k, [3][6]
constexpr int KR_CX = 20;   // 2 kappa_k Q (x_{k+1} - r_k)
constexpr int KR_DU = 32;   // 2 lambda_k R (u_k - ubar_k)
constexpr int KR_PI = 38;   // force projector, symmetric: xx xy xz yy yz zz
constexpr int KR_TM = 44;   // torque mask (1: the component must vanish), contiguous with KR_PI

// stage classes
constexpr int CL_SWING = 0, CL_APEX = 1, CL_REG = 2;

__device__ __forceinline__ double wave_max(double x) {
  x = fmax(x, dpp<kDppXor1>(x));
  x = fmax(x, dpp<kDppXor2>(x));
  x = fmax(x, dpp<kDppHalfMirror>(x));
  x = fmax(x, dpp<kDppMirror>(x));
  return fmax(fmax(rdlane(x, 0), rdlane(x, 16)), fmax(rdlane(x, 32), rdlane(x, 48)));
}

// One backward step shared by pass 1 and pass 2: m = Bd_k' P + base du_k, then
// (k > 0) P <- Ad_k' P + base cx_{k-1} + [this lane's z row is stage k] e_2.
template <int VAR>
__device__ __forceinline__ void back_step(int k, const double* recs, double dt, double dtm, double base,
                                          int zstage, double (&P)[12], double (&m)[6]) {
  const double* rec = recs + kKktRec * k;
  bdt_times<VAR>(P, rec[KR_CS], rec[KR_CS + 1], rec + KR_BW, dtm, m);
#pragma unroll
  for (int c = 0; c < 6; ++c) m[c] = fma(base, rec[KR_DU + c], m[c]);
  if (k > 0) {
    adt_times(P, dt, rec[KR_CS], rec[KR_CS + 1]);
    const double* prev = rec - kKktRec;
#pragma unroll
    for (int r = 0; r < 12; ++r) P[r] = fma(base, prev[KR_CX + r], P[r]);
    P[2] += (zstage == k) ? 1.0 : 0.0;
  }
}

struct KktShared {
  double rec[65 * kKktRec];   // one spare record / row / slot for the idle lanes
  double tile[64 * 6];
  double nu[65];
  double lam[65 * 11];
  int zidx[64];
};

template <int VAR>
__global__ void __launch_bounds__(64) kkt_kernel(KktArgs a) {
  __shared__ __attribute__((aligned(16))) KktShared sh;
  const int lane = threadIdx.x;
  const int N = a.N;
  const double dt = a.dt, dtm = a.dt / a.m;
  const bool st = lane < N;          // this lane owns a stage
  const int k = st ? lane : N - 1;   // clamped: loads stay in bounds
  const double base = lane == 0 ? 1.0 : 0.0;

  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    const double mu = a.mu ? a.mu[b] : a.mu_default;
    const double tol = a.act_tol;
    // ------------------------------------------------------------ pass 0
    const double* xk = a.x + (b * (N + 1) + k) * 12;
    const double* xl = a.x_lin + (b * (N + 1) + k) * 12;
    const double* xr = a.x_ref + (b * N + k) * 12;
    const double* pfp = a.pf + (b * N + k) * 3;
    double u[6], x0[12], x1[12], cs[2], bw[18];
#pragma unroll
    for (int c = 0; c < 6; ++c) u[c] = a.u[(b * N + k) * 6 + c];
#pragma unroll
    for (int r = 0; r < 12; ++r) { x0[r] = xk[r]; x1[r] = xk[12 + r]; }
    const bool stance = a.C[b * N + k] != 0.0;
    const bool last = k == N - 1;
    const double kap = last ? kTermQ : 1.0, lamk = last ? 0.0 : 1.0;
    {
      const double p[3] = {xl[0], xl[1], xl[2]};
      const double pfk[3] = {pfp[0], pfp[1], pfp[2]};
      stage_dynamics_vals<VAR, double>(0, xl[5], p, pfk, a.Jinv, a.rh, dt, cs, bw);
    }
    double* rec = sh.rec + kKktRec * (st ? lane : 64);   // idle lanes write a spare record
    double peq = 0.0, pin = 0.0, qmax = 0.0;
    // u_ref of this stage's cost (aliased: the last stage's)
    const bool uref_on = a.uref_aliased ? (a.C[b * N + N - 1] != 0.0) : stance;
    const double uref2 = uref_on ? 2.0 * a.m * a.g : 0.0;
    double cx[12], du[6];
#pragma unroll
    for (int r = 0; r < 12; ++r) {
      const double w = 2.0 * kap * kQ[r];
      cx[r] = w * (x1[r] - xr[r]);
      qmax = fmax(qmax, fabs(w * xr[r]));
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) du[c] = 2.0 * lamk * kRdiag * (u[c] - (c == 2 ? uref2 : 0.0));
    qmax = fmax(qmax, fabs(2.0 * lamk * kRdiag * uref2));
    // dynamics residual x_{k+1} - Ad x_k - Bd u_k - Gd
    {
      double y[12];
#pragma unroll
      for (int r = 0; r < 12; ++r) y[r] = x0[r];
      ad_times(y, dt, cs[0], cs[1]);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double acc = y[6 + r];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc = fma(bv<VAR>(r, c, dtm, cs[0], cs[1]), u[c], acc);
        y[6 + r] = acc;
        acc = y[9 + r];
#pragma unroll
        for (int c = 0; c < 6; ++c) acc = fma(bw[6 * r + c], u[c], acc);
        y[9 + r] = acc;
      }
      y[8] -= a.g * dt;
#pragma unroll
      for (int r = 0; r < 12; ++r) peq = fmax(peq, fabs(x1[r] - y[r]));
#pragma unroll
      for (int r = 0; r < 12; ++r) peq = fmax(peq, lane == 0 ? fabs(x0[r] - a.x_in[b * 12 + r]) : 0.0);
    }
    // the active set by the shared rule; the slacks stay for the certificate
    const StageClass sc = classify_stage<VAR>(u, x0[2], stance, mu, tol);
    // z row of this stage (nu_0 = 0: that row sits on the fixed x_0)
    const double zslack = sc.zslack;
    pin = fmax(pin, -zslack);
    const bool zact = st && lane >= 1 && sc.zact;
    // torques
    double tsl[3];   // slack of the active (or nearer) torque bound
    double tm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double lim = tau_lim(3 + c);
      const double sup = lim - u[3 + c], slo = u[3 + c] + lim;
      pin = fmax(pin, fmax(-sup, -slo));
      tsl[c] = (sc.tmask & (A_TUP << c)) ? sup : slo;
      tm[c] = torque_free(sc, c);
    }
    // forces, branch-free (selects)
    if (VAR == 2) peq = fmax(peq, fabs(u[1]));
    peq = fmax(peq, stance ? 0.0 : fmax(fabs(u[0]), fmax(fabs(u[1]), fabs(u[2]))));
    const double szl = u[2], szu = kFzMax - u[2];
    const bool apex = sc.apex, reg = sc.reg;
    const int cls = !stance ? CL_SWING : (apex ? CL_APEX : CL_REG);
    double fsl[5];   // slacks of slots 3..6 and of the fz bound in play (0 on swing stages)
    fsl[0] = stance ? sc.fs[0] : 0.0;
    fsl[1] = stance ? sc.fs[1] : 0.0;
    fsl[2] = (stance && VAR == 3) ? sc.fs[2] : 0.0;
    fsl[3] = (stance && VAR == 3) ? sc.fs[3] : 0.0;
    fsl[4] = stance ? (apex ? szl : szu) : 0.0;
    pin = fmax(pin, stance ? fmax(fmax(-fsl[0], -fsl[1]), fmax(-szl, -szu)) : 0.0);
    pin = fmax(pin, fmax(-fsl[2], -fsl[3]));
    const int mask = sc.tmask | (reg ? sc.fm : 0);   // the rows that receive a multiplier
    double pi[6];
    force_projector<VAR>(mask, mu, pi);
    // swing and apex stages: every force component is free
#pragma unroll
    for (int i = 0; i < 6; ++i) pi[i] = reg ? pi[i] : 0.0;
    __syncthreads();   // the previous instance's reads of the shared block are done
    rec[KR_CS] = cs[0];
    rec[KR_CS + 1] = cs[1];
#pragma unroll
    for (int i = 0; i < 18; ++i) rec[KR_BW + i] = bw[i];
#pragma unroll
    for (int r = 0; r < 12; ++r) rec[KR_CX + r] = cx[r];
#pragma unroll
    for (int c = 0; c < 6; ++c) rec[KR_DU + c] = du[c];
#pragma unroll
    for (int i = 0; i < 6; ++i) rec[KR_PI + i] = pi[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) rec[KR_TM + c] = tm[c];
    sh.nu[lane] = 0.0;
    peq = wave_max(st ? peq : 0.0);
    pin = wave_max(st ? pin : 0.0);
    qmax = wave_max(st ? qmax : 0.0);
    // active z rows -> lanes 1..nq, in stage order
    const unsigned long long zb = __ballot(zact);
    const int nq = __popcll(zb);
    sh.zidx[zact ? 1 + __popcll(zb & ((1ull << lane) - 1ull)) : 0] = lane;   // slot 0: spare
    __syncthreads();
    const int zi = sh.zidx[lane];   // (unassigned lanes read a stale slot: selected away)
    const int zstage = (lane >= 1 && lane <= nq) ? zi : -1;

    // ------------------------------------------------------------ pass 1
    double P[12], m[6];
    double G[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) G[j] = 0.0;
    double D0 = 0.0;
    if (nq > 0) {
      {
        const double* lastrec = sh.rec + kKktRec * (N - 1);
#pragma unroll
        for (int r = 0; r < 12; ++r) P[r] = base * lastrec[KR_CX + r];
      }
#pragma unroll 1
      for (int kk = N - 1; kk >= 0; --kk) {
        back_step<VAR>(kk, sh.rec, dt, dtm, base, zstage, P, m);
        pi_apply(sh.rec + kKktRec * kk + KR_PI, m);   // the components that must vanish
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          sh.tile[6 * lane + c] = m[c];
          D0 = fma(m[c], m[c], D0);
        }
        __syncthreads();
        gram_row(G, m, sh.tile, nq + 1);   // own Gram row, columns 0..nq
        __syncthreads();
      }
    }
    // ------------------------------------------------ factor and solve
    // rows 1..nq of G, right-hand side in column 0 (G[i][0] = m~_i . g~0);
    // elimination with reciprocal pivots, row per lane, the pivot row by
    // readlane.  A pivot below the floor: the row is dependent given the
    // pinned inputs -- flag it and leave its nu at 0.
    int singular = 0;
    double rhs[1] = {G[0]};
    solve_rows<1, 1>(G, rhs, D0, nq, lane, singular);
    const double nu_own = zstage >= 0 ? rhs[0] : 0.0;
    sh.nu[zstage >= 0 ? zstage : 64] = nu_own;   // slot 64: spare
    __syncthreads();
    const double nuk = sh.nu[lane];   // nu of this lane's stage

    // ------------------------------------------------------------ pass 2
    double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    {
      const double coef = lane == 0 ? 1.0 : -nu_own;
      const double* lastrec = sh.rec + kKktRec * (N - 1);
#pragma unroll
      for (int r = 0; r < 12; ++r) P[r] = base * lastrec[KR_CX + r];
#pragma unroll 1
      for (int kk = N - 1; kk >= 0; --kk) {
        back_step<VAR>(kk, sh.rec, dt, dtm, base, zstage, P, m);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const double s = wave_sum(coef * m[c]);
          g[c] = lane == kk ? s : g[c];
        }
      }
    }
    // lane = stage again: local multipliers and the certificate's maxima
    double stat = 0.0, dneg = fmax(0.0, -nuk), comp = fabs(nuk * zslack);
    double lam[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) lam[i] = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double gt = g[3 + c];
      const bool up = (mask & (A_TUP << c)) != 0, lo = (mask & (A_TLO << c)) != 0;
      lam[c] = (up || lo) ? -gt : 0.0;
      dneg = fmax(dneg, up ? gt : (lo ? -gt : 0.0));
      comp = fmax(comp, (up || lo) ? fabs(gt * tsl[c]) : 0.0);
      stat = fmax(stat, (up || lo) ? 0.0 : fabs(gt));
    }
    const double w[3] = {-g[0], -g[1], -g[2]};
    {
      // Every class is evaluated and selected per slot (no divergent region).
      // Apex (stance, fz = 0): the five rows are dependent, the force
      // components are free and the dual condition is membership of the normal
      // cone, w_z <= -mu (|w_x| + |w_y|); the minimal nonnegative split.
      // Regular stance: the <= 3 independent active rows by the stage's QR.
      const bool swing = cls == CL_SWING, apex = cls == CL_APEX, reg = cls == CL_REG;
      const double ylo = -w[2] - mu * (fabs(w[0]) + (VAR == 3 ? fabs(w[1]) : 0.0));
      StageQr s;
      stage_qr<VAR>(mask, mu, s);
      double t[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = s.q[i][0] * w[0] + s.q[i][1] * w[1] + s.q[i][2] * w[2];
      const double y2 = t[2] * s.ri[2];
      const double y1 = (t[1] - s.r12 * y2) * s.ri[1];
      const double y0 = (t[0] - s.r01 * y1 - s.r02 * y2) * s.ri[0];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        stat = fmax(stat, reg ? fabs(w[c] - (t[0] * s.q[0][c] + t[1] * s.q[1][c] + t[2] * s.q[2][c])) : 0.0);
      lam[3] = apex ? fmax(w[0], 0.0) : ((mask & A_FXP) ? y0 : 0.0);
      lam[4] = apex ? fmax(-w[0], 0.0) : ((mask & A_FXM) ? y0 : 0.0);
      if (VAR == 3) {
        lam[5] = apex ? fmax(w[1], 0.0) : ((mask & A_FYP) ? y1 : 0.0);
        lam[6] = apex ? fmax(-w[1], 0.0) : ((mask & A_FYM) ? y1 : 0.0);
      }
      lam[7] = apex ? -ylo : ((mask & A_FZU) ? y2 : 0.0);
      lam[8] = swing ? w[0] : 0.0;
      lam[9] = swing ? w[1] : (VAR == 2 ? (apex ? w[1] : y1) : 0.0);
      lam[10] = swing ? w[2] : 0.0;
      // friction multipliers are >= 0; fz: <= 0 at the lower bound (apex), >= 0 at f_max
      dneg = fmax(dneg, fmax(fmax(-lam[3], -lam[4]), fmax(-lam[5], -lam[6])));
      dneg = fmax(dneg, apex ? lam[7] : -lam[7]);
#pragma unroll
      for (int i = 0; i < 5; ++i) comp = fmax(comp, fabs(lam[3 + i] * fsl[i]));
    }
    stat = wave_max(st ? stat : 0.0);
    dneg = wave_max(st ? dneg : 0.0);
    comp = wave_max(st ? comp : 0.0);
    // ------------------------------------------------------------ stores
    if (a.lam) {
#pragma unroll
      for (int i = 0; i < 11; ++i) sh.lam[11 * (st ? lane : 64) + i] = lam[i];
      __syncthreads();
      for (int t = lane; t < 11 * N; t += 64) a.lam[b * 11 * N + t] = sh.lam[t];
    }
    if (a.nu && st) a.nu[b * N + lane] = nuk;
    if (lane < 5) {
      const double v = lane == 0 ? peq : lane == 1 ? fmax(pin, 0.0) : lane == 2 ? dneg
                     : lane == 3 ? stat / (1.0 + qmax) : comp;
      a.cert[b * 5 + lane] = v;
    }
    if (a.flags && lane == 0) a.flags[b] = singular;
  }
}

}  // namespace

void launch_kkt(int variant, const KktArgs& a, hipStream_t s) {
  if (a.B <= 0) return;
  // one wave per workgroup, grid-stride: enough workgroups to fill the chip
  const unsigned grid = (unsigned)(a.B < 4096 ? a.B : 4096);
  if (variant == 2) hipLaunchKernelGGL(kkt_kernel<2>, dim3(grid), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(kkt_kernel<3>, dim3(grid), dim3(64), 0, s, a);
}

}  // namespace hmpc
