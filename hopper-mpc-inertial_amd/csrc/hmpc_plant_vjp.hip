// hmpc_plant_vjp.hip -- hmpc_plant_vjp_batch: the adjoint of one hmpc_plant_batch
// call (n_steps of rk4_normalized, src/robotrunner.py:154-164, then convert,
// :19-28) and, with n_steps = 0, of hmpc_convert_batch alone.
//
// One lane per robot, as the forward: the plant is irregular 3-vector algebra
// (each of dp, dq, dv, dw has its own formula), so lanes that shared a robot
// would each run every formula under selects.
//
// Checkpoints come from the forward (X_hist: the state at the start of step s is
// X0 for s = 0, X_hist[:, s-1] otherwise; the load for step s-1 is issued before
// step s's arithmetic), the stages are recomputed: going backwards, a step
//   1. recomputes Y2 = X_s + h/2 f1, Y3, Y4 and the un-normalised next state
//      with the forward's own `dynamics` (Y1 = X_s; f1..f4 are not kept),
//   2. pulls the cotangent through q = qt/|qt|:  g_qt = (g_q - q (q.g_q)) / |qt|,
//   3. runs the RK4 adjoint, four hand-written `dynamics_vjp` calls:
//        a4 = h/6 abar,           g4 = vjp(Y4; a4)
//        a3 = h/3 abar + h g4,    g3 = vjp(Y3; a3)
//        a2 = h/3 abar + h/2 g3,  g2 = vjp(Y2; a2)
//        a1 = h/6 abar + h/2 g2,  g1 = vjp(Y1; a1)
//        abar += g1 + g2 + g3 + g4
//      whose U parts accumulate into grad_U and whose pf parts sum into grad_pf[s],
//   4. adds g_X_hist[:, s-1].
// The adjoint of convert runs first, on the recomputed final state.
#include <hip/hip_runtime.h>

#include "hmpc_internal.h"
#include "hmpc_plant_model.h"

namespace hmpc {

namespace {

// gq += sum_ij G[i][j] dR[i][j]/dq.  Every entry of R = Rot(q) is a quadratic form
// in q (R is not normalised: it scales with |q|^2), so this is one contraction.
__device__ __forceinline__ void rot_vjp(const double* q, const double (&G)[3][3], double* gq) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double a = G[2][1] - G[1][2], b = G[0][2] - G[2][0], c = G[1][0] - G[0][1];   // w's partners
  const double sxy = G[0][1] + G[1][0], sxz = G[0][2] + G[2][0], syz = G[1][2] + G[2][1];
  gq[0] += 2.0 * (w * (G[0][0] + G[1][1] + G[2][2]) + x * a + y * b + z * c);
  gq[1] += 2.0 * (x * (G[0][0] - G[1][1] - G[2][2]) + w * a + y * sxy + z * sxz);
  gq[2] += 2.0 * (y * (G[1][1] - G[0][0] - G[2][2]) + w * b + x * sxy + z * syz);
  gq[3] += 2.0 * (z * (G[2][2] - G[0][0] - G[1][1]) + w * c + x * sxz + y * syz);
}

// (gY, gU +=, gpf +=) = (df/dX, df/dU, df/dpf)' ac at (Y, U, pf): the adjoint of
// `dynamics`.  With gh = J^-T a_w:  g_tau = gh, g_r = fb x gh, g_fb = gh x r; the
// gyroscopic term gives g_w -= Jw x gh + J'(gh x w); dv gives g_ftb = a_v / m,
// g_w -= v x a_v, g_v -= a_v x w.  Each R' and R product adds a rank-one term to
// the adjoint G of R and sends R (or R') times the cotangent to its operand.
__device__ __forceinline__ void dynamics_vjp(const PlantArgs& a, const double* Y, const double* U,
                                             const double* pf, const double* ac, double* gY,
                                             double* gU, double* gpf) {
  const double* p = Y;
  const double* q = Y + 3;
  const double* v = Y + 7;
  const double* w = Y + 10;
  const double* a_p = ac;
  const double* a_q = ac + 3;
  const double* a_v = ac + 7;
  const double* a_w = ac + 10;
  const Rot R(q);
  // the forward's operands of the torque arm
  const double fw[3] = {U[0], U[1], U[2] - a.g * a.m};
  double dpf[3], r[3], fb[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) dpf[i] = pf[i] - p[i];
  R.apply_t(dpf, r);
#pragma unroll
  for (int i = 0; i < 3; ++i) r[i] += a.rh[i];
  R.apply_t(U, fb);
  // dw = J^-1 (tau + r x fb - w x J w)
  double gh[3], g_r[3], g_fb[3], jw[3], c1[3], c2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) gh[i] = a.Jinv[i] * a_w[0] + a.Jinv[3 + i] * a_w[1] + a.Jinv[6 + i] * a_w[2];
  cross(fb, gh, g_r);
  cross(gh, r, g_fb);
#pragma unroll
  for (int i = 0; i < 3; ++i) jw[i] = a.J[3 * i] * w[0] + a.J[3 * i + 1] * w[1] + a.J[3 * i + 2] * w[2];
  cross(jw, gh, c1);
  cross(gh, w, c2);
  double g_w[3], g_v[3], va[3], aw[3], g_f[3];
  cross(v, a_v, va);
  cross(a_v, w, aw);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    g_w[i] = -(c1[i] + a.J[i] * c2[0] + a.J[3 + i] * c2[1] + a.J[6 + i] * c2[2]) - va[i];
    g_f[i] = a_v[i] / a.m;   // g_ftb
  }
  // dq = 0.5 L(q) H w, bilinear in (q, w)
  double g_q[4];
  g_w[0] += 0.5 * (-q[1] * a_q[0] + q[0] * a_q[1] + q[3] * a_q[2] - q[2] * a_q[3]);
  g_w[1] += 0.5 * (-q[2] * a_q[0] - q[3] * a_q[1] + q[0] * a_q[2] + q[1] * a_q[3]);
  g_w[2] += 0.5 * (-q[3] * a_q[0] + q[2] * a_q[1] - q[1] * a_q[2] + q[0] * a_q[3]);
  g_q[0] = 0.5 * (w[0] * a_q[1] + w[1] * a_q[2] + w[2] * a_q[3]);
  g_q[1] = 0.5 * (-w[0] * a_q[0] - w[2] * a_q[2] + w[1] * a_q[3]);
  g_q[2] = 0.5 * (-w[1] * a_q[0] + w[2] * a_q[1] - w[0] * a_q[3]);
  g_q[3] = 0.5 * (-w[2] * a_q[0] - w[1] * a_q[1] + w[0] * a_q[2]);
  // dp = R v;  ftb = R' fw, r = R' (pf - p) + rh, fb = R' F
  R.apply_t(a_p, g_v);
  double G[3][3], gF[3], gP[3], sum[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    g_v[i] -= aw[i];
    sum[i] = g_f[i] + g_fb[i];
  }
  R.apply(sum, gF);
  R.apply(g_r, gP);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      G[i][j] = a_p[i] * v[j] + fw[i] * g_f[j] + dpf[i] * g_r[j] + U[i] * g_fb[j];
  rot_vjp(q, G, g_q);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    gU[i] += gF[i];
    gU[3 + i] += gh[i];
    gpf[i] += gP[i];
    gY[i] = -gP[i];
    gY[7 + i] = g_v[i];
    gY[10 + i] = g_w[i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) gY[3 + i] = g_q[i];
}

// gX += (d convert / dX)' gx at X, along the branch convert_state takes.  The
// Euler angles read M = Rot(q) / |q|^2 (transforms3d's quat2mat), so their
// cotangent GM joins the adjoint of R scaled by 1 / |q|^2, and |q|^2 itself
// receives -<GM, M> / |q|^2.  At the gimbal branch (cy <= 4 eps) the map is not
// differentiable: x[5] contributes 0 and cy is held constant; the rest of the
// result is undefined there.
__device__ __forceinline__ void convert_vjp(const double* X, const double* gx, double* gX) {
  const double* q = X + 3;
  const double* v = X + 7;
  const double* w = X + 10;
  const Rot R(q);
  double G[3][3], t[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) G[i][j] = gx[6 + i] * v[j] + gx[9 + i] * w[j];
  R.apply_t(gx + 6, t);
#pragma unroll
  for (int i = 0; i < 3; ++i) { gX[i] += gx[i]; gX[7 + i] += t[i]; }
  R.apply_t(gx + 9, t);
#pragma unroll
  for (int i = 0; i < 3; ++i) gX[10 + i] += t[i];
  const double nq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (nq >= 2.220446049250313e-16) {   // else M = I: the angles do not depend on q
    const double inv = 1.0 / nq;
    const double M00 = R.r[0][0] * inv, M10 = R.r[1][0] * inv, M20 = R.r[2][0] * inv;
    const double cy2 = M00 * M00 + M10 * M10, cy = sqrt(cy2);
    double GM[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    const double dp = gx[4] / (M20 * M20 + cy2);   // pitch = atan2(-M20, cy)
    GM[2][0] = -dp * cy;
    if (cy > 4.0 * 2.220446049250313e-16) {
      const double M21 = R.r[2][1] * inv, M22 = R.r[2][2] * inv;
      const double dr = gx[3] / (M21 * M21 + M22 * M22);   // roll = atan2(M21, M22)
      GM[2][1] = dr * M22;
      GM[2][2] = -dr * M21;
      const double dy = gx[5] / cy2, dc = dp * M20 / cy;   // yaw = atan2(M10, M00); cy
      GM[0][0] = dc * M00 - dy * M10;
      GM[1][0] = dc * M10 + dy * M00;
    } else {
      const double M11 = R.r[1][1] * inv, M12 = R.r[1][2] * inv;
      const double dr = gx[3] / (M11 * M11 + M12 * M12);   // roll = atan2(-M12, M11)
      GM[1][2] = -dr * M11;
      GM[1][1] = dr * M12;
    }
    double dot = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        dot += GM[i][j] * R.r[i][j];
        G[i][j] += GM[i][j] * inv;
      }
    const double gn = -2.0 * dot * inv * inv;   // d/dq of |q|^2 is 2 q
#pragma unroll
    for (int i = 0; i < 4; ++i) gX[3 + i] += gn * q[i];
  }
  rot_vjp(q, G, gX + 3);
}

// Not capped at two waves per SIMD: at 256 registers the stage points, the
// cotangents and the hoisted constants spill to scratch.
__global__ void __launch_bounds__(64) plant_vjp_kernel(PlantVjpArgs a) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  const int n = a.n_steps;
  const double h = a.dt;
  double U[6], gU[6], abar[13], X[13];
  for (int i = 0; i < 6; ++i) { U[i] = a.U[b * a.U_bs + i]; gU[i] = 0.0; }
  for (int i = 0; i < 13; ++i) abar[i] = a.g_X ? a.g_X[b * 13 + i] : 0.0;
  if (n > 0 && a.g_X_hist)
    for (int i = 0; i < 13; ++i) abar[i] += a.g_X_hist[(b * n + (n - 1)) * 13 + i];
  {
    const double* src = n >= 2 ? a.Xh + (b * n + (n - 2)) * 13 : a.X0 + b * 13;   // the start of the last step
    for (int i = 0; i < 13; ++i) X[i] = src[i];
  }
  if (n == 0 && a.g_x_out) convert_vjp(X, a.g_x_out + b * 12, abar);
#pragma unroll 1
  for (int s = n - 1; s >= 0; --s) {
    double Xp[13];   // the start of step s - 1: in flight under this step's arithmetic
    if (s >= 1) {
      const double* src = s >= 2 ? a.Xh + (b * n + (s - 2)) * 13 : a.X0 + b * 13;
      for (int i = 0; i < 13; ++i) Xp[i] = src[i];
    }
    const double* pf = a.pf + b * a.pf_bs + (int64_t)s * a.pf_ss;
    const double pfl[3] = {pf[0], pf[1], pf[2]};
    // the forward's stages again (its order of operations), f1..f4 summed on the way
    double Y2[13], Y3[13], Y4[13], Xn[13], f[13];
    dynamics(a, X, U, pfl, f);
    for (int i = 0; i < 13; ++i) { Y2[i] = X[i] + 0.5 * h * f[i]; Xn[i] = f[i]; }
    dynamics(a, Y2, U, pfl, f);
    for (int i = 0; i < 13; ++i) { Y3[i] = X[i] + 0.5 * h * f[i]; Xn[i] += 2.0 * f[i]; }
    dynamics(a, Y3, U, pfl, f);
    for (int i = 0; i < 13; ++i) { Y4[i] = X[i] + h * f[i]; Xn[i] += 2.0 * f[i]; }
    dynamics(a, Y4, U, pfl, f);
    for (int i = 0; i < 13; ++i) Xn[i] = X[i] + (h / 6.0) * (Xn[i] + f[i]);
    const double nq = sqrt(Xn[3] * Xn[3] + Xn[4] * Xn[4] + Xn[5] * Xn[5] + Xn[6] * Xn[6]);
    for (int i = 3; i < 7; ++i) Xn[i] = Xn[i] / nq;
    if (s == n - 1 && a.g_x_out) convert_vjp(Xn, a.g_x_out + b * 12, abar);
    // q = qt / |qt|
    const double qg = Xn[3] * abar[3] + Xn[4] * abar[4] + Xn[5] * abar[5] + Xn[6] * abar[6];
    for (int i = 3; i < 7; ++i) abar[i] = (abar[i] - Xn[i] * qg) / nq;
    // the RK4 adjoint
    double ac[13], g[13], gs[13], gpf[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < 13; ++i) ac[i] = (h / 6.0) * abar[i];
    dynamics_vjp(a, Y4, U, pfl, ac, g, gU, gpf);
    for (int i = 0; i < 13; ++i) { gs[i] = g[i]; ac[i] = (h / 3.0) * abar[i] + h * g[i]; }
    dynamics_vjp(a, Y3, U, pfl, ac, g, gU, gpf);
    for (int i = 0; i < 13; ++i) { gs[i] += g[i]; ac[i] = (h / 3.0) * abar[i] + 0.5 * h * g[i]; }
    dynamics_vjp(a, Y2, U, pfl, ac, g, gU, gpf);
    for (int i = 0; i < 13; ++i) { gs[i] += g[i]; ac[i] = (h / 6.0) * abar[i] + 0.5 * h * g[i]; }
    dynamics_vjp(a, X, U, pfl, ac, g, gU, gpf);
    for (int i = 0; i < 13; ++i) abar[i] += gs[i] + g[i];
    if (a.grad_pf)
      for (int i = 0; i < 3; ++i) a.grad_pf[(b * n + s) * 3 + i] = gpf[i];
    if (s >= 1) {
      if (a.g_X_hist)
        for (int i = 0; i < 13; ++i) abar[i] += a.g_X_hist[(b * n + (s - 1)) * 13 + i];
      for (int i = 0; i < 13; ++i) X[i] = Xp[i];
    }
  }
  if (a.grad_X0)
    for (int i = 0; i < 13; ++i) a.grad_X0[b * 13 + i] = abar[i];
  if (a.grad_U)
    for (int i = 0; i < 6; ++i) a.grad_U[b * 6 + i] = gU[i];
}

}  // namespace

void launch_plant_vjp(const PlantVjpArgs& a, hipStream_t s) {
  if (a.B <= 0) return;
  hipLaunchKernelGGL(plant_vjp_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, s, a);
}

}  // namespace hmpc
