// hmpc_plant_fb.hip -- the plant under the feedback law of hmpc_sens_batch's K_0
// (hmpc_plant_fb_batch).  No reference analogue: the reference
// holds u*_0 over a whole MPC period (src/robotrunner.py:104-113); here every
// low-level step s applies
//
//   x_s  = convert(X_s)
//   xbar = x_nom[0] + (s / stage_steps) (x_nom[1] - x_nom[0])     (HMPC_FB_INTERP)
//   d    = x_s - xbar,  d[5] wrapped to (-pi, pi]
//   u_s  = clip(U + K d)                                          (HMPC_FB_CLIP)
//   X_s+1 = rk4_normalized(X_s, u_s, pf_s)
//
// with the forward plant's own dynamics / convert_state (hmpc_plant_model.h).
// clip is the input set of build_qp (src/mpc_cvx_euler_3f.py:113-136, 2f).
//
// One lane per robot, 64-thread workgroups, as hmpc_plant.hip.  The 72 gains of
// a robot would not fit beside plant_kernel's live set, so the workgroup's
// 64 x 72 block goes through LDS once per launch: loaded flat (consecutive
// lanes read consecutive doubles of a row, rows K_bs apart), stored with a row
// stride of 73 doubles, read back per step as 72 lane-own ds_reads (73 is odd:
// the 32 lanes of a b64 access fall on 32 distinct bank pairs).
#include <hip/hip_runtime.h>

#include "hmpc_internal.h"
#include "hmpc_model.h"
#include "hmpc_plant_model.h"

namespace hmpc {

namespace {

constexpr int kGainRow = 73;        // LDS row stride, doubles
constexpr double kSatTol = 1e-8;    // act_tol's rule: moved by more than kSatTol (1 + |bound|)
constexpr double kTwoPi = 6.283185307179586;

// c = u clamped to [lo, hi]; moved |= the clamp changed u by more than the rule's tolerance at
// the bound it went to
__device__ __forceinline__ double clamp_count(double u, double lo, double hi, int& moved) {
  const double c = u < lo ? lo : (u > hi ? hi : u);
  const double bd = u < lo ? lo : hi;
  moved |= fabs(c - u) > kSatTol * (1.0 + fabs(bd)) ? 1 : 0;
  return c;
}

__global__ void __launch_bounds__(64) plant_fb_kernel(PlantFbArgs a) {
  __shared__ double Ks[64 * kGainRow];
  const int lane = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * 64;
  const int64_t b = b0 + lane;
  {   // the workgroup's gains: element i = lane + 64 t of the [rows][72] block
    // A fixed trip count without a branch, so that the loads of an unrolled batch are in
    // flight together (one at a time, 72 round trips to memory cost more than the 20 steps).
    // Past the batch's last robot the last robot's row is read again; its LDS row is not used.
    const int last = a.B - b0 < 64 ? (int)(a.B - b0) - 1 : 63;
    int r = 0, c = lane;   // lane < 72
#pragma unroll 18
    for (int t = 0; t < 72; ++t) {
      const int rr = r < last ? r : last;
      Ks[r * kGainRow + c] = a.K[(b0 + rr) * a.K_bs + c];
      c += 64;
      const int wrap = c >= 72 ? 1 : 0;
      c -= 72 * wrap;
      r += wrap;
    }
  }
  __syncthreads();
  if (b >= a.B) return;
  const double* Kl = Ks + lane * kGainRow;
  double X[13], U[6], x0[12], dx[12];
  for (int i = 0; i < 13; ++i) X[i] = a.X[b * 13 + i];
  for (int i = 0; i < 6; ++i) U[i] = a.U[b * a.U_bs + i];
  const bool interp = (a.flags & 2) != 0, clip = (a.flags & 1) != 0;
  for (int i = 0; i < 12; ++i) x0[i] = a.x_nom[b * a.xnom_bs + i];
  // (without HMPC_FB_INTERP row 0 again: dx = 0 with no branch around the loads, row 1 is not read)
  const int64_t row1 = b * a.xnom_bs + (interp ? 12 : 0);
  for (int i = 0; i < 12; ++i) dx[i] = a.x_nom[row1 + i] - x0[i];
  const bool stance = a.C0 ? a.C0[b * a.C0_bs] != 0.0 : true;
  const double mu = a.mu ? a.mu[b] : a.mu_default;
  const double h = a.dt;
  int sat = 0;
#pragma unroll 1
  for (int s = 0; s < a.n_steps; ++s) {
    const double* pf = a.pf + b * a.pf_bs + (int64_t)s * a.pf_ss;
    const double pfl[3] = {pf[0], pf[1], pf[2]};   // issued here: the law below hides the latency
    double u[6];
    {
      double x[12], d[12];
      convert_state(X, x);
      const double fr = interp ? (double)s / (double)a.stage_steps : 0.0;
      for (int i = 0; i < 12; ++i) d[i] = x[i] - (x0[i] + fr * dx[i]);
      d[5] -= kTwoPi * rint(d[5] / kTwoPi);
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 12; ++j) acc += Kl[12 * i + j] * d[j];
        u[i] = U[i] + acc;
      }
    }
    {   // the QP's input set, every choice a select; computed always, applied with the flag
      int mt = 0, ms = 0, mw = 0;   // a torque / a stance force / a swing force moved
      double c[6];
      for (int i = 3; i < 6; ++i) c[i] = clamp_count(u[i], -tau_lim(i), tau_lim(i), mt);
      const double fz = clamp_count(u[2], 0.0, kFzMax, ms);
      const double lim = mu * fz;   // friction after the fz clamp
      const double ylim = a.fy_zero ? 0.0 : lim;
      const double fx = clamp_count(u[0], -lim, lim, ms);
      const double fy = clamp_count(u[1], -ylim, ylim, ms);
      for (int i = 0; i < 3; ++i) mw |= fabs(u[i]) > kSatTol ? 1 : 0;   // swing: f = 0, bound 0
      c[0] = stance ? fx : 0.0;
      c[1] = stance ? fy : 0.0;
      c[2] = stance ? fz : 0.0;
      for (int i = 0; i < 6; ++i) u[i] = clip ? c[i] : u[i];
      sat += clip ? (mt | (stance ? ms : mw)) : 0;
    }
    if (a.U_hist)
      for (int i = 0; i < 6; ++i) a.U_hist[(b * a.n_steps + s) * 6 + i] = u[i];
    double f1[13], f2[13], f3[13], f4[13], Y[13];
    dynamics(a, X, u, pfl, f1);
    for (int i = 0; i < 13; ++i) Y[i] = X[i] + 0.5 * h * f1[i];
    dynamics(a, Y, u, pfl, f2);
    for (int i = 0; i < 13; ++i) Y[i] = X[i] + 0.5 * h * f2[i];
    dynamics(a, Y, u, pfl, f3);
    for (int i = 0; i < 13; ++i) Y[i] = X[i] + h * f3[i];
    dynamics(a, Y, u, pfl, f4);
    for (int i = 0; i < 13; ++i) X[i] = X[i] + (h / 6.0) * (f1[i] + 2.0 * f2[i] + 2.0 * f3[i] + f4[i]);
    const double nq = sqrt(X[3] * X[3] + X[4] * X[4] + X[5] * X[5] + X[6] * X[6]);
    for (int i = 3; i < 7; ++i) X[i] = X[i] / nq;
    if (a.X_hist)
      for (int i = 0; i < 13; ++i) a.X_hist[(b * a.n_steps + s) * 13 + i] = X[i];
  }
  for (int i = 0; i < 13; ++i) a.X[b * 13 + i] = X[i];
  if (a.x_out) {
    double x[12];
    convert_state(X, x);
    for (int i = 0; i < 12; ++i) a.x_out[b * 12 + i] = x[i];
  }
  if (a.sat) a.sat[b] = sat;
}

}  // namespace

void launch_plant_fb(const PlantFbArgs& a, hipStream_t s) {
  if (a.B <= 0) return;
  hipLaunchKernelGGL(plant_fb_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, s, a);
}

}  // namespace hmpc
