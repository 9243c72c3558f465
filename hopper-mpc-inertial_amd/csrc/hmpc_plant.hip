// hmpc_plant.hip -- the Runner's plant on the device:
// batched RK4 integration of the SE(3) rigid-body dynamics between MPC
// solves, and the SE(3) -> Euler state conversion that feeds the next solve.
//
//   dynamics_ct     src/robotrunner.py:126-152   (hmpc_plant_model.h)
//   rk4_normalized  src/robotrunner.py:154-164
//   convert         src/robotrunner.py:19-28 (quat2euler: src/utils.py:54-62,
//                   transforms3d 'rzyx' = quat2mat + mat2euler; hmpc_plant_model.h)
//
// One thread per robot: the state (13 doubles), the held input and the
// constants live in registers; a launch integrates `n_steps` low-level steps
// (one MPC period = mpc_factor steps in the Runner) so the state never leaves
// the chip between them.  This is ~1e4 flops per robot per period: latency
// of a small launch, not throughput, is what it costs next to the solve.
#include <hip/hip_runtime.h>

#include "hmpc_internal.h"
#include "hmpc_plant_model.h"

namespace hmpc {

namespace {

__global__ void __launch_bounds__(64) plant_kernel(PlantArgs a) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  double X[13], U[6];
  for (int i = 0; i < 13; ++i) X[i] = a.X[b * 13 + i];
  for (int i = 0; i < 6; ++i) U[i] = a.U[b * a.U_bs + i];
  const double h = a.dt;
#pragma unroll 1
  for (int s = 0; s < a.n_steps; ++s) {
    const double* pf = a.pf + b * a.pf_bs + (int64_t)s * a.pf_ss;
    double pfl[3] = {pf[0], pf[1], pf[2]};
    double f1[13], f2[13], f3[13], f4[13], Y[13];
    dynamics(a, X, U, pfl, f1);
    for (int i = 0; i < 13; ++i) Y[i] = X[i] + 0.5 * h * f1[i];
    dynamics(a, Y, U, pfl, f2);
    for (int i = 0; i < 13; ++i) Y[i] = X[i] + 0.5 * h * f2[i];
    dynamics(a, Y, U, pfl, f3);
    for (int i = 0; i < 13; ++i) Y[i] = X[i] + h * f3[i];
    dynamics(a, Y, U, pfl, f4);
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
}

__global__ void __launch_bounds__(64) convert_kernel(int64_t B, const double* X, double* x) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double Xl[13], xl[12];
  for (int i = 0; i < 13; ++i) Xl[i] = X[b * 13 + i];
  convert_state(Xl, xl);
  for (int i = 0; i < 12; ++i) x[b * 12 + i] = xl[i];
}

}  // namespace

void launch_plant(const PlantArgs& a, hipStream_t s) {
  if (a.B <= 0) return;
  hipLaunchKernelGGL(plant_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, s, a);
}

void launch_convert(int64_t B, const double* X, double* x, hipStream_t s) {
  if (B <= 0) return;
  hipLaunchKernelGGL(convert_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, B, X, x);
}

}  // namespace hmpc
