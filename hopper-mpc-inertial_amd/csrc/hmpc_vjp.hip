// hmpc_vjp.hip -- hmpc_vjp_batch: the adjoint kernel of hmpc_vjp_kernel.h with
// its own epilogue alone (grad_x_in, grad_x_ref, grad_pf).
#include "hmpc_vjp_kernel.h"

namespace hmpc {

void launch_vjp(int variant, const VjpArgs& a, hipStream_t s) {
  launch_vjp_kernel<VjpArgs, NoEpilogue>(variant, a, s);
}

}  // namespace hmpc
