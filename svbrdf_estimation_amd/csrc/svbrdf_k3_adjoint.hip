// The forward+adjoint RenderingLoss kernels k_rendering_loss{,_inl}<GRAD, L1=0, HEAD=0> -- the headline kernel of a
// training step -- and their launcher, in a unit of their own for its scheduler set (csrc/Makefile: SCHED_ADJOINT).
#include "svbrdf_k3_kernels.h"

void svbrdf_internal_launch_k3_adjoint_plain(SVBRDF_K3_ADJOINT_ARGS)
{
    launch_k3<true, 0>(with_l1 != 0, head != 0, rows, dim3(gx, gy, 1), lds_bytes,
                       static_cast<hipStream_t>(stream), input, target, scenes, xrow, eps, inv_count, loss_scale, fixed_scale,
                       L1Params{l1_sum_scale, l1_grad_scale, l1_eps}, grad_input, ws, loss_out, B, S, H, W);
}
