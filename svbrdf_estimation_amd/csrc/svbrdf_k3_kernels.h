// svbrdf_k3_kernels.h -- the two K3 kernel templates and their launcher, for the three units that instantiate them.
//
// The order the compiler leaves the instructions in moves these VALU-bound kernels by up to 20 % at an identical
// instruction mix, and no single set of LLVM scheduler options suits every kernel (measured grid: csrc/Makefile,
// profiles/r02_sched_grid.txt).  So the variants of K3 are spread over three units, each built with its own set:
//   svbrdf_main.hip              the forward-only variants <GRAD=0, ...>                  (bottom-up post-RA scheduler)
//   svbrdf_k3_adjoint.hip        forward+adjoint RenderingLoss <GRAD, L1=0, HEAD=0>
//   svbrdf_k3_adjoint_extra.hip  forward+adjoint MixedLoss / head-fused (L1 or HEAD set)
//                                (both: no post-RA scheduler, iterative-minreg strategy, round 1's register-assignment
//                                options; separate units so that each can take its own set again when the optimum moves)
// That makes this the ONE header of csrc/ that holds __global__: templates only.  It holds no instantiation and no entry
// point; a unit gets the kernels it names through launch_k3<G, WHICH> and no others.
#ifndef SVBRDF_K3_KERNELS_H
#define SVBRDF_K3_KERNELS_H
#include "svbrdf_device.h"

namespace {

#define SVBRDF_K3_ATTRS __launch_bounds__(kLossThreads) __attribute__((amdgpu_waves_per_eu(SVBRDF_K3_MIN_WAVES, 8)))

// scene table in device memory (any B*S)
template <bool WITH_GRAD, bool WITH_L1, bool HEAD>
__global__ SVBRDF_K3_ATTRS void k_rendering_loss(const float *__restrict__ input, const float *__restrict__ target,
                                                 const float *__restrict__ scenes, const float *__restrict__ xrow,
                                                 float eps, float inv_count, double loss_scale, float fixed_scale,
                                                 L1Params l1, float *__restrict__ grad_input,
                                                 unsigned long long *__restrict__ ws, float *__restrict__ loss_out,
                                                 int S, int H, int W)
{
    rendering_loss_body<WITH_GRAD, WITH_L1, HEAD>(input, target, scenes, xrow, eps, inv_count, loss_scale, fixed_scale,
                                                  l1, grad_input, ws, loss_out, S, H, W);
}

// Scene table passed BY VALUE in the kernel-argument block (B*S <= SVBRDF_HOST_SCENES_MAX_ROWS).
// The table is drawn on the host for every call (losses.py:35), so it has to cross to the device
// once per call either way; as a kernel argument it rides in the dispatch packet's own argument
// buffer: no device allocation, no hipMemcpyAsync command in front of the kernel, no pinned
// staging slot and no event to guard its reuse.  Measured on config 2: the memcpy route costs
// ~24 us of host time per call and makes the step host-bound at ~60 us; this route leaves one
// dispatch per step and the loop GPU-bound at the kernel's own ~53 us.  The body reads the rows
// with the same wave-uniform scalar loads, from the kernarg segment instead of a global buffer.
// Capacity: 288 rows (10,368 bytes) -- configs[3] (16 x 9 rows) and config 5 at batch 8 (8 x 32) fit; the
// runtime takes argument blocks of 32 KB and more on gfx950 (tools: a by-value struct of 32,000 bytes launches and
// reads back correctly), and marshalling 10 KB costs the launch ~0.2 us.
// `table` is the FIRST argument, i.e. it sits at offset 0 of the kernarg segment, and is read through
// the segment pointer: taking the address of the by-value parameter itself makes the compiler
// copy the whole block into scratch in the adjoint variants (seen in the resource report).
template <bool WITH_GRAD, bool WITH_L1, bool HEAD>
__global__ SVBRDF_K3_ATTRS void k_rendering_loss_inl([[maybe_unused]] const SceneBlock table,
                                                     const float *__restrict__ input, const float *__restrict__ target,
                                                     const float *__restrict__ xrow, float eps, float inv_count,
                                                     double loss_scale, float fixed_scale, L1Params l1,
                                                     float *__restrict__ grad_input, unsigned long long *__restrict__ ws,
                                                     float *__restrict__ loss_out, int S, int H, int W)
{
    const float *__restrict__ rows = (const float *)__builtin_amdgcn_kernarg_segment_ptr();
    rendering_loss_body<WITH_GRAD, WITH_L1, HEAD, true>(input, target, rows, xrow, eps, inv_count, loss_scale,
                                                           fixed_scale, l1, grad_input, ws, loss_out, S, H, W);
}

// launches one K3 variant; `rows` = the host scene table for the by-value kernels (NULL: device table `scenes`).
// WHICH selects the variants the call instantiates: 0 = <G, L1=0, HEAD=0> only, 1 = the other three.
template <bool G, int WHICH>
void launch_k3(bool with_l1, bool head, const float *rows, dim3 grid, size_t lds_bytes, hipStream_t st,
               const float *input, const float *target, const float *scenes, const float *xrow, float eps,
               float inv_count, double loss_scale, float fixed_scale, L1Params l1, float *grad_input,
               unsigned long long *ws, float *loss_out, int B, int S, int H, int W)
{
    SceneBlock block_arg;      // only the first B*S rows are ever read
    if (rows) std::memcpy(block_arg.v, rows, (size_t)B * S * 9 * sizeof(float));
#define SVBRDF_LAUNCH_K3_AS(KERNEL, KERNEL_INL, THREADS)                                                        \
    do {                                                                                                        \
        if (rows)                                                                                               \
            hipLaunchKernelGGL(KERNEL_INL, grid, dim3(THREADS), lds_bytes, st, block_arg, input, target, xrow,  \
                               eps, inv_count, loss_scale, fixed_scale, l1, grad_input, ws, loss_out, S, H, W); \
        else                                                                                                    \
            hipLaunchKernelGGL(KERNEL, grid, dim3(THREADS), lds_bytes, st, input, target, scenes, xrow, eps,    \
                               inv_count, loss_scale, fixed_scale, l1, grad_input, ws, loss_out, S, H, W);      \
    } while (0)
#define SVBRDF_LAUNCH_K3(L, HD)                                                                                 \
    SVBRDF_LAUNCH_K3_AS((k_rendering_loss<G, L, HD>), (k_rendering_loss_inl<G, L, HD>), kLossThreads)
    static_assert(WHICH == 0 || WHICH == 1, "launch_k3: WHICH is 0 or 1");
    if constexpr (WHICH == 1) {
        if (head) { if (with_l1) SVBRDF_LAUNCH_K3(true, true); else SVBRDF_LAUNCH_K3(false, true); }
        else if (with_l1) SVBRDF_LAUNCH_K3(true, false);
    } else {
        if (!head && !with_l1) SVBRDF_LAUNCH_K3(false, false);
    }
#undef SVBRDF_LAUNCH_K3
#undef SVBRDF_LAUNCH_K3_AS
}

}  // namespace

// the forward+adjoint variants live in their own translation units (see the top of this file)
#define SVBRDF_K3_ADJOINT_ARGS                                                                                        \
    int with_l1, int head, const float *rows, unsigned gx, unsigned gy, size_t lds_bytes, void *stream,                 \
        const float *input, const float *target, const float *scenes, const float *xrow, float eps, float inv_count,   \
        double loss_scale, float fixed_scale, float l1_sum_scale, float l1_grad_scale, float l1_eps, float *grad_input, \
        unsigned long long *ws, float *loss_out, int B, int S, int H, int W
extern "C" __attribute__((visibility("hidden"))) void svbrdf_internal_launch_k3_adjoint_plain(SVBRDF_K3_ADJOINT_ARGS);
extern "C" __attribute__((visibility("hidden"))) void svbrdf_internal_launch_k3_adjoint_extra(SVBRDF_K3_ADJOINT_ARGS);

#endif  // SVBRDF_K3_KERNELS_H
