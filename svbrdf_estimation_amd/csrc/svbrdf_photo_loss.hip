// svbrdf_photo_loss.hip -- translation unit of libsvbrdf_hip.so: the fused PHOTO loss (ABI version 8).
//
//   L = mean_{b,s,c,i,j} | log(render(scene[b,s], input[b]) + eps) - log(photo[b,s] + eps) |
//
// K3 (svbrdf_device.h) compares the renderings of two sets of maps; this kernel compares the renderings of ONE set
// of maps with given photographs -- the inverse-rendering use of the engine, where ground-truth maps do not exist.  Per
// pixel it loads the 12 input planes once, loops the S scenes in registers, shades the input with K3's own primitives
// (dots / lobe / shade_loss / shade_bwd: tied-roughness fast path and three-lobe path), takes the target side of every
// term from three loads instead of a second shading, accumulates the analytic gradient in registers, stores the 12
// gradient planes once and reduces the loss through K3's fixed-point finalise (loss_arrive: same 65-word scratch, left
// zeroed for the next call).  HBM traffic (12 + 3 S + 12) * 4 bytes per pixel, one launch.
//
// The device functions and the launchers' checks are in svbrdf_photo_loss_device.h, which the other photo units include
// too; this file holds the sixteen kernels, their launcher and their entry points.  A unit of its own so that K3's
// machine code cannot move (tests/test_counter_replay_guard.py hashes it) and so that this kernel takes its own scheduler
// option set (csrc/Makefile: SCHED_PHOTO).  Numerics contract as K3: -ffp-contract=off, the coords -> NH path exact.
#include "svbrdf_photo_loss_device.h"

namespace {

// scene table in device memory (any B*S)
template <bool WITH_GRAD>
__global__ SVBRDF_PHOTO_LOSS_ATTRS void k_photo_loss(const float *__restrict__ input, const float *__restrict__ photos,
                                                     const float *__restrict__ scenes, const float *__restrict__ xrow,
                                                     float eps, float inv_count, double loss_scale, float fixed_scale,
                                                     float *__restrict__ grad_input, unsigned long long *__restrict__ ws,
                                                     float *__restrict__ loss_out, int S, int H, int W)
{
    photo_loss_body<WITH_GRAD, false>(input, photos, scenes, xrow, eps, inv_count, loss_scale, fixed_scale, grad_input,
                                      ws, loss_out, S, H, W);
}

// scene table BY VALUE in the kernel-argument block, first argument, read through the segment pointer
// (k_rendering_loss_inl has the reasons)
template <bool WITH_GRAD>
__global__ SVBRDF_PHOTO_LOSS_ATTRS void k_photo_loss_inl([[maybe_unused]] const SceneBlock table,
                                                         const float *__restrict__ input, const float *__restrict__ photos,
                                                         const float *__restrict__ xrow, float eps, float inv_count,
                                                         double loss_scale, float fixed_scale,
                                                         float *__restrict__ grad_input, unsigned long long *__restrict__ ws,
                                                         float *__restrict__ loss_out, int S, int H, int W)
{
    const float *__restrict__ rows = (const float *)__builtin_amdgcn_kernarg_segment_ptr();
    photo_loss_body<WITH_GRAD, true>(input, photos, rows, xrow, eps, inv_count, loss_scale, fixed_scale, grad_input, ws,
                                     loss_out, S, H, W);
}

// the head variants (svbrdf_head_photo_loss_fwd_bwd*): `encoded9` [B,9,H,W] in, its gradient out
template <bool WITH_GRAD>
__global__ SVBRDF_PHOTO_LOSS_ATTRS void k_head_photo(const float *__restrict__ encoded9, const float *__restrict__ photos,
                                                     const float *__restrict__ scenes, const float *__restrict__ xrow,
                                                     float eps, float inv_count, double loss_scale, float fixed_scale,
                                                     float *__restrict__ grad_encoded9, unsigned long long *__restrict__ ws,
                                                     float *__restrict__ loss_out, int S, int H, int W)
{
    photo_loss_body<WITH_GRAD, false, true>(encoded9, photos, scenes, xrow, eps, inv_count, loss_scale, fixed_scale,
                                            grad_encoded9, ws, loss_out, S, H, W);
}

template <bool WITH_GRAD>
__global__ SVBRDF_PHOTO_LOSS_ATTRS void k_head_photo_inl([[maybe_unused]] const SceneBlock table,
                                                         const float *__restrict__ encoded9, const float *__restrict__ photos,
                                                         const float *__restrict__ xrow, float eps, float inv_count,
                                                         double loss_scale, float fixed_scale,
                                                         float *__restrict__ grad_encoded9, unsigned long long *__restrict__ ws,
                                                         float *__restrict__ loss_out, int S, int H, int W)
{
    const float *__restrict__ rows = (const float *)__builtin_amdgcn_kernarg_segment_ptr();
    photo_loss_body<WITH_GRAD, true, true>(encoded9, photos, rows, xrow, eps, inv_count, loss_scale, fixed_scale,
                                           grad_encoded9, ws, loss_out, S, H, W);
}

// The WEIGHTED kernels (svbrdf_*photo_loss_weighted_fwd_bwd*): the same four shapes with `weights` and its plane count.
// (Names that hold neither "k_photo_loss" nor "k_head_photo": the unweighted kernels are counted by those.)
#define SVBRDF_WPHOTO_KERNEL(NAME, EARLY, HEAD)                                                                       \
    template <bool WITH_GRAD>                                                                                         \
    __global__ SVBRDF_PHOTO_LOSS_ATTRS void NAME(const float *__restrict__ input, const float *__restrict__ photos,   \
                                                 const float *__restrict__ weights, int weight_planes,                \
                                                 const float *__restrict__ scenes, const float *__restrict__ xrow,    \
                                                 float eps, float inv_count, double loss_scale, float fixed_scale,    \
                                                 float *__restrict__ grad_input, unsigned long long *__restrict__ ws, \
                                                 float *__restrict__ loss_out, int S, int H, int W)                   \
    {                                                                                                                 \
        photo_loss_body<WITH_GRAD, EARLY, HEAD, true>(input, photos, scenes, xrow, eps, inv_count, loss_scale,        \
                                                      fixed_scale, grad_input, ws, loss_out, S, H, W, weights,        \
                                                      weight_planes);                                                 \
    }
#define SVBRDF_WPHOTO_KERNEL_INL(NAME, HEAD)                                                                          \
    template <bool WITH_GRAD>                                                                                         \
    __global__ SVBRDF_PHOTO_LOSS_ATTRS void NAME([[maybe_unused]] const SceneBlock table,                             \
                                                 const float *__restrict__ input, const float *__restrict__ photos,   \
                                                 const float *__restrict__ weights, int weight_planes,                \
                                                 const float *__restrict__ xrow, float eps, float inv_count,          \
                                                 double loss_scale, float fixed_scale,                                \
                                                 float *__restrict__ grad_input, unsigned long long *__restrict__ ws, \
                                                 float *__restrict__ loss_out, int S, int H, int W)                   \
    {                                                                                                                 \
        const float *__restrict__ rows = (const float *)__builtin_amdgcn_kernarg_segment_ptr();                       \
        photo_loss_body<WITH_GRAD, true, HEAD, true>(input, photos, rows, xrow, eps, inv_count, loss_scale,           \
                                                     fixed_scale, grad_input, ws, loss_out, S, H, W, weights,         \
                                                     weight_planes);                                                  \
    }
SVBRDF_WPHOTO_KERNEL(k_wphoto, false, false)
SVBRDF_WPHOTO_KERNEL_INL(k_wphoto_inl, false)
SVBRDF_WPHOTO_KERNEL(k_head_wphoto, false, true)
SVBRDF_WPHOTO_KERNEL_INL(k_head_wphoto_inl, true)
#undef SVBRDF_WPHOTO_KERNEL
#undef SVBRDF_WPHOTO_KERNEL_INL

// One launcher for the sixteen kernels: the table by value (`rows`) or in device memory, `weights, weight_planes` for the
// weighted kernels only, the tail from `xrow` on common to all.
template <bool G, bool HEAD, bool WEIGHTED>
void launch_photo(const float *rows, dim3 grid, size_t lds_bytes, hipStream_t st, const float *input, const float *photos,
                  const float *weights, int weight_planes, const float *scenes, const float *xrow, float eps,
                  float inv_count, double loss_scale, float fixed_scale, float *grad_input, unsigned long long *ws,
                  float *loss_out, int B, int S, int H, int W)
{
    const auto launch = [&](auto kernel, const auto &...front) {
        hipLaunchKernelGGL(kernel, grid, dim3(kLossThreads), lds_bytes, st, front..., xrow, eps, inv_count, loss_scale,
                           fixed_scale, grad_input, ws, loss_out, S, H, W);
    };
    if (rows) {
        SceneBlock block_arg;      // only the first B*S rows are ever read
        std::memcpy(block_arg.v, rows, (size_t)B * S * 9 * sizeof(float));
        if constexpr (WEIGHTED)
            launch(HEAD ? k_head_wphoto_inl<G> : k_wphoto_inl<G>, block_arg, input, photos, weights, weight_planes);
        else
            launch(HEAD ? k_head_photo_inl<G> : k_photo_loss_inl<G>, block_arg, input, photos);
    } else {
        if constexpr (WEIGHTED)
            launch(HEAD ? k_head_wphoto<G> : k_wphoto<G>, input, photos, weights, weight_planes, scenes);
        else
            launch(HEAD ? k_head_photo<G> : k_photo_loss<G>, input, photos, scenes);
    }
}

// Argument checks, grid and fixed-point scale: K3's own (plan_loss in svbrdf_host.h; no L1 term here).  The launch
// is counted by the main unit's counter through launch_status() (svbrdf_internal_launch_status).
// `head`: input and grad_input are the 9 encoded planes (svbrdf_head_photo_loss_fwd_bwd*), same checks.
// `weighted`: the same plan (a weight in [0, 1] keeps a term within plan_loss's bound of 32, so the fixed-point scale
// stands), `weights` among the required pointers, `weight_planes` 1 or S -- all before any launch.
int photo_impl(const char *who, bool scenes_on_host, bool head, bool weighted, const float *input, const float *photos,
               const float *weights, int weight_planes, const float *scenes, const float *xrow, float eps, float *loss_out,
               float *grad_input, void *workspace, size_t workspace_bytes, int B, int S, int H, int W, void *stream)
{
    using Required = std::initializer_list<const void *>;
    LossPlan p;
    if (int e = plan_loss(who, scenes_on_host,
                          weighted ? Required{input, photos, weights, scenes, xrow, loss_out}
                                   : Required{input, photos, scenes, xrow, loss_out},
                          grad_input, workspace, workspace_bytes, "eps", eps, 0.0f, B, S, H, W, &p)) return e;
    // (the weighted entries' weights passed plan_loss, non-null and aligned; the others pass none and 0 planes)
    if (int e = weights_check(who, weights, weight_planes, S, "weight_planes must be 1 (one plane per item) or S (one per photo)"))
        return e;
    static constexpr decltype(&launch_photo<false, false, false>) kLaunch[2][2][2] = {     // [weighted][head][gradient]
        {{launch_photo<false, false, false>, launch_photo<true, false, false>},
         {launch_photo<false, true, false>, launch_photo<true, true, false>}},
        {{launch_photo<false, false, true>, launch_photo<true, false, true>},
         {launch_photo<false, true, true>, launch_photo<true, true, true>}}};
    kLaunch[weighted][head][grad_input != nullptr](
        scenes_on_host ? scenes : nullptr, p.grid, p.lds_bytes, static_cast<hipStream_t>(stream), input, photos, weights,
        weight_planes, scenes, xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale, grad_input, p.ws, loss_out, B, S, H, W);
    return launch_status(who);
}

}  // namespace

extern "C" {

// Per-pixel confidence weights (added to ABI version 8 without a bump: see include/svbrdf_hip.h)
int svbrdf_photo_loss_weighted_fwd_bwd(const float *input, const float *photos, const float *weights, int weight_planes,
                                       const float *scenes, const float *xrow, float eps, float *loss_out,
                                       float *grad_input, void *workspace, size_t workspace_bytes, int B, int S, int H,
                                       int W, void *stream)
{
    return photo_impl("photo_loss_weighted", false, false, true, input, photos, weights, weight_planes, scenes, xrow, eps,
                       loss_out, grad_input, workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_photo_loss_weighted_fwd_bwd_host_scenes(const float *input, const float *photos, const float *weights,
                                                   int weight_planes, const float *scenes_host, const float *xrow,
                                                   float eps, float *loss_out, float *grad_input, void *workspace,
                                                   size_t workspace_bytes, int B, int S, int H, int W, void *stream)
{
    return photo_impl("photo_loss_weighted_host_scenes", true, false, true, input, photos, weights, weight_planes, scenes_host,
                       xrow, eps, loss_out, grad_input, workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_head_photo_loss_weighted_fwd_bwd(const float *encoded9, const float *photos, const float *weights,
                                            int weight_planes, const float *scenes, const float *xrow, float eps,
                                            float *loss_out, float *grad_encoded9, void *workspace, size_t workspace_bytes,
                                            int B, int S, int H, int W, void *stream)
{
    return photo_impl("head_photo_loss_weighted", false, true, true, encoded9, photos, weights, weight_planes, scenes, xrow, eps,
                       loss_out, grad_encoded9, workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_head_photo_loss_weighted_fwd_bwd_host_scenes(const float *encoded9, const float *photos, const float *weights,
                                                        int weight_planes, const float *scenes_host, const float *xrow,
                                                        float eps, float *loss_out, float *grad_encoded9, void *workspace,
                                                        size_t workspace_bytes, int B, int S, int H, int W, void *stream)
{
    return photo_impl("head_photo_loss_weighted_host_scenes", true, true, true, encoded9, photos, weights, weight_planes,
                       scenes_host, xrow, eps, loss_out, grad_encoded9, workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_photo_loss_fwd_bwd(const float *input, const float *photos, const float *scenes, const float *xrow, float eps,
                              float *loss_out, float *grad_input, void *workspace, size_t workspace_bytes, int B, int S,
                              int H, int W, void *stream)
{
    return photo_impl("photo_loss", false, false, false, input, photos, nullptr, 0, scenes, xrow, eps, loss_out, grad_input,
                      workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_photo_loss_fwd_bwd_host_scenes(const float *input, const float *photos, const float *scenes_host,
                                          const float *xrow, float eps, float *loss_out, float *grad_input,
                                          void *workspace, size_t workspace_bytes, int B, int S, int H, int W, void *stream)
{
    return photo_impl("photo_loss_host_scenes", true, false, false, input, photos, nullptr, 0, scenes_host, xrow, eps, loss_out,
                      grad_input, workspace, workspace_bytes, B, S, H, W, stream);
}

// The network head folded in (added to ABI version 8 without a bump: see include/svbrdf_hip.h)
int svbrdf_head_photo_loss_fwd_bwd(const float *encoded9, const float *photos, const float *scenes, const float *xrow,
                                   float eps, float *loss_out, float *grad_encoded9, void *workspace,
                                   size_t workspace_bytes, int B, int S, int H, int W, void *stream)
{
    return photo_impl("head_photo_loss", false, true, false, encoded9, photos, nullptr, 0, scenes, xrow, eps, loss_out,
                      grad_encoded9, workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_head_photo_loss_fwd_bwd_host_scenes(const float *encoded9, const float *photos, const float *scenes_host,
                                               const float *xrow, float eps, float *loss_out, float *grad_encoded9,
                                               void *workspace, size_t workspace_bytes, int B, int S, int H, int W,
                                               void *stream)
{
    return photo_impl("head_photo_loss_host_scenes", true, true, false, encoded9, photos, nullptr, 0, scenes_host, xrow, eps,
                      loss_out, grad_encoded9, workspace, workspace_bytes, B, S, H, W, stream);
}

}  // extern "C"
